"""Lens distortion without a GPU: the host entry points (rsac_undistort_points,
rsac_project_points_dist -- rsac_math.h's functions, the source the kernels run) against the
NumPy restatement of the contract (tests/distref.py), bit for bit, and the cv2 shims.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import distref as D  # noqa: E402
import pyoracle as O  # noqa: E402
import rsac  # noqa: E402
import rsac.cv2compat as cv  # noqa: E402
from rsac import synth  # noqa: E402


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _pixels(n, seed):
    """pixels inside and well outside the 2142 x 1620 image"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-600.0, synth.IMAGE_W + 600.0, n), rng.uniform(-500.0, synth.IMAGE_H + 500.0, n)], 1)


@pytest.mark.parametrize("dist", [D.D5, D.D8, D.D5[:4]], ids=["D5", "D8", "D4"])
def test_host_undistort_matches_restatement_bitwise(dist):
    K = synth.main_v1_K()
    cam = O.cam_from_K(K)
    px = _pixels(1000, 21)
    u = px.astype(np.float32).astype(np.float64)
    x, y, _ = D.undistort(cam, dist, u[:, 0], u[:, 1])
    norm = rsac.undistort_points(px, K, dist)
    assert norm.dtype == np.float64 and norm.shape == (1000, 2)
    assert _bits_equal(norm, np.stack([x, y], 1))
    Uu, Vu = D.ideal_pixels(cam, dist, u[:, 0], u[:, 1])
    ideal = rsac.undistort_points(px, K, dist, ideal=True)
    assert ideal.dtype == np.float32
    assert _bits_equal(ideal, np.stack([Uu, Vu], 1))
    # five rounds of the fixed point land on the distorted pixel again (moderate distortion, in the image)
    inside = (px[:, 0] > 0) & (px[:, 0] < synth.IMAGE_W) & (px[:, 1] > 0) & (px[:, 1] < synth.IMAGE_H)
    back = rsac.project_points(np.stack([x, y, np.ones_like(x)], 1), K, dist, np.eye(3), np.zeros(3))
    assert np.abs(back - u)[inside].max() < 0.05


@pytest.mark.parametrize("dist", [D.D5, D.D8, D.D5[:4]], ids=["D5", "D8", "D4"])
def test_host_project_matches_restatement_bitwise(dist):
    pr = synth.pnp_problem(1000, 0.0, seed=9, noise_px=0.0)
    p3 = pr["points3d"].copy()
    p3[::50] += 400.0 * np.random.default_rng(3).normal(size=(20, 3))  # some land outside the image / behind
    cam = O.cam_from_K(pr["K"])
    pu, pv = D.project(pr["R"], pr["t"], cam, dist, p3[:, 0], p3[:, 1], p3[:, 2])
    got = rsac.project_points(p3, pr["K"], dist, pr["R"], pr["t"])
    assert _bits_equal(got, np.stack([pu, pv], 1))
    # a Rodrigues vector is accepted like a matrix
    rv = rsac.rodrigues(pr["R"])
    assert _bits_equal(rsac.project_points(p3, pr["K"], dist, rv, pr["t"]),
                       rsac.project_points(p3, pr["K"], dist, rsac.rodrigues(rv), pr["t"]))


def test_project_without_distortion_is_the_pinhole_projection():
    pr = synth.pnp_problem(300, 0.0, seed=2, noise_px=0.0)
    a = rsac.project_points(pr["points3d"], pr["K"], None, pr["R"], pr["t"])
    b = rsac.project_points(pr["points3d"], pr["K"], np.zeros(5), pr["R"], pr["t"])
    assert _bits_equal(a, b)
    ref = O.reproj_errors(pr["points3d"], pr["points2d"], pr["K"], pr["R"], pr["t"], projections=True)[1]
    assert _bits_equal(a, ref)


def test_negative_icd_exit_returns_the_start_point():
    K = synth.main_v1_K()
    cam = O.cam_from_K(K)
    dist = (-5.0, 0.0, 0.0, 0.0)
    # far from the centre: 1 + k1 r2 < 0 on the first round; near the centre: the ordinary iteration
    px = np.array([[synth.IMAGE_W - 5.0, synth.IMAGE_H - 5.0], [K[0, 2] + 30.0, K[1, 2] - 20.0]])
    u = px.astype(np.float32).astype(np.float64)
    x, y, took = D.undistort(cam, dist, u[:, 0], u[:, 1])
    assert took.tolist() == [True, False]
    x0 = (u[:, 0] - cam[2]) * (1.0 / cam[0])
    y0 = (u[:, 1] - cam[3]) * (1.0 / cam[1])
    got = rsac.undistort_points(px, K, dist)
    assert got[0, 0] == x0[0] and got[0, 1] == y0[0]
    assert _bits_equal(got, np.stack([x, y], 1))
    assert (got[1, 0], got[1, 1]) != (x0[1], y0[1])


def test_shims_shapes_and_values():
    pr = synth.pnp_problem(200, 0.0, seed=4, noise_px=0.0)
    cam = O.cam_from_K(pr["K"])
    d5 = np.array(D.D5).reshape(5, 1)
    rvec = rsac.rodrigues(pr["R"]).reshape(3, 1)
    R = rsac.rodrigues(rvec)  # projectPoints goes through Rodrigues(rvec)
    proj, jac = cv.projectPoints(pr["points3d"], rvec, pr["t"].reshape(3, 1), pr["K"], d5)
    assert jac is None and proj.shape == (200, 1, 2) and proj.dtype == np.float64
    p3 = pr["points3d"]
    pu, pv = D.project(R, pr["t"], cam, D.D5, p3[:, 0], p3[:, 1], p3[:, 2])
    assert _bits_equal(proj.reshape(-1, 2), np.stack([pu, pv], 1))
    und = cv.undistortPoints(proj, pr["K"], d5)
    assert und.shape == (200, 1, 2) and und.dtype == np.float64
    u = proj.reshape(-1, 2).astype(np.float32).astype(np.float64)
    x, y, _ = D.undistort(cam, D.D5, u[:, 0], u[:, 1])
    assert _bits_equal(und.reshape(-1, 2), np.stack([x, y], 1))
    # P = K: the ideal pixels in f64; identity R accepted, another R is not built
    und_px = cv.undistortPoints(proj.reshape(-1, 2), pr["K"], d5, R=np.eye(3), P=pr["K"])
    np.testing.assert_array_equal(und_px.reshape(-1, 2), np.stack([x * cam[0] + cam[2], y * cam[1] + cam[3]], 1))
    assert cv.undistortPoints(proj.astype(np.float32), pr["K"], d5).dtype == np.float32
    with pytest.raises(NotImplementedError):
        cv.undistortPoints(proj, pr["K"], d5, R=rsac.rodrigues(np.array([0.1, 0.0, 0.0])))


@pytest.mark.parametrize("k", [12, 14])
def test_thin_prism_and_tilt_lengths_are_not_implemented(k):
    pr = synth.pnp_problem(20, 0.0, seed=1, noise_px=0.0)
    d = np.full(k, 1e-3)
    with pytest.raises(NotImplementedError):
        cv.undistortPoints(pr["points2d"], pr["K"], d)
    with pytest.raises(NotImplementedError):
        cv.projectPoints(pr["points3d"], np.zeros(3), pr["t"], pr["K"], d)
    with pytest.raises(NotImplementedError):
        cv.solvePnPRansac(pr["points3d"], pr["points2d"], pr["K"], d)
    with pytest.raises(NotImplementedError):
        cv.solvePnPRefineLM(pr["points3d"], pr["points2d"], pr["K"], d, np.zeros(3), pr["t"])
    with pytest.raises(NotImplementedError):
        rsac.undistort_points(pr["points2d"], pr["K"], d)
    # the C entry points refuse them too, with a message
    from rsac import _lib as L
    out = np.zeros((20, 2))
    p2 = np.ascontiguousarray(pr["points2d"])
    K9 = np.ascontiguousarray(pr["K"].reshape(9))
    assert L.lib().rsac_undistort_points(p2.ctypes.data, 20, K9.ctypes.data, d.ctypes.data, k, out.ctypes.data,
                                         None) == L.EINVAL
    assert b"not supported" in L.lib().rsac_last_error()
    assert L.lib().rsac_undistort_points(p2.ctypes.data, 20, K9.ctypes.data, d.ctypes.data, 7, out.ctypes.data,
                                         None) == L.EINVAL


def test_combinations_not_built_name_themselves():
    pr = synth.pnp_problem(20, 0.0, seed=1, noise_px=0.0)
    with pytest.raises(NotImplementedError, match="pnp_ransac_batched"):
        rsac.pnp_ransac_batched([pr["points2d"]], [pr["points3d"]], [pr["K"]], dist=D.D5)
    with pytest.raises(NotImplementedError, match="estimate_camera_orientation"):
        rsac.estimate_camera_orientation(pr["points3d"], pr["points2d"], [240.0], [(127.0, 178.0)],
                                         (synth.IMAGE_W, synth.IMAGE_H), dist=D.D5)
    with pytest.raises(ValueError):
        rsac.undistort_points(pr["points2d"], pr["K"], np.ones(6))


def test_zero_or_missing_distortion_is_todays_output():
    pr = synth.pnp_problem(500, 0.0, seed=5, noise_px=0.5)
    t0 = pr["t"] + np.array([0.5, -0.3, 0.2])
    R, t = rsac.refine_pose(pr["points2d"], pr["points3d"], pr["K"], pr["R"], t0)
    for d in (None, np.zeros((4, 1)), np.zeros(5), np.zeros(8), np.zeros(14)):
        Rd, td = rsac.refine_pose(pr["points2d"], pr["points3d"], pr["K"], pr["R"], t0, dist=d)
        np.testing.assert_array_equal(Rd, R)
        np.testing.assert_array_equal(td, t)
    # undistortion without coefficients is the normalisation
    cam = O.cam_from_K(pr["K"])
    u = pr["points2d"].astype(np.float32).astype(np.float64)
    und = cv.undistortPoints(pr["points2d"], pr["K"], None).reshape(-1, 2)
    np.testing.assert_array_equal(und, np.stack([(u[:, 0] - cam[2]) * (1.0 / cam[0]),
                                                 (u[:, 1] - cam[3]) * (1.0 / cam[1])], 1))
    np.testing.assert_array_equal(cv.undistortPoints(pr["points2d"], pr["K"], np.zeros((5, 1))).reshape(-1, 2), und)


def test_refine_with_distortion_is_the_refit_on_ideal_pixels():
    pr = D.distorted_problem(333, 0.0, 4, D.D5)
    soa, soa_i, cam = D.soa_pair(pr["points3d"], pr["points2d"], pr["K"], D.D5)
    t0 = pr["t"] + np.array([0.5, -0.3, 0.2])
    R, t = rsac.refine_pose(pr["points2d"], pr["points3d"], pr["K"], pr["R"], t0, dist=D.D5)
    Ro, to, _ = O.pnp_refine(soa_i, np.ones(333, np.uint8), cam, pr["R"], t0)
    np.testing.assert_array_equal(R, Ro)
    np.testing.assert_array_equal(t, to)
    # and it is a good pose of the distorted camera: the true inliers reproject within a pixel
    e = np.sqrt(D.err2(R, t, cam, D.D5, soa))
    assert np.median(e) < 1.0
