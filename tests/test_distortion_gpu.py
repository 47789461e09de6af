"""Lens distortion on the GPU: every comparison is exact equality with the reference chain of
tests/distref.py -- the unchanged CPU oracle on the restated ideal pixels for models, status,
scan and refit; the NumPy restatement of the distorted test on the raw pixels for counts and
masks.  Data: distref.distorted_problem (the project's synthetic scene seen through the lens),
8 px threshold, seed 0x5EED.
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

pytestmark = pytest.mark.gpu

THR, SEED = 8.0, 0x5EED
DISTS = {"D5": D.D5, "D8": D.D8}
# (n, outlier ratio, seed): the five inputs whose chain results were checked on the CPU
FIVE = [(12, .25, 5), (64, .3, 7), (333, .5, 4), (2000, .4, 3), (4097, .5, 8)]
# expected RANSAC-phase counts / iterations of the chain for D5 and D8 (CPU runs of the chain)
FIVE_COUNTS = {"D5": [9, 45, 167, 1200, 2050], "D8": [9, 45, 167, 1200, 2049]}
FIVE_ITERS = [12, 16, 70, 33, 71]


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


# n: below one wave, one wave, both sides of kLanePts (256), no multiple of the 512-point tile, several
# tiles per wave; H = 512 is a multiple of the block's 32 hypotheses, 5000 is not
@pytest.mark.parametrize("dn", ["D5", "D8"])
@pytest.mark.parametrize("n,outl,seed", [(12, .25, 5), (64, .3, 7), (256, .5, 8), (257, .5, 8), (333, .5, 4),
                                         (4097, .5, 8)])
def test_hypotheses_exhaustive(n, outl, seed, dn):
    dist = DISTS[dn]
    pr = D.distorted_problem(n, outl, seed, dist)
    st, cnt, mdl = rsac.hypotheses("pnp", pr["points3d"], pr["points2d"], pr["K"], 0, 512, THR, seed=SEED, dist=dist)
    rs, rc, rm = D.hypotheses(pr["points3d"], pr["points2d"], pr["K"], dist, THR, SEED, 512)
    np.testing.assert_array_equal(st, rs)
    assert _bits_equal(mdl[:, :12], rm[:, :12])
    np.testing.assert_array_equal(cnt, rc)
    assert rc.max() > 4  # the table holds real models of the distorted scene


def test_hypotheses_h_not_a_multiple_of_the_block():
    pr = D.distorted_problem(1000, .5, 5, D.D5)
    st, cnt, mdl = rsac.hypotheses("pnp", pr["points3d"], pr["points2d"], pr["K"], 0, 5000, THR, seed=SEED,
                                   dist=D.D5)
    rs, rc, rm = D.hypotheses(pr["points3d"], pr["points2d"], pr["K"], D.D5, THR, SEED, 5000)
    np.testing.assert_array_equal(st, rs)
    assert _bits_equal(mdl[:, :12], rm[:, :12])
    np.testing.assert_array_equal(cnt, rc)


@pytest.mark.parametrize("dn", ["D5", "D8"])
def test_undistort_device_equals_host(dn):
    import torch
    dist = DISTS[dn]
    pr = D.distorted_problem(4097, .5, 8, dist)
    for ideal in (False, True):
        host = rsac.undistort_points(pr["points2d"], pr["K"], dist, ideal=ideal)
        dev = rsac.undistort_points(pr["points2d"], pr["K"], dist, ideal=ideal, device=0)
        assert dev.dtype == host.dtype
        np.testing.assert_array_equal(dev.view(np.uint8), host.view(np.uint8))
        t = rsac.undistort_points(torch.as_tensor(pr["points2d"].copy(), device="cuda"), pr["K"], dist, ideal=ideal)
        assert t.is_cuda
        np.testing.assert_array_equal(t.cpu().numpy().view(np.uint8), host.view(np.uint8))


@pytest.mark.parametrize("dn", ["D5", "D8"])
@pytest.mark.parametrize("case", range(5))
def test_pnp_ransac_equals_chain(case, dn):
    n, outl, seed = FIVE[case]
    dist = DISTS[dn]
    pr = D.distorted_problem(n, outl, seed, dist)
    ref = D.ransac_case(n, outl, seed, dist)
    R, t, mask, info = rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 5000, THR, seed=SEED, dist=dist,
                                       return_info=True)
    assert R is not None
    assert (info.best_hyp, info.iters, info.n_inliers) == (ref["best"], ref["iters"], ref["n_inliers"])
    np.testing.assert_array_equal(mask, ref["mask"])
    assert _bits_equal(R, ref["R"]) and _bits_equal(t, ref["t"])
    assert info.score_ms > 0.0  # the new scorer is what score_ms times
    # without the refit: the winner's record
    R0, t0, mask0, info0 = rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 5000, THR, seed=SEED, dist=dist,
                                           refine=False, return_info=True)
    assert info0.best_hyp == ref["best"]
    np.testing.assert_array_equal(mask0, ref["mask"])
    assert _bits_equal(R0, ref["R0"]) and _bits_equal(t0, ref["t0"])
    # ground truth (checked on the CPU for these inputs): every true inlier is found, and the pinhole
    # call on the same raw pixels finds strictly fewer
    assert (info.n_inliers, info.iters) == (FIVE_COUNTS[dn][case], FIVE_ITERS[case])
    assert np.all(np.asarray(mask)[pr["inlier"]])
    _, _, _, pin = rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 5000, THR, seed=SEED, return_info=True)
    assert info.n_inliers > pin.n_inliers


def test_scan_leaves_the_first_round():
    pr = D.distorted_problem(500, .8, 11, D.D5)
    ref = D.ransac_case(500, .8, 11, D.D5)
    assert ref["iters"] > 256
    R, t, mask, info = rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 5000, THR, seed=SEED, dist=D.D5,
                                       return_info=True)
    assert (info.best_hyp, info.iters, info.n_inliers) == (ref["best"], ref["iters"], ref["n_inliers"])
    assert info.rounds > 1
    np.testing.assert_array_equal(mask, ref["mask"])
    assert _bits_equal(R, ref["R"]) and _bits_equal(t, ref["t"])


def test_epnp_final_solve_and_direct_branch_run_on_ideal_pixels():
    pr = D.distorted_problem(333, .5, 4, D.D5)
    ref = D.ransac_case(333, .5, 4, D.D5)
    _, soa_i, cam = D.soa_pair(pr["points3d"], pr["points2d"], pr["K"], D.D5)
    m8 = ref["mask"].astype(np.uint8)
    Ro, to = O.pnp_epnp(soa_i, m8, cam)
    R, t, m = rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 5000, THR, dist=D.D5, refine="epnp")
    np.testing.assert_array_equal(m, ref["mask"])
    assert _bits_equal(R, Ro) and _bits_equal(t, to)
    Rl, tl, _ = O.pnp_refine(soa_i, m8, cam, Ro, to)
    R2, t2, _ = rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 5000, THR, dist=D.D5, refine="epnp+lm")
    assert _bits_equal(R2, Rl) and _bits_equal(t2, tl)
    # 4 correspondences: solvePnPRansac's count == model_points branch (one minimal solve on all the
    # points, every index an inlier, no final solve), solved on the ideal pixels
    idx = np.flatnonzero(pr["inlier"])[:4]
    p3, p2 = pr["points3d"][idx], pr["points2d"][idx]
    _, sub_i, _ = D.soa_pair(p3, p2, pr["K"], D.D5)
    want = O.pnp_minimal(sub_i, np.arange(4), cam)
    R4, t4, m4, info = rsac.pnp_ransac(p2, p3, pr["K"], 5000, THR, dist=D.D5, return_info=True)
    assert want is not None and R4 is not None
    assert _bits_equal(R4, want[0]) and _bits_equal(t4, want[1])
    assert m4.all() and info.n_inliers == 4 and info.iters == 0


def test_reference_mode_hypotheses_and_shim():
    n = 333
    pr = D.distorted_problem(n, .5, 4, D.D5)
    subs, sst = O.mwc_subsets(n, 512, s=5)
    st, cnt, mdl = rsac.hypotheses("pnp", pr["points3d"], pr["points2d"], pr["K"], 0, 512, THR, subsets=subs,
                                   minimal="epnp5", dist=D.D5)
    rs, rc, rm = D.hypotheses(pr["points3d"], pr["points2d"], pr["K"], D.D5, THR, 0, 512, subsets=subs,
                              sub_status=sst, minimal="epnp5")
    np.testing.assert_array_equal(st, rs)
    assert _bits_equal(mdl[:, :12], rm[:, :12])
    np.testing.assert_array_equal(cnt, rc)
    # cv2.solvePnPRansac's defaults: 100 iterations, 8 px, 0.99; SOLVEPNP_ITERATIVE = 5-point EPnP
    # samples, models through the rvec round trip, LM from the best model as the final solve
    ref = D.ransac(pr["points3d"], pr["points2d"], pr["K"], D.D5, THR, 0, 100, reference_mode=True)
    ok, rvec, tvec, inl = cv.solvePnPRansac(pr["points3d"], pr["points2d"], pr["K"], np.array(D.D5).reshape(5, 1))
    assert ok and rvec.shape == (3, 1) and tvec.shape == (3, 1) and inl.dtype == np.int32 and inl.shape[1] == 1
    np.testing.assert_array_equal(inl[:, 0], np.flatnonzero(ref["mask"]))
    assert _bits_equal(tvec.ravel(), ref["t"])
    assert _bits_equal(rsac.rodrigues(rvec), rsac.rodrigues(rsac.rodrigues(ref["R"])))
    # solvePnPRefineLM through the shim: undistort, then the LM on the ideal pixels
    idx = inl[:, 0]
    r2, t2 = cv.solvePnPRefineLM(pr["points3d"][idx], pr["points2d"][idx], pr["K"], np.array(D.D5), rvec, tvec)
    _, sub_i, cam = D.soa_pair(pr["points3d"][idx], pr["points2d"][idx], pr["K"], D.D5)
    Ro, to, _ = O.pnp_refine(sub_i, np.ones(len(idx), np.uint8), cam, rsac.rodrigues(rvec), tvec.ravel())
    assert _bits_equal(t2.ravel(), to)
    assert _bits_equal(rsac.rodrigues(r2), rsac.rodrigues(rsac.rodrigues(Ro)))


def _poses(pr, n_poses=64):
    """the true pose, perturbed copies, and poses that put points behind the camera"""
    rng = np.random.default_rng(77)
    poses = np.zeros((n_poses, 12))
    for i in range(n_poses):
        dR = rsac.rodrigues(rng.normal(0.0, 1e-3 * i, 3)) if i else np.eye(3)
        R = dR @ pr["R"]
        t = dR @ pr["t"] + (rng.normal(0.0, 0.05 * i, 3) if i else 0.0)
        if i % 16 == 15:  # half a turn about the camera's x axis: every point behind the camera
            F = np.diag([1.0, -1.0, -1.0])
            R, t = F @ R, F @ t
        poses[i, :9], poses[i, 9:] = R.reshape(9), t
    return poses


@pytest.mark.parametrize("dn", ["D5", "D8"])
def test_score_poses_mask_and_reprojection_against_numpy(dn):
    dist = DISTS[dn]
    pr = D.distorted_problem(333, .5, 4, dist)
    soa, _, cam = D.soa_pair(pr["points3d"], pr["points2d"], pr["K"], dist)
    poses = _poses(pr)
    t2 = np.float32(O.thr2(THR))
    ref_masks = [D.err2(p[:9], p[9:], cam, dist, soa) <= t2 for p in poses]
    counts = rsac.score_poses(pr["points2d"], pr["points3d"], pr["K"], poses, THR, dist=dist)
    np.testing.assert_array_equal(counts, [int(m.sum()) for m in ref_masks])
    assert counts[0] == int(pr["inlier"].sum()) and counts[15] < counts[0]
    for i in (0, 1, 15, 40):
        m, c = rsac.pose_mask(pr["points2d"], pr["points3d"], pr["K"], poses[i], THR, dist=dist)
        np.testing.assert_array_equal(m, ref_masks[i])
        assert c == int(ref_masks[i].sum())
    for i in (0, 15):
        proj, err = D.reproj(poses[i, :9], poses[i, 9:], cam, dist, pr["points3d"], pr["points2d"])
        e, p = rsac.reprojection_errors(pr["points3d"], pr["points2d"], pr["K"], poses[i, :9].reshape(3, 3),
                                        poses[i, 9:], return_projection=True, dist=dist)
        assert _bits_equal(p, proj) and _bits_equal(e, err)
    e2 = rsac.compute_reprojection_error(pr["points3d"], pr["points2d"], pr["K"], np.array(dist),
                                         rsac.rodrigues(pr["R"]), pr["t"])
    Rr = rsac.rodrigues(rsac.rodrigues(pr["R"]))
    assert _bits_equal(e2, D.reproj(Rr, pr["t"], cam, dist, pr["points3d"], pr["points2d"])[1])


def test_device_tensors_give_the_host_outputs():
    import torch
    pr = D.distorted_problem(2000, .4, 3, D.D5)
    d3 = torch.as_tensor(pr["points3d"].copy(), device="cuda")
    d2 = torch.as_tensor(pr["points2d"].copy(), device="cuda")
    R, t, mask, info = rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 5000, THR, dist=D.D5,
                                       return_info=True)
    Rd, td, maskd, infod = rsac.pnp_ransac(d2, d3, pr["K"], 5000, THR, dist=D.D5, return_info=True)
    assert maskd.is_cuda
    assert (infod.best_hyp, infod.iters, infod.n_inliers) == (info.best_hyp, info.iters, info.n_inliers)
    np.testing.assert_array_equal(maskd.cpu().numpy(), mask)
    assert _bits_equal(Rd, R) and _bits_equal(td, t)
    h = rsac.hypotheses("pnp", pr["points3d"], pr["points2d"], pr["K"], 0, 300, THR, dist=D.D5)
    hd = rsac.hypotheses("pnp", d3, d2, pr["K"], 0, 300, THR, dist=D.D5)
    for a, b in zip(h, hd):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    poses = _poses(pr, 8)
    np.testing.assert_array_equal(rsac.score_poses(d2, d3, pr["K"], poses, THR, dist=D.D5),
                                  rsac.score_poses(pr["points2d"], pr["points3d"], pr["K"], poses, THR, dist=D.D5))
    m, c = rsac.pose_mask(pr["points2d"], pr["points3d"], pr["K"], poses[0], THR, dist=D.D5)
    md, cd = rsac.pose_mask(d2, d3, pr["K"], poses[0], THR, dist=D.D5)
    assert cd == c
    np.testing.assert_array_equal(md.cpu().numpy(), m)
    e = rsac.reprojection_errors(pr["points3d"], pr["points2d"], pr["K"], pr["R"], pr["t"], dist=D.D5)
    ed = rsac.reprojection_errors(d3, d2, pr["K"], pr["R"], pr["t"], dist=D.D5)
    assert ed.is_cuda and _bits_equal(ed.cpu().numpy(), e)


def test_zero_distortion_is_the_call_without_it():
    pr = D.distorted_problem(2000, .4, 3, D.D5)
    zeros = np.zeros(5)
    a = rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 5000, THR, return_info=True)
    b = rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 5000, THR, dist=zeros, return_info=True)
    assert _bits_equal(a[0], b[0]) and _bits_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2], b[2])
    assert (a[3].best_hyp, a[3].iters, a[3].n_inliers) == (b[3].best_hyp, b[3].iters, b[3].n_inliers)
    h = rsac.hypotheses("pnp", pr["points3d"], pr["points2d"], pr["K"], 0, 300, THR)
    hz = rsac.hypotheses("pnp", pr["points3d"], pr["points2d"], pr["K"], 0, 300, THR, dist=zeros)
    for x, y in zip(h, hz):
        np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))
    poses = _poses(pr, 8)
    np.testing.assert_array_equal(rsac.score_poses(pr["points2d"], pr["points3d"], pr["K"], poses, THR),
                                  rsac.score_poses(pr["points2d"], pr["points3d"], pr["K"], poses, THR, dist=zeros))
    # ... down to the C entry points, which delegate
    from rsac import _lib as L
    ctx = L.context(0)
    p3 = np.ascontiguousarray(pr["points3d"])
    p2 = np.ascontiguousarray(pr["points2d"])
    K9 = np.ascontiguousarray(pr["K"].reshape(9))
    R, t, m = np.zeros(9), np.zeros(3), np.zeros(2000, np.uint8)
    with ctx.lock:
        code = L.lib().rsac_pnp_ransac_dist(ctx.handle, p3.ctypes.data, p2.ctypes.data, 2000, K9.ctypes.data,
                                            zeros.ctypes.data, 5, 5000, THR, 0.99, SEED, L.F_ADAPTIVE | L.F_REFINE,
                                            R.ctypes.data, t.ctypes.data, m.ctypes.data, None, None)
        assert code == L.OK
        d5 = np.array(D.D5)
        bad = L.lib().rsac_pnp_ransac_dist(ctx.handle, p3.ctypes.data, p2.ctypes.data, 2000, K9.ctypes.data,
                                           d5.ctypes.data, 5, 5000, THR, 0.99, SEED, L.F_ADAPTIVE | L.F_LO,
                                           R.ctypes.data, t.ctypes.data, m.ctypes.data, None, None)
        assert bad == L.EINVAL and b"RSAC_F_LO" in L.lib().rsac_last_error()
    assert _bits_equal(R.reshape(3, 3), a[0]) and _bits_equal(t, a[1])
    np.testing.assert_array_equal(m.view(np.bool_), a[2])
    with pytest.raises(NotImplementedError, match="lo=True"):
        rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 5000, THR, dist=D.D5, lo=True)
