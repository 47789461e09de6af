"""What the drivers of rsac_api.hip report around their results: the rsac_stats of every driver,
rsac_last_stats under rsac_set_timing, the batched homography call against the single-problem one
(direct branch, device mask, refit), caller-supplied subsets with bad indices, and the error codes of
the shared argument checks.  The results themselves are pinned by test_gpu_parity.py, test_direct.py,
test_lmeds_gpu.py, test_msac_gpu.py and test_distortion_gpu.py; every comparison here is exact too,
but for gpu_ms == solve_ms + score_ms: the three are sums of the same float32 event times taken in
two orders (DESIGN.md "Driver helpers"), so they agree to a few ulps of a double per round.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lmedsref as M  # noqa: E402
import pyoracle as O  # noqa: E402
import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402
from rsac import api as A  # noqa: E402
from rsac import synth  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0x5EED


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


@functools.lru_cache(maxsize=None)
def _pnp(n, outl, seed):
    return synth.pnp_problem(n, outl, seed=seed)


@functools.lru_cache(maxsize=None)
def _hom(n, outl, seed):
    return synth.homography_problem(n, outl, seed=seed)


@functools.lru_cache(maxsize=None)
def _hom_ref(n, outl, seed):
    pr = _hom(n, outl, seed)
    return O.hom_ransac(pr["src"], pr["dst"], 3.0, 0.995, 2000, SEED, sampler="opencv")


# ---------------------------------------------------------------------------------------------
# 1. return_info of the four drivers
# ---------------------------------------------------------------------------------------------
def _check_info(info, mask, ref):
    assert (info.best_hyp, info.n_inliers, info.iters) == (ref["best"], ref["n_inliers"], ref["iters"])
    assert info.n_inliers == int(np.asarray(mask).sum())
    assert info.hyps_scored >= info.iters
    assert info.rounds >= 1
    assert math.isclose(info.gpu_ms, info.solve_ms + info.score_ms, rel_tol=1e-12, abs_tol=1e-12)
    assert info.lo_improvements == 0


def test_info_pnp_ransac():
    pr = _pnp(200, 0.3, 14)
    R, t, mask, info = rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 5000, 30.0, return_info=True)
    assert R is not None and info.ok
    _check_info(info, mask, O.pnp_ransac(pr["points3d"], pr["points2d"], pr["K"], 30.0, 0.99, 5000, SEED))


def test_info_homography_ransac():
    pr = _hom(64, 0.3, 6)
    H, mask, info = rsac.homography_ransac(pr["src"], pr["dst"], 3.0, return_info=True)
    assert H is not None and info.ok
    _check_info(info, mask, _hom_ref(64, 0.3, 6))


def test_info_homography_lmeds():
    pr = M.problem(64, 0.3, 164)
    H, mask, info = rsac.homography_lmeds(pr["src"], pr["dst"], return_info=True)
    assert H is not None and info.ok
    _check_info(info, mask, M.lmeds_case(64, 0.3, 164))


def test_info_fundamental_ransac():
    pr = synth.fundamental_problem(64, 0.3, seed=2)
    F, mask, info = rsac.fundamental_ransac(pr["pts1"], pr["pts2"], 1.5, max_iters=3000, return_info=True)
    assert F is not None and info.ok
    _check_info(info, mask, O.fm_ransac(pr["pts1"], pr["pts2"], 1.5, 0.99, 3000))


# ---------------------------------------------------------------------------------------------
# 2. rsac_set_timing + rsac_last_stats: the batched calls leave problem 0's figures, the
#    fundamental-matrix driver leaves the context's statistics alone
# ---------------------------------------------------------------------------------------------
def _check_last(st, ref, n_inliers):
    assert (st["best_hyp"], st["n_inliers"], st["iters"]) == (ref["best"], ref["n_inliers"], ref["iters"])
    assert st["n_inliers"] == n_inliers
    assert st["hyps_scored"] >= st["iters"] and st["rounds"] >= 1 and st["lo_improvements"] == 0
    assert st["gpu_ms"] > 0


def test_last_stats_of_batched_calls():
    ctx = L.context(0)
    pnp = [_pnp(50, 0.3, 6 + p) for p in range(3)]
    hom = [(40, 0.3, 30), (64, 0.3, 6), (30, 0.2, 32)]
    lmeds = [(64, 0.3, 164), (33, 0.3, 133), (12, 0.3, 112)]
    ctx.set_timing(True)
    try:
        out = rsac.pnp_ransac_batched([p["points2d"] for p in pnp], [p["points3d"] for p in pnp],
                                      [p["K"] for p in pnp], 5000, 30.0)
        _check_last(ctx.last_stats(), O.pnp_ransac(pnp[0]["points3d"], pnp[0]["points2d"], pnp[0]["K"], 30.0, 0.99,
                                                   5000, SEED), out[0][3])
        out = rsac.homography_ransac_batched([_hom(*k)["src"] for k in hom], [_hom(*k)["dst"] for k in hom], 3.0)
        _check_last(ctx.last_stats(), _hom_ref(*hom[0]), out[0][2])
        out = rsac.homography_lmeds_batched([M.problem(*k)["src"] for k in lmeds],
                                            [M.problem(*k)["dst"] for k in lmeds])
        before = ctx.last_stats()
        _check_last(before, M.lmeds_case(*lmeds[0]), out[0][2])
        pr = synth.fundamental_problem(64, 0.3, seed=2)
        F, _ = rsac.fundamental_ransac(pr["pts1"], pr["pts2"], 1.5, max_iters=3000)
        assert F is not None
        assert ctx.last_stats() == before
    finally:
        ctx.set_timing(False)


# ---------------------------------------------------------------------------------------------
# 3. batched RANSAC homography == the single-problem calls (4 points: the direct branch; 5 points
#    with refine: the smallest refit)
# ---------------------------------------------------------------------------------------------
BATCH = [(4, 0.0, 41), (12, 0.3, 42), (4, 0.0, 43), (33, 0.3, 44), (5, 0.0, 45)]


@pytest.mark.parametrize("refine", [True, False])
@pytest.mark.parametrize("device_mask", [True, False])
def test_homography_batched_equals_single_calls(device_mask, refine):
    import torch
    prs = [_hom(*k) for k in BATCH]
    s, off = A._concat([p["src"] for p in prs], 2)
    d, _ = A._concat([p["dst"] for p in prs], 2)
    P, N = len(prs), int(off[-1])
    H, status, ninl = np.zeros((P, 9)), np.full(P, -7, np.int32), np.full(P, -7, np.int32)
    flags = A._flags(True, refine, "opencv")
    if device_mask:
        mask = torch.full((N,), 7, dtype=torch.uint8, device="cuda")
        mptr, flags = mask.data_ptr(), flags | L.F_DEVICE_OUT
    else:
        mask = np.full(N, 7, np.uint8)
        mptr = mask.ctypes.data
    ctx = L.context(0)
    with ctx.lock:
        L.check(L.lib().rsac_homography_ransac_batched(ctx.handle, s.ctypes.data, d.ctypes.data, off.ctypes.data, P,
                                                       2000, 3.0, 0.995, SEED, flags, H.ctypes.data,
                                                       status.ctypes.data, ninl.ctypes.data, mptr, None))
    m = mask.cpu().numpy() if device_mask else mask
    assert set(np.unique(m)) <= {0, 1}
    for p, pr in enumerate(prs):
        H1, m1, info = rsac.homography_ransac(pr["src"], pr["dst"], 3.0, refine=refine, return_info=True)
        assert (status[p] == L.OK) == (H1 is not None)
        if H1 is not None:
            assert _bits_equal(H[p].reshape(3, 3), H1)
        np.testing.assert_array_equal(m[off[p]:off[p + 1]].astype(bool), m1)
        assert ninl[p] == info.n_inliers == int(m1.sum())
    assert status[0] == L.OK and ninl[0] == 4  # the direct model of four points in general position


# ---------------------------------------------------------------------------------------------
# 4. caller-supplied subsets with indices out of range
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("medians", [False, True])
def test_homography_subsets_with_bad_indices(medians):
    n, Hn = 33, 16
    pr = _hom(n, 0.3, 44)
    good, sst = O.mwc_subsets(n, Hn, 4, hom=O.soa_hom(pr["src"], pr["dst"]))
    assert (sst == 1).all()
    bad = np.array(good, np.int32)
    bad[3, 2] = n  # one past the last point
    bad[10, 0] = -1
    ref = rsac.hypotheses("homography", pr["src"], pr["dst"], n_hyps=Hn, reproj_thresh=3.0, subsets=good,
                          medians=medians)
    got = rsac.hypotheses("homography", pr["src"], pr["dst"], n_hyps=Hn, reproj_thresh=3.0, subsets=bad,
                          medians=medians)
    assert (ref[0] != -1).all()
    np.testing.assert_array_equal(np.flatnonzero(got[0] == -1), [3, 10])
    keep = np.ones(Hn, bool)
    keep[[3, 10]] = False
    np.testing.assert_array_equal(got[0][keep], ref[0][keep])
    if medians:
        assert got[1].dtype == np.float64 and np.array_equal(got[1][keep], ref[1][keep], equal_nan=True)
    else:
        np.testing.assert_array_equal(got[1][keep], ref[1][keep])
    assert np.array_equal(got[2][keep].view(np.uint64), ref[2][keep].view(np.uint64))


# ---------------------------------------------------------------------------------------------
# 5. the shared argument checks keep their codes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [0.0, float("inf"), float("nan")])
def test_msac_threshold_is_checked(thr):
    pr = _pnp(50, 0.3, 6)
    calls = [
        lambda: rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 500, thr, score="msac"),
        lambda: rsac.score_poses(pr["points2d"], pr["points3d"], pr["K"], np.hstack([np.eye(3), np.ones((3, 1))])[None],
                                 thr, costs=True),
        lambda: rsac.hypotheses("pnp", pr["points3d"], pr["points2d"], pr["K"], 0, 16, thr, costs=True),
    ]
    for call in calls:
        with pytest.raises(rsac.RsacError, match="finite positive threshold") as ei:
            call()
        assert ei.value.code == L.EINVAL


def test_twelve_distortion_coefficients_are_refused():
    pr = _pnp(50, 0.3, 6)
    n = 50
    p3, p2 = np.ascontiguousarray(pr["points3d"]), np.ascontiguousarray(pr["points2d"])
    K9 = np.ascontiguousarray(np.asarray(pr["K"], np.float64).reshape(9))
    d12 = np.full(12, 1e-3)
    R, t, mask = np.zeros(9), np.zeros(3), np.zeros(n, np.uint8)
    model = np.concatenate([np.eye(3).reshape(9), np.ones(3)])
    counts, cnt = np.zeros(1, np.int32), L.C.c_int32(0)
    ctx = L.context(0)
    lib = L.lib()
    with ctx.lock:
        code = lib.rsac_pnp_ransac_dist(ctx.handle, p3.ctypes.data, p2.ctypes.data, n, K9.ctypes.data, d12.ctypes.data,
                                        12, 500, 30.0, 0.99, SEED, L.F_ADAPTIVE, R.ctypes.data, t.ctypes.data,
                                        mask.ctypes.data, None, None)
        assert code == L.EINVAL and b"thin prism" in lib.rsac_last_error()
        code = lib.rsac_pnp_mask_dist(ctx.handle, p3.ctypes.data, p2.ctypes.data, n, K9.ctypes.data, d12.ctypes.data,
                                      12, model.ctypes.data, 30.0, 0, mask.ctypes.data, L.C.byref(cnt), None)
        assert code == L.EINVAL and b"thin prism" in lib.rsac_last_error()
        code = lib.rsac_score_poses_dist(ctx.handle, p3.ctypes.data, p2.ctypes.data, n, K9.ctypes.data,
                                         d12.ctypes.data, 12, model.ctypes.data, 1, 30.0, 0, counts.ctypes.data, None)
        assert code == L.EINVAL and b"thin prism" in lib.rsac_last_error()
