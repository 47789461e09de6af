"""LMedS PnP on the GPU (k_pnp_median, k_pnp_median_block, k_pnp_median_lane, rsac_pnp_lmeds): every
comparison is exact equality with the chain of tests/pnplmedsref.py -- the unchanged CPU oracle for
samples, models, status and refit, the NumPy restatement for errors, medians, scan, sigma and masks.

Sizes of the probe: kLaneKeyPts = 32 (keys in LDS / recomputed, one lane per hypothesis), kLanePts =
256 (lane / wave kernel), 512 = 64 * kPnpMedP (wave / block kernel), 16384 (the block kernel's 16- /
64-slot instance), 65536 (keys in a block's registers / in key rows, or recomputed), odd and even.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pnplmedsref as M  # noqa: E402
import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

K_LANE_KEY_PTS = 32
BLOCK_CAP = 65536
SIZES = [12, 13, K_LANE_KEY_PTS, K_LANE_KEY_PTS + 1, 64, 65, 256, 257, 512, 513, 4097]


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def _key(n):
    return (n, 0.3, 100 + n % 50)


def _check_probe(n, H, hyp0):
    key = _key(n)
    pr = M.problem(*key)
    rs, rmed, rm, _, _ = M.hypotheses_case(*key, H, hyp0)
    st, med, mdl = rsac.pnp_medians(pr["points2d"], pr["points3d"], pr["K"], hyp0, H, seed=M.SEED)
    np.testing.assert_array_equal(st, rs)
    assert _bits_equal(mdl[:, :12], rm[:, :12])
    assert med.dtype == np.float64 and _same(med, rmed)
    assert (med[st > 0] >= 0).all() and (med[st <= 0] == -1.0).all()
    return med


# 130 hypotheses: neither a multiple of 4 (the wave kernel's block) nor of 256 (the lane kernel's)
@pytest.mark.parametrize("hyp0", [0, 7])
@pytest.mark.parametrize("n", SIZES)
def test_medians_per_hypothesis(n, hyp0):
    _check_probe(n, 130, hyp0)


# one point past each further boundary of the launcher (and the last size before it)
@pytest.mark.parametrize("n", [16384, 16385, BLOCK_CAP, BLOCK_CAP + 1])
def test_medians_at_the_block_kernel_boundaries(n):
    _check_probe(n, 8, 0)


def test_key_rows_in_chunks_and_recomputed_keys_agree():
    n = BLOCK_CAP + 1
    ctx = L.context(0)
    try:
        ref = _check_probe(n, 8, 0)  # the default budget: one chunk
        ctx.debug_set(L.DBG_LMEDS_KEYS, 3 * n * 4 + 100)  # rows for 3 hypotheses: chunks of 3, 3 and 2
        assert _same(_check_probe(n, 8, 0), ref)
        ctx.debug_set(L.DBG_LMEDS_KEYS, n * 4 - 4)  # not one row: recomputed
        assert _same(_check_probe(n, 8, 0), ref)
        ctx.debug_set(L.DBG_LMEDS_KEYS, -1)  # no rows: every pass recomputes the keys
        assert _same(_check_probe(n, 8, 0), ref)
    finally:
        ctx.debug_set(L.DBG_LMEDS_KEYS, 0)


def test_probe_with_caller_subsets_and_reference_mode():
    key = (64, .3, 7)
    pr = M.problem(*key)
    rng = np.random.default_rng(5)
    subs = np.array([rng.choice(64, 4, replace=False) for _ in range(130)], np.int32)
    subs[3] = [0, 0, 1, 2]  # a repeated point: no model
    subs[9] = [0, 1, 2, 64]  # out of range: status -1
    rs, rmed, rm, _, _ = M.hypotheses(pr["points3d"], pr["points2d"], pr["K"], 130, subsets=subs)
    st, med, mdl = rsac.pnp_medians(pr["points2d"], pr["points3d"], pr["K"], 0, 130, subsets=subs)
    np.testing.assert_array_equal(st, rs)
    assert rs[9] == -1 and rmed[3] == rmed[9] == -1.0
    assert _bits_equal(mdl[st > 0, :12], rm[st > 0, :12]) and _same(med, rmed)
    # reference mode: OpenCV's MWC subsets of 5 points, EPnP, the rvec round trip
    import pyoracle as O
    rs, rmed, rm, _, _ = M.hypotheses_case(*key, 89, 0, True)
    subs5, sst = O.mwc_subsets(64, 89, s=5)
    assert (sst == 1).all()
    st, med, mdl = rsac.pnp_medians(pr["points2d"], pr["points3d"], pr["K"], 0, 89, subsets=subs5, minimal="epnp5")
    np.testing.assert_array_equal(st, rs)
    assert _bits_equal(mdl[:, :12], rm[:, :12]) and _same(med, rmed)


def _check_full(pr, ref, **kw):
    R, t, mask, info = rsac.pnp_lmeds(pr["points2d"], pr["points3d"], pr["K"], return_info=True, **kw)
    assert (info.best_hyp, info.median, info.n_inliers, info.iters) == (ref["best"], ref["median"], ref["n_inliers"],
                                                                        ref["iters"])
    np.testing.assert_array_equal(np.asarray(mask), ref["mask"])
    if ref["best"] < 0:
        assert R is None and t is None and not info.ok
    else:
        assert info.ok and _bits_equal(R, ref["R"]) and _bits_equal(t, ref["t"])
    return info


@pytest.mark.parametrize("refine", [True, False, "epnp"])
@pytest.mark.parametrize("row", range(len(M.TABLE)))
def test_full_call_equals_table_and_chain(row, refine):
    key, (best, median, ones) = M.TABLE[row]
    ref = M.lmeds_case(*key, refine=refine)
    assert (ref["best"], ref["median"], ref["n_inliers"]) == (best, median, ones)
    info = _check_full(M.problem(*key), ref, refine=refine)
    assert info.hyps_scored == 48 and info.rounds == 1 and info.score_ms > 0.0  # the median kernel's time


@pytest.mark.parametrize("refine", [True, False, "epnp"])
@pytest.mark.parametrize("row", range(len(M.TABLE)))
def test_full_call_with_40_hypotheses(row, refine):
    key = M.TABLE[row][0]
    ref = M.lmeds_case(*key, n_iters=40, refine=refine)
    assert ref["iters"] == 40
    _check_full(M.problem(*key), ref, n_iters=40, refine=refine)


@pytest.mark.parametrize("refine", [True, False, "epnp"])
@pytest.mark.parametrize("row", range(len(M.TABLE_REF)))
def test_full_call_reference_mode(row, refine):
    key, (best, median, ones) = M.TABLE_REF[row]
    ref = M.lmeds_case(*key, refine=refine, reference_mode=True)
    assert (ref["best"], ref["median"], ref["n_inliers"], ref["iters"]) == (best, median, ones, 89)
    _check_full(M.problem(*key), ref, sampler="opencv", minimal="epnp5", refine=refine)


def _check_batch(p2s, p3s, Ks, **kw):
    out = rsac.pnp_lmeds_batched(p2s, p3s, Ks, **kw)
    assert len(out) == len(Ks)
    for p, (R, t, mask, ninl, med) in enumerate(out):
        ref = M.lmeds(p3s[p], p2s[p], Ks[p], **kw)
        R1, t1, m1, info = rsac.pnp_lmeds(p2s[p], p3s[p], Ks[p], return_info=True, **kw)
        np.testing.assert_array_equal(mask, ref["mask"])
        np.testing.assert_array_equal(mask, m1)
        assert (ninl, med) == (ref["n_inliers"], ref["median"]) == (info.n_inliers, info.median), p
        if ref["best"] < 0:
            assert R is None and t is None and R1 is None and (ninl, med) == (0, -1.0)
        else:
            assert _bits_equal(R, ref["R"]) and _bits_equal(t, ref["t"]), p
            assert _bits_equal(R, R1) and _bits_equal(t, t1), p
    return out


@pytest.mark.parametrize("refine", [True, False])
def test_batched_k_sweep_of_the_12_point_problem(refine):
    pr = M.problem(12, .25, 5)
    Ks = []
    for f in (0.8, 0.9, 1.0, 1.1, 1.25):  # five intrinsics, shared points
        K = np.array(pr["K"])
        K[0, 0] *= f
        K[1, 1] *= f
        Ks.append(K)
    out = _check_batch([pr["points2d"]] * 5, [pr["points3d"]] * 5, Ks, refine=refine)
    meds = [o[4] for o in out]
    assert meds[2] == M.TABLE[0][1][1] and min(meds) == meds[2]  # the true focal length has the lowest median


# (12, 257, 4097): the block kernel serves all three; (12, 300): the wave kernel serves the 12-point
# problem, which the lane kernel serves in its single call -- the kernels agree
@pytest.mark.parametrize("sizes", [(12, 257, 4097), (12, 300), (5, 4, 13)])
def test_batched_mixed_sizes_equal_single_calls(sizes):
    prs = [M.problem(*(M.NO_MODEL if n == 5 else (n, 0.0, 104) if n == 4 else _key(n))) for n in sizes]
    _check_batch([p["points2d"] for p in prs], [p["points3d"] for p in prs], [p["K"] for p in prs])


def test_torch_device_inputs_and_device_mask():
    import torch
    key = M.TABLE[5][0]  # 257 points
    pr, ref = M.problem(*key), M.lmeds_case(*key)
    p2 = torch.tensor(pr["points2d"], dtype=torch.float64, device="cuda")
    p3 = torch.tensor(pr["points3d"], dtype=torch.float64, device="cuda")
    R, t, mask, info = rsac.pnp_lmeds(p2, p3, pr["K"], return_info=True)
    assert mask.is_cuda and mask.dtype == torch.bool
    np.testing.assert_array_equal(mask.cpu().numpy(), ref["mask"])
    assert (info.best_hyp, info.median) == (ref["best"], ref["median"])
    assert _bits_equal(R, ref["R"]) and _bits_equal(t, ref["t"])
    R2, t2, m2 = rsac.pnp_lmeds(pr["points2d"], pr["points3d"], pr["K"])
    assert _bits_equal(R, R2) and _bits_equal(t, t2) and np.array_equal(m2, ref["mask"])


def test_direct_problems_of_four_and_five_points():
    p4 = M.problem(4, 0.0, 104)
    ref = M.lmeds(p4["points3d"], p4["points2d"], p4["K"])
    R, t, mask, info = rsac.pnp_lmeds(p4["points2d"], p4["points3d"], p4["K"], return_info=True)
    assert ref["best"] == 0 and info.ok and info.median == 0.0 and mask.all() and info.n_inliers == 4
    assert _bits_equal(R, ref["R"]) and _bits_equal(t, ref["t"])
    p5 = M.problem(5, 0.0, 105)
    ref = M.lmeds(p5["points3d"], p5["points2d"], p5["K"], reference_mode=True)
    R, t, mask, info = rsac.pnp_lmeds(p5["points2d"], p5["points3d"], p5["K"], sampler="opencv", minimal="epnp5",
                                      return_info=True)
    assert ref["best"] == 0 and info.ok and info.median == 0.0 and mask.all() and info.n_inliers == 5
    assert _bits_equal(R, ref["R"]) and _bits_equal(t, ref["t"])


def test_80_percent_outliers_no_model():
    pr, ref = M.problem(*M.NO_MODEL), M.lmeds_case(*M.NO_MODEL)
    assert ref["best"] == -1 and ref["iters"] == 48  # the chain: a winner, but a mask of 3 ones
    R, t, mask, info = rsac.pnp_lmeds(pr["points2d"], pr["points3d"], pr["K"], return_info=True)
    assert R is None and t is None and not mask.any() and not info.ok
    assert (info.best_hyp, info.median, info.n_inliers, info.iters) == (-1, -1.0, 0, 48)
    # and a larger 80 % problem: whatever the chain says, the call says
    big = (500, .8, 11)
    _check_full(M.problem(*big), M.lmeds_case(*big))


def test_c_abi_contract():
    pr = M.problem(*M.TABLE[1][0])
    p3 = np.ascontiguousarray(pr["points3d"])
    p2 = np.ascontiguousarray(pr["points2d"])
    K9 = np.ascontiguousarray(pr["K"], np.float64).reshape(9)
    n = len(p3)
    ctx = L.context(0)
    R, t, mask = np.zeros(9), np.zeros(3), np.zeros(n, np.uint8)

    def call(flags, conf=0.99, n_pts=n, mask_ptr=mask.ctypes.data, max_iters=2000):
        return L.lib().rsac_pnp_lmeds(ctx.handle, p3.ctypes.data, p2.ctypes.data, n_pts, K9.ctypes.data, max_iters,
                                      conf, M.SEED, flags, R.ctypes.data, t.ctypes.data, mask_ptr, None, None, None)

    assert call(L.F_ADAPTIVE) == L.OK
    for flag, name in [(L.F_EXACT_ONLY, b"RSAC_F_EXACT_ONLY"), (L.F_LO, b"RSAC_F_LO"), (L.F_ASYNC, b"RSAC_F_ASYNC"),
                       (L.F_MSAC, b"RSAC_F_MSAC")]:
        assert call(L.F_ADAPTIVE | flag) == L.EINVAL and name in L.lib().rsac_last_error()
    assert call(1 << 20) == L.EINVAL and b"unknown flag" in L.lib().rsac_last_error()
    for conf in (0.0, 1.0):
        assert call(L.F_ADAPTIVE, conf=conf) == L.EINVAL and b"confidence" in L.lib().rsac_last_error()
    assert call(0, max_iters=0) == L.EINVAL and b"max_iters" in L.lib().rsac_last_error()
    assert call(L.F_ADAPTIVE, n_pts=3) == L.ETOOFEW
    assert call(L.F_ADAPTIVE | L.F_DEVICE_OUT, mask_ptr=None) == L.EINVAL and b"mask_out" in L.lib().rsac_last_error()
    # the probe takes neither the sampler nor the refit flags
    med, st = np.zeros(8), np.zeros(8, np.int8)
    code = L.lib().rsac_pnp_medians(ctx.handle, p3.ctypes.data, p2.ctypes.data, n, K9.ctypes.data, 0, 8, 1,
                                    L.F_REFINE, None, med.ctypes.data, st.ctypes.data, None, None)
    assert code == L.EINVAL and b"RSAC_F_REFINE" in L.lib().rsac_last_error()
    # rsac_set_timing: the call's figures in rsac_last_stats
    assert L.lib().rsac_set_timing(ctx.handle, 1) == L.OK
    try:
        assert call(L.F_ADAPTIVE) == L.OK
        s = L.Stats()
        assert L.lib().rsac_last_stats(ctx.handle, C.byref(s)) == L.OK
        assert (s.iters, s.hyps_scored, s.rounds) == (48, 48, 1) and s.score_ms > 0.0
        assert s.n_inliers == int(mask.sum()) == M.lmeds_case(*M.TABLE[1][0])["n_inliers"]
    finally:
        L.lib().rsac_set_timing(ctx.handle, 0)
