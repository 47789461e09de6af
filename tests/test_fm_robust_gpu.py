"""MSAC and LMedS for the fundamental matrix on the GPU (RSAC_F_MSAC through rsac_fundamental_ransac,
rsac_fundamental_lmeds; k_fm_cost, k_fm_cost_lane, k_fm_median, k_fm_median_lane): every comparison
of status, counts, costs, medians, masks and model bits is exact equality -- with the restatement
of tests/fmrobustref.py at its (small) shapes, and with the library's own host functions, which the
CPU tests tie to that restatement, beyond them.  Data: synth.fundamental_problem at its default
noise, 1.5 px (k = 18, Q = 589824), seed 0x5EED.

Sizes: kLanePts = 256 (lane / tile kernels), 256 = one wave's tile and 1024 = one pass of the four
waves of k_fm_cost<4, 32>, 512 = the register keys of k_fm_median<8>, 1024 = one key slot of the 16
waves of k_fm_median_block<16, 64> and 65536 = all its slots, 256 = one step of the recomputing
pass beyond; each with its neighbours.  8200 points at 90 % outliers for a cost above 2^32.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fmrobustref as R  # noqa: E402
import pyoracle as O  # noqa: E402
import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402
from rsac import synth  # noqa: E402

pytestmark = pytest.mark.gpu

THR, SEED = R.THR, R.SEED


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _np(m):
    return m.cpu().numpy() if hasattr(m, "cpu") else np.asarray(m)


def _probe(pr, hyp0, H):
    st, cnt, mdl, cost = rsac.fundamental_costs(pr["pts1"], pr["pts2"], hyp0, H, THR, seed=SEED)
    st2, med, mdl2 = rsac.hypotheses("fundamental", pr["pts1"], pr["pts2"], None, hyp0, H, seed=SEED, medians=True)
    np.testing.assert_array_equal(st2, st)
    assert _bits_equal(mdl2[:, :9], mdl[:, :9])
    assert cost.dtype == np.int64 and med.dtype == np.float64
    assert (cost[st <= 0] == -1).all() and (cnt[st <= 0] == 0).all() and (med[st <= 0] == -1.0).all()
    # the counts are the exact count kernel's own
    st3, cnt3, mdl3 = rsac.hypotheses("fundamental", pr["pts1"], pr["pts2"], None, hyp0, H, THR, seed=SEED,
                                      exact_only=True)
    np.testing.assert_array_equal(st3, st)
    np.testing.assert_array_equal(cnt3, cnt)
    assert _bits_equal(mdl3[:, :9], mdl[:, :9])
    return st, cnt, cost, med, mdl


def _check_against_restatement(key, H, hyp0=0):
    rs, rc, rcost, rmed, rm = R.hypotheses_case(*key, H, hyp0)
    st, cnt, cost, med, mdl = _probe(R.problem(*key), hyp0, H)
    np.testing.assert_array_equal(st, rs)
    assert _bits_equal(mdl[:, :9], rm[:, :9])
    np.testing.assert_array_equal(cnt, rc)
    np.testing.assert_array_equal(cost, rcost)
    assert _bits_equal(med, rmed)
    return cost


def _check_against_host(key, H, hyp0=0):
    pr = R.problem(*key)
    st, cnt, cost, med, mdl = _probe(pr, hyp0, H)
    ocnt, ost, omdl = O.fm_hypotheses(O.soa_hom(pr["pts1"], pr["pts2"]), THR, SEED, H, hyp0=hyp0, models=True)
    np.testing.assert_array_equal(st, ost)
    assert _bits_equal(mdl[:, :9], omdl[:, :9])
    np.testing.assert_array_equal(cnt[st > 0], ocnt[st > 0])
    assert (st > 0).any()
    for h in np.flatnonzero(st > 0):
        assert rsac.fundamental_cost(pr["pts1"], pr["pts2"], mdl[h, :9], THR) == (int(cnt[h]), int(cost[h])), h
        assert _bits_equal(rsac.fm_median(pr["pts1"], pr["pts2"], mdl[h, :9]), med[h]), h
    return cost


def _case(n):
    return (n, 0.0 if n <= 9 else 0.3, 100 + n)


@pytest.mark.parametrize("key", R.INPUTS)
def test_per_hypothesis_equals_restatement(key):
    _check_against_restatement(key, 64)


def test_costs_accumulate_in_64_bits():
    cost = _check_against_restatement(R.BIG, 8)
    assert cost.max() > 2**32
    assert _check_against_host(R.BIG, 64).max() > 2**32


@pytest.mark.parametrize("n", [8, 9, 12, 13, 63, 64, 65, 255, 256, 257, 511, 512, 513, 768, 769, 1023, 1024, 1025, 2049])
def test_per_hypothesis_equals_host_functions(n):
    _check_against_host(_case(n), 512)


@pytest.mark.parametrize("n", [65535, 65536, 65537, 65792, 65793])
def test_per_hypothesis_around_the_block_kernels_capacity(n):
    """65536 points = the keys a block of k_fm_median_block<16, 64> holds; beyond it k_fm_median<8>
    recomputes the keys on every pass, 256 points a step"""
    _check_against_host(_case(n), 6)


@pytest.mark.parametrize("n", [12, 257, 513])
@pytest.mark.parametrize("H", [1, 100])
def test_h_not_a_multiple_of_the_block(n, H):
    _check_against_host(_case(n), H)


@pytest.mark.parametrize("n", [12, 257, 513])
def test_from_hyp_begin_4096(n):
    _check_against_host(_case(n), 100, hyp0=4096)


def test_from_hyp_begin_4096_equals_restatement():
    _check_against_restatement((64, .3, 2), 32, hyp0=4096)


# ---------------------------------------------------------------------------------------------
# end to end: fundamental_ransac(score="msac")
# ---------------------------------------------------------------------------------------------
def _check_msac(pr, ref, **kw):
    F, mask, info = rsac.fundamental_ransac(pr["pts1"], pr["pts2"], THR, max_iters=R.MAX_ITERS, confidence=R.CONF,
                                            seed=SEED, score="msac", return_info=True, **kw)
    assert (info.best_hyp, info.cost, info.n_inliers, info.iters) == (ref["best"], ref["cost"], ref["n_inliers"],
                                                                      ref["iters"])
    np.testing.assert_array_equal(_np(mask), ref["mask"])
    if ref["best"] < 0:
        assert F is None and not info.ok and info.cost == -1 and np.isnan(info.cost_px2)
    else:
        assert info.ok and _bits_equal(F, ref["F"])
        assert info.cost_px2 == ref["cost"] / 2.0**18
        assert info.score_ms > 0.0  # the cost kernel is what score_ms times
    return info


@pytest.mark.parametrize("row", range(len(R.MSAC_TABLE)))
def test_fundamental_ransac_msac_equals_table(row):
    key, want = R.MSAC_TABLE[row]
    ref = R.msac_case(*key)
    assert (ref["best"], ref["cost"], ref["n_inliers"], ref["iters"], ref["count_best"]) == want
    pr = R.problem(*key)
    _check_msac(pr, ref)
    # the count rule still picks its own winner
    infoc = rsac.fundamental_ransac(pr["pts1"], pr["pts2"], THR, max_iters=R.MAX_ITERS, confidence=R.CONF, seed=SEED,
                                    return_info=True)[2]
    assert (infoc.best_hyp, infoc.n_inliers, infoc.iters) == (ref["count_best"], ref["count_good"], ref["count_iters"])
    assert infoc.cost == -1 and np.isnan(infoc.cost_px2)


@pytest.mark.parametrize("row", [0, 2])
def test_fundamental_ransac_msac_fixed_budget(row):
    """adaptive=False scores all max_iters hypotheses in one round; the scan over them is the same
    sequential scan, so the result is the adaptive call's."""
    key, _ = R.MSAC_TABLE[row]
    info = _check_msac(R.problem(*key), R.msac_case(*key), adaptive=False)
    assert info.hyps_scored == R.MAX_ITERS and info.rounds == 1


@pytest.mark.parametrize("row", [1, 2])
def test_fundamental_ransac_msac_torch_device_inputs_and_mask(row):
    import torch
    key, _ = R.MSAC_TABLE[row]
    pr = R.problem(*key)
    dev = dict(pts1=torch.as_tensor(pr["pts1"].copy(), device="cuda"),
               pts2=torch.as_tensor(pr["pts2"].copy(), device="cuda"))
    F, mask, info = rsac.fundamental_ransac(dev["pts1"], dev["pts2"], THR, max_iters=R.MAX_ITERS, seed=SEED,
                                            score="msac", return_info=True)
    assert hasattr(mask, "is_cuda") and mask.is_cuda  # device inputs: the mask stays on the device
    _check_msac(dev, R.msac_case(*key))


def _no_model_scene():
    """every first-image point the same: the 8-point normalisation fails, no hypothesis has a model"""
    rng = np.random.default_rng(3)
    return dict(pts1=np.tile([[100.0, 200.0]], (12, 1)), pts2=rng.uniform(0, 1000, (12, 2)))


def test_scene_without_any_model():
    pr = _no_model_scene()
    ref = R.msac(pr["pts1"], pr["pts2"], max_iters=64)
    assert ref["best"] == -1 and O.fm_ransac(pr["pts1"], pr["pts2"], THR, R.CONF, 64, SEED)["best"] == -1
    F, mask, info = rsac.fundamental_ransac(pr["pts1"], pr["pts2"], THR, max_iters=64, seed=SEED, score="msac",
                                            return_info=True)
    assert F is None and not info.ok and info.cost == -1 and np.isnan(info.cost_px2) and not _np(mask).any()
    assert info.iters == ref["iters"]
    F, mask, info = rsac.fundamental_lmeds(pr["pts1"], pr["pts2"], n_iters=64, seed=SEED, return_info=True)
    assert F is None and not info.ok and info.median == -1.0 and not _np(mask).any()


# ---------------------------------------------------------------------------------------------
# end to end: fundamental_lmeds
# ---------------------------------------------------------------------------------------------
def _check_lmeds(pr, ref, **kw):
    F, mask, info = rsac.fundamental_lmeds(pr["pts1"], pr["pts2"], seed=SEED, return_info=True, **kw)
    np.testing.assert_array_equal(_np(mask), ref["mask"])
    assert (info.best_hyp, info.n_inliers, info.iters) == (ref["best"], ref["n_inliers"], ref["iters"])
    assert _bits_equal(info.median, ref["median"])
    if ref["best"] < 0:
        assert F is None and not info.ok
    else:
        assert info.ok and _bits_equal(F, ref["F"]) and info.score_ms > 0.0
    return info


@pytest.mark.parametrize("row", range(len(R.LMEDS_TABLE)))
def test_fundamental_lmeds_equals_table(row):
    """(row 0 is n = 9, the smallest problem the call takes)"""
    key, want = R.LMEDS_TABLE[row]
    pr = R.problem(*key)
    F, mask, info = rsac.fundamental_lmeds(pr["pts1"], pr["pts2"], seed=SEED, return_info=True)
    assert (info.best_hyp, info.median, info.n_inliers) == want and info.iters == 548 and info.hyps_scored == 548
    assert F is not None and int(_np(mask).sum()) == want[2]
    if key[0] <= 300:  # the whole chain restated (the CPU tests pin every row's restatement to the table)
        _check_lmeds(pr, R.lmeds_case(*key))


@pytest.mark.parametrize("key", [(12, .25, 5), (257, .3, 8)])
def test_fundamental_lmeds_given_iteration_count(key):
    info = _check_lmeds(R.problem(*key), R.lmeds_case(*key, n_iters=40), n_iters=40)
    assert info.hyps_scored == 40


def test_fundamental_lmeds_device_inputs_and_mask():
    import torch
    key = (256, .3, 8)
    pr = R.problem(*key)
    dev = dict(pts1=torch.as_tensor(pr["pts1"].copy(), device="cuda"),
               pts2=torch.as_tensor(pr["pts2"].copy(), device="cuda"))
    F, mask = rsac.fundamental_lmeds(dev["pts1"], dev["pts2"], seed=SEED)
    assert hasattr(mask, "is_cuda") and mask.is_cuda
    _check_lmeds(dev, R.lmeds_case(*key))


def _few_ones_scene():
    """9 unrelated points, 24 hypotheses: the winner's sigma bound passes fewer than 8 of them"""
    rng = np.random.default_rng(8)
    return dict(pts1=rng.uniform(0, 1000, (9, 2)), pts2=rng.uniform(0, 1000, (9, 2)))


def test_fundamental_lmeds_fewer_than_8_ones_is_no_model():
    pr = _few_ones_scene()
    ref = R.lmeds(pr["pts1"], pr["pts2"], n_iters=24)
    assert ref["best"] == -1 and (ref["status"] > 0).any() and ref["median"] == -1.0
    _check_lmeds(pr, ref, n_iters=24)
    n = 9
    a, b = np.ascontiguousarray(pr["pts1"]), np.ascontiguousarray(pr["pts2"])
    F, mask, med = np.ones(9), np.ones(n, np.uint8), C.c_double(5.0)  # the C call zeroes F and the mask itself
    ctx = L.context(0)
    with ctx.lock:
        code = L.lib().rsac_fundamental_lmeds(ctx.handle, a.ctypes.data, b.ctypes.data, n, 24, 0.99, SEED, 0,
                                              F.ctypes.data, mask.ctypes.data, C.byref(med), None, None)
    assert code == L.NO_MODEL and not F.any() and not mask.any() and med.value == -1.0


# ---------------------------------------------------------------------------------------------
# contracts
# ---------------------------------------------------------------------------------------------
def test_score_count_is_the_default_and_unchanged():
    key = (256, .3, 8)
    pr = R.problem(*key)
    kw = dict(max_iters=R.MAX_ITERS, confidence=R.CONF, seed=SEED, return_info=True)
    a = rsac.fundamental_ransac(pr["pts1"], pr["pts2"], THR, **kw)
    b = rsac.fundamental_ransac(pr["pts1"], pr["pts2"], THR, score="count", **kw)
    assert _bits_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert (a[2].best_hyp, a[2].iters, a[2].n_inliers, a[2].cost) == (b[2].best_hyp, b[2].iters, b[2].n_inliers, -1)
    ref = O.fm_ransac(pr["pts1"], pr["pts2"], THR, R.CONF, R.MAX_ITERS, SEED)
    assert (a[2].best_hyp, a[2].n_inliers, a[2].iters) == (ref["best"], ref["n_inliers"], ref["iters"]) == (88, 155, 253)
    assert _bits_equal(a[0], ref["F"]) and np.array_equal(a[1], ref["mask"])


def test_c_level_contracts():
    key, (best, cost, count, iters, _) = R.MSAC_TABLE[2]
    pr = R.problem(*key)
    n = key[0]
    a = np.ascontiguousarray(pr["pts1"], np.float64)
    b = np.ascontiguousarray(pr["pts2"], np.float64)
    Fm, mask = np.zeros(9), np.zeros(n, np.uint8)
    ctx = L.context(0)
    lib = L.lib()

    def call(flags, thr=THR, npts=n):
        with ctx.lock:
            return lib.rsac_fundamental_ransac(ctx.handle, a.ctypes.data, b.ctypes.data, npts, R.MAX_ITERS, thr, R.CONF,
                                               SEED, flags, Fm.ctypes.data, mask.ctypes.data, None, None)

    def last(P):
        out = np.zeros(P, np.int64)
        with ctx.lock:
            return lib.rsac_last_costs(ctx.handle, out.ctypes.data, P), out

    for bad in (L.F_LO, L.F_ASYNC):
        assert call(L.F_ADAPTIVE | L.F_MSAC | bad) == L.EINVAL
        assert b"RSAC_F_MSAC" in lib.rsac_last_error()
    for thr in (0.0, float("nan"), float("inf"), 1e30, 1e-30):  # thr2 = 0, NaN or inf as a float
        assert call(L.F_ADAPTIVE | L.F_MSAC, thr) == L.EINVAL, thr
        assert b"threshold" in lib.rsac_last_error()
    assert call(L.F_ADAPTIVE | L.F_MSAC, npts=7) == L.ETOOFEW
    assert call(L.F_ADAPTIVE | L.F_MSAC) == L.OK
    code, costs = last(1)
    assert code == L.OK and costs[0] == cost
    assert last(2)[0] == L.EINVAL
    assert call(L.F_ADAPTIVE) == L.OK  # a count call leaves the costs as it found them
    code, costs = last(1)
    assert code == L.OK and costs[0] == cost
    # the count probe rejects the flag and names the cost probe; the cost probe requires its output
    cnt, st = np.zeros(8, np.int32), np.zeros(8, np.int8)
    with ctx.lock:
        code = lib.rsac_fundamental_hypotheses(ctx.handle, a.ctypes.data, b.ctypes.data, n, 0, 8, THR, SEED, L.F_MSAC,
                                               cnt.ctypes.data, st.ctypes.data, None, None)
    assert code == L.EINVAL and b"rsac_fundamental_hypotheses_msac" in lib.rsac_last_error()
    with ctx.lock:
        code = lib.rsac_fundamental_hypotheses_msac(ctx.handle, a.ctypes.data, b.ctypes.data, n, 0, 8, THR, SEED, 0,
                                                    cnt.ctypes.data, st.ctypes.data, None, None, None)
    assert code == L.EINVAL and b"costs_out" in lib.rsac_last_error()
    cost8 = np.zeros(8, np.int64)
    with ctx.lock:
        code = lib.rsac_fundamental_hypotheses_msac(ctx.handle, a.ctypes.data, b.ctypes.data, n, 0, 8, float("nan"),
                                                    SEED, 0, cnt.ctypes.data, st.ctypes.data, None,
                                                    cost8.ctypes.data, None)
    assert code == L.EINVAL and b"threshold" in lib.rsac_last_error()

    # rsac_fundamental_lmeds
    med = C.c_double(0)

    def lmeds(flags=L.F_ADAPTIVE, npts=n, conf=0.99, mask_ptr=mask.ctypes.data):
        with ctx.lock:
            return lib.rsac_fundamental_lmeds(ctx.handle, a.ctypes.data, b.ctypes.data, npts, 2000, conf, SEED, flags,
                                              Fm.ctypes.data, mask_ptr, C.byref(med), None, None)

    assert lmeds(npts=8) == L.ETOOFEW and b"n - 8" in lib.rsac_last_error()
    for conf in (0.0, 1.0, float("nan")):
        assert lmeds(conf=conf) == L.EINVAL and b"confidence" in lib.rsac_last_error()
    for flag, name in ((L.F_SAMPLER_OPENCV, b"RSAC_F_SAMPLER_OPENCV"), (L.F_REFINE, b"RSAC_F_REFINE"),
                       (L.F_MSAC, b"RSAC_F_MSAC"), (L.F_LO, b"RSAC_F_LO"), (L.F_ASYNC, b"RSAC_F_ASYNC"),
                       (L.F_EXACT_ONLY, b"RSAC_F_EXACT_ONLY")):
        assert lmeds(L.F_ADAPTIVE | flag) == L.EINVAL and name in lib.rsac_last_error()
    assert lmeds(L.F_ADAPTIVE | L.F_DEVICE_OUT, mask_ptr=None) == L.EINVAL
    assert lmeds() == L.OK and med.value == R.LMEDS_TABLE[2][1][1]
    # rsac_fundamental_medians takes the device flags only
    m8 = np.zeros(8)
    with ctx.lock:
        code = lib.rsac_fundamental_medians(ctx.handle, a.ctypes.data, b.ctypes.data, n, 0, 8, SEED, L.F_ADAPTIVE,
                                            m8.ctypes.data, st.ctypes.data, None, None)
    assert code == L.EINVAL and b"RSAC_F_ADAPTIVE" in lib.rsac_last_error()
    with ctx.lock:
        code = lib.rsac_fundamental_medians(ctx.handle, a.ctypes.data, b.ctypes.data, n, 0, 8, SEED, 0, None,
                                            st.ctypes.data, None, None)
    assert code == L.EINVAL


def test_context_stats_are_left_alone():
    ctx = L.context(0)
    pr = R.problem(64, .3, 2)
    hp = synth.homography_problem(40, 0.3, seed=30)
    ctx.set_timing(True)
    try:
        rsac.homography_ransac(hp["src"], hp["dst"], 3.0)
        before = ctx.last_stats()
        assert before["gpu_ms"] > 0
        F, _ = rsac.fundamental_ransac(pr["pts1"], pr["pts2"], THR, max_iters=R.MAX_ITERS, score="msac")
        assert F is not None and ctx.last_stats() == before
        F, _ = rsac.fundamental_lmeds(pr["pts1"], pr["pts2"])
        assert F is not None and ctx.last_stats() == before
    finally:
        ctx.set_timing(False)
