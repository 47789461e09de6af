"""The least-squares fundamental matrix and its local optimisation on the GPU (k_fm_fit_sums,
k_fm_fit_finish; rsac_fundamental_fit_device, rsac_fundamental_local_opt, RSAC_F_REFINE on
rsac_fundamental_ransac): every comparison of model bits, masks, counts and rounds is exact equality
with the library's host fit, which tests/test_fm_fit.py ties to the restatement of
tests/fmfitref.py, and with that file's pinned table.

Sizes: the summation order cuts the points into ranges of 4096 (one block each) of 512 slots (one
thread each) in waves of 64 -- 63 / 64 / 65, 511 / 512 / 513, 4095 / 4096 / 4097 and 8191 / 8192 /
8193 lie around a wave, a pass of the slots, and the first two range boundaries; 70 000 (18 ranges,
the last one short) and 300 000 (74 ranges) cover the finishing kernel's long rows.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fmfitref as R  # noqa: E402
import fmrobustref as RR  # noqa: E402
import pyoracle as O  # noqa: E402
import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402
from rsac import synth  # noqa: E402

pytestmark = pytest.mark.gpu

THR, SEED = R.THR, R.SEED
TABLE = dict(R.TABLE)


def _bits_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _np(m):
    return m.cpu().numpy() if hasattr(m, "cpu") else np.asarray(m)


def _dev(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device="cuda", dtype=dtype)


@functools.lru_cache(maxsize=None)
def _problem(n):
    pr = synth.fundamental_problem(n, 0.0 if n < 20 else 0.3, seed=100 + n)
    return pr["pts1"], pr["pts2"]


def _masks(n):
    """name -> mask (None = all) of the issue's list; the ranges are those of the summation order"""
    nr = R.ranges(n)
    out = {"ones": None, "third": np.arange(n) % 3 != 0}
    eight = np.zeros(n, bool)  # exactly 8 ones: the first four points and the last four (the last range's end)
    eight[:4] = eight[n - 4:] = True
    assert int(eight.sum()) == 8
    out["eight"] = eight
    gap = np.ones(n, bool)  # one whole range masked out (the only one: no model)
    r = nr // 2
    gap[r * R.RANGE:(r + 1) * R.RANGE] = False
    out["gap"] = gap
    seven = eight.copy()
    seven[n - 1] = False
    out["seven"] = seven
    return out


def _fit_soa(p1, p2, mask):
    """rsac_fundamental_fit_device over f32 SoA device inputs (the C ABI directly)"""
    import torch
    a, b = _dev(p1.T, torch.float32), _dev(p2.T, torch.float32)
    m = None if mask is None else _dev(mask.astype(np.uint8))
    ctx = L.context(0)
    F = np.zeros(9)
    with ctx.lock:
        code = L.check(L.lib().rsac_fundamental_fit_device(ctx.handle, a.data_ptr(), b.data_ptr(), p1.shape[0],
                                                           None if m is None else m.data_ptr(), L.F_DEVICE_SOA,
                                                           F.ctypes.data, None))
    torch.cuda.synchronize()
    return F.reshape(3, 3) if code == L.OK else None


@pytest.mark.parametrize("n", [8, 9, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 8193, 70000, 300000])
def test_device_fit_equals_host_fit(n):
    import torch
    p1, p2 = _problem(n)
    t1, t2 = _dev(p1), _dev(p2)
    for name, mask in _masks(n).items():
        want = rsac.fundamental_fit(p1, p2, mask)
        ones = n if mask is None else int(mask.sum())
        assert (want is None) == (ones < 8), (name, ones)
        assert _bits_equal(rsac.fundamental_fit(p1, p2, mask, device=0), want), name
        dm = None if mask is None else _dev(mask)
        assert dm is None or dm.dtype == torch.bool
        assert _bits_equal(rsac.fundamental_fit(t1, t2, dm), want), name
        assert _bits_equal(_fit_soa(p1, p2, mask), want), name


def test_device_fit_ignores_what_the_mask_hides():
    p1, p2 = (a.copy() for a in _problem(4097))
    mask = np.arange(4097) % 3 != 0
    want = rsac.fundamental_fit(p1, p2, mask)
    p1[0], p2[3], p1[4095, 1], p2[4092, 0] = np.nan, np.inf, -np.inf, np.nan  # indices with i % 3 == 0
    assert _bits_equal(rsac.fundamental_fit(_dev(p1), _dev(p2), _dev(mask)), want)
    p1[1, 0] = np.nan  # under the mask: no model on both sides
    assert rsac.fundamental_fit(p1, p2, mask) is None and rsac.fundamental_fit(_dev(p1), _dev(p2), _dev(mask)) is None


def test_device_fit_of_coincident_points():
    p1, p2 = (a.copy() for a in _problem(513))
    p1[:], p2[:] = p1[0], p2[0]
    assert rsac.fundamental_fit(p1, p2) is None and rsac.fundamental_fit(p1, p2, device=0) is None


# ---------------------------------------------------------------------------------------------
# fundamental_ransac(refine=True)
# ---------------------------------------------------------------------------------------------
def _same_info(a, b):
    keys = ("ok", "n_inliers", "best_hyp", "iters", "hyps_scored", "rounds", "lo_improvements", "cost")
    return [getattr(a, k) for k in keys] == [getattr(b, k) for k in keys]


@pytest.mark.parametrize("key", [(64, .3, 2), (257, .3, 8), (4097, .5, 4)])
@pytest.mark.parametrize("variant", ["default", "msac", "device", "fixed"])
def test_ransac_refine(key, variant):
    """(fails on a library without the refit: it answers RSAC_F_REFINE with RSAC_EINVAL)"""
    pr = R.problem(*key)
    p1, p2 = pr["pts1"], pr["pts2"]
    kw = dict(return_info=True)
    if variant == "msac":
        kw["score"] = "msac"
    elif variant == "fixed":
        kw.update(adaptive=False, max_iters=2000)
    a1, a2 = (_dev(p1), _dev(p2)) if variant == "device" else (p1, p2)
    F0, m0, i0 = rsac.fundamental_ransac(a1, a2, THR, **kw)
    F1, m1, i1 = rsac.fundamental_ransac(a1, a2, THR, refine=True, **kw)
    assert F0 is not None and F1 is not None
    if variant == "device":
        assert m1.is_cuda
    elif variant == "default":
        best = TABLE[key][0]
        assert (i0.best_hyp, i0.n_inliers) == (best, TABLE[key][1])
    assert np.array_equal(_np(m0), _np(m1)) and _same_info(i0, i1)
    assert i1.n_inliers == int(_np(m1).sum())
    want = rsac.fundamental_fit(p1, p2, _np(m1))
    assert want is not None and _bits_equal(F1, want)
    assert not _bits_equal(F1, F0)
    if variant == "default":
        assert O.fm_count(F1, R.soa_of(key), THR) == TABLE[key][2]


# ---------------------------------------------------------------------------------------------
# fundamental_local_opt and refine="lo"
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _winner(key):
    return R.winner_from_index(key, TABLE[key][0])


def _host_fit(key):
    pr = R.problem(*key[:3])
    return lambda soa, m: rsac.fundamental_fit(pr["pts1"], pr["pts2"], m)


@pytest.mark.parametrize("key", [k for k, _ in R.TABLE], ids=[str(k[0]) for k, _ in R.TABLE])
def test_local_opt_equals_the_table(key):
    pr, soa = R.problem(*key[:3]), R.soa_of(key)
    F0, mask0, c0 = _winner(key)
    best, c0_t, c1_t, c8_t, steps8_t, _ = TABLE[key]
    assert c0 == c0_t
    for cap in (1, 4, 8):
        F, mask, count, steps = rsac.fundamental_local_opt(pr["pts1"], pr["pts2"], F0, THR, max_rounds=cap)
        rF, rmask, rcount, rsteps = R.local_opt(soa, F0, THR, cap, _host_fit(key))
        assert (count, steps) == (rcount, rsteps)
        assert np.array_equal(mask, rmask) and int(mask.sum()) == count
        assert _bits_equal(F, rF)
        if cap == 1:
            assert (count, steps) == ((c1_t, 1) if c1_t > c0_t else (c0_t, 0))
        if cap == 8:
            assert (count, steps) == (c8_t, steps8_t)


@pytest.mark.parametrize("key", [(64, .3, 2), (1025, .3, 6), (4097, .5, 4), (50000, .8, 2, 100000)],
                         ids=["64", "1025", "4097", "50000"])
def test_ransac_refine_lo(key):
    pr, soa = R.problem(*key[:3]), R.soa_of(key)
    p1, p2 = _dev(pr["pts1"]), _dev(pr["pts2"])
    F, mask, info = rsac.fundamental_ransac(p1, p2, THR, refine="lo", return_info=True)
    assert info.best_hyp == TABLE[key][0] and mask.is_cuda
    rF, rmask, rcount, rsteps = R.local_opt(soa, _winner(key)[0], THR, 4, _host_fit(key))
    assert (info.n_inliers, info.lo_improvements) == (rcount, rsteps)
    assert np.array_equal(_np(mask), rmask) and _bits_equal(F, rF)
    if TABLE[key][4] <= 4:
        assert (rcount, rsteps) == TABLE[key][3:5]


def test_local_opt_from_a_model_without_support():
    pr = R.problem(257, .3, 8)
    F0 = np.array([[0, 0, 1.0], [0, 0, 0], [0, 0, 0]])  # x2 = 0: fewer than 8 points lie within 1.5 px of it
    want_c, want_m = O.fm_count(F0, R.soa_of((257, .3, 8)), THR, mask=True)
    assert want_c < 8
    for a1, a2 in ((pr["pts1"], pr["pts2"]), (_dev(pr["pts1"]), _dev(pr["pts2"]))):
        F, mask, count, steps = rsac.fundamental_local_opt(a1, a2, F0, THR, max_rounds=8)
        assert _bits_equal(F, F0) and (count, steps) == (want_c, 0) and np.array_equal(_np(mask), want_m)


def test_local_opt_from_an_all_zero_model():
    """the start rule of the single call: every row is a model, all zeros too (the batched call takes
    it for no model).  Every point passes the test of F = 0 (a zero Sampson error), so the count is n;
    no fit can raise it: F itself comes back after 0 steps"""
    pr = R.problem(64, .3, 2)
    for a1, a2 in ((pr["pts1"], pr["pts2"]), (_dev(pr["pts1"]), _dev(pr["pts2"]))):
        F, mask, count, steps = rsac.fundamental_local_opt(a1, a2, np.zeros((3, 3)), THR, max_rounds=8)
        print("fundamental_local_opt(F = 0):", F.tolist(), int(_np(mask).sum()), count, steps)
        assert _bits_equal(F, np.zeros((3, 3))) and (count, steps) == (64, 0)
        assert np.array_equal(_np(mask), np.ones(64, bool))


# ---------------------------------------------------------------------------------------------
# fundamental_lmeds(refine=)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(64, .3, 2), (257, .3, 8)])
def test_lmeds_refine(key):
    pr, soa = R.problem(*key), R.soa_of(key)
    F0, m0, i0 = rsac.fundamental_lmeds(pr["pts1"], pr["pts2"], return_info=True)
    F1, m1, i1 = rsac.fundamental_lmeds(pr["pts1"], pr["pts2"], refine=True, return_info=True)
    assert np.array_equal(m0, m1) and _same_info(i0, i1) and i0.median == i1.median
    assert _bits_equal(F1, rsac.fundamental_fit(pr["pts1"], pr["pts2"], m1)) and not _bits_equal(F1, F0)
    F2, m2, i2 = rsac.fundamental_lmeds(_dev(pr["pts1"]), _dev(pr["pts2"]), refine="lo", return_info=True)
    sigma = rsac.lmeds_sigma(i0.median, key[0], 8)
    rF, rmask, rcount, rsteps = R.local_opt(soa, F0, sigma, 4, _host_fit(key))
    assert (i2.n_inliers, i2.lo_improvements) == (rcount, rsteps)
    assert np.array_equal(_np(m2), rmask) and _bits_equal(F2, rF)


# ---------------------------------------------------------------------------------------------
# contracts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(64, .3, 2), (257, .3, 8)])
def test_defaults_are_unchanged(key):
    pr = R.problem(*key)
    F, mask, info = rsac.fundamental_ransac(pr["pts1"], pr["pts2"], THR, max_iters=3000, return_info=True)
    ref = O.fm_ransac(pr["pts1"], pr["pts2"], THR, 0.99, 3000, SEED)
    assert (info.best_hyp, info.n_inliers, info.iters) == (ref["best"], ref["n_inliers"], ref["iters"])
    assert _bits_equal(F, ref["F"]) and np.array_equal(mask, ref["mask"]) and info.lo_improvements == 0
    F, mask = rsac.fundamental_lmeds(pr["pts1"], pr["pts2"])
    ref = RR.lmeds_case(*key)
    assert _bits_equal(F, ref["F"]) and np.array_equal(mask, ref["mask"])


def _code_and_message(fn, *args):
    with pytest.raises(L.RsacError) as e:
        L.check(fn(*args))
    return e.value.code, str(e.value)


def test_rejected_flags_are_named():
    pr = R.problem(64, .3, 2)
    a, b = np.ascontiguousarray(pr["pts1"]), np.ascontiguousarray(pr["pts2"])
    ctx = L.context(0)
    F, mask, st = np.zeros(9), np.zeros(64, np.uint8), L.Stats()
    lib = L.lib()
    with ctx.lock:
        for flag, name in ((L.F_LO, "RSAC_F_LO"), (L.F_SAMPLER_OPENCV, "RSAC_F_SAMPLER_OPENCV"),
                           (L.F_EPNP, "RSAC_F_EPNP")):
            for extra in (0, L.F_REFINE):
                code, msg = _code_and_message(lib.rsac_fundamental_ransac, ctx.handle, a.ctypes.data, b.ctypes.data, 64,
                                              2000, THR, 0.99, SEED, L.F_ADAPTIVE | flag | extra, F.ctypes.data,
                                              mask.ctypes.data, C.byref(st), None)
                assert code == L.EINVAL and name in msg, msg
        med = C.c_double(0)
        code, msg = _code_and_message(lib.rsac_fundamental_lmeds, ctx.handle, a.ctypes.data, b.ctypes.data, 64, 2000,
                                      0.99, SEED, L.F_ADAPTIVE | L.F_REFINE, F.ctypes.data, mask.ctypes.data,
                                      C.byref(med), C.byref(st), None)
        assert code == L.EINVAL and "RSAC_F_REFINE" in msg
        for flag, name in ((L.F_DEVICE_OUT, "RSAC_F_DEVICE_OUT"), (L.F_REFINE, "RSAC_F_REFINE"),
                           (L.F_MSAC, "RSAC_F_MSAC")):
            code, msg = _code_and_message(lib.rsac_fundamental_fit_device, ctx.handle, a.ctypes.data, b.ctypes.data,
                                          64, None, flag, F.ctypes.data, None)
            assert code == L.EINVAL and name in msg, msg
        cnt, steps = C.c_int32(0), C.c_int32(0)

        def lo(thr, rounds, flags):
            return _code_and_message(lib.rsac_fundamental_local_opt, ctx.handle, a.ctypes.data, b.ctypes.data, 64,
                                     F.ctypes.data, thr, rounds, flags, F.ctypes.data, C.byref(cnt), C.byref(steps),
                                     mask.ctypes.data, None)

        for flag, name in ((L.F_ADAPTIVE, "RSAC_F_ADAPTIVE"), (L.F_REFINE, "RSAC_F_REFINE"), (L.F_LO, "RSAC_F_LO")):
            code, msg = lo(THR, 4, flag)
            assert code == L.EINVAL and name in msg, msg
        for rounds in (0, -3):
            code, msg = lo(THR, rounds, 0)
            assert code == L.EINVAL and "max_rounds" in msg
        for thr in (0.0, -1.0, float("nan"), float("inf"), 1e30):
            code, msg = lo(thr, 4, 0)
            assert code == L.EINVAL and "threshold" in msg, (thr, msg)


def test_last_stats_are_left_alone():
    ctx = L.context(0)
    pn = synth.pnp_problem(50, 0.3, seed=6)
    pr = R.problem(257, .3, 8)
    p1, p2 = pr["pts1"], pr["pts2"]
    ctx.set_timing(True)
    try:
        rsac.pnp_ransac(pn["points2d"], pn["points3d"], pn["K"], 5000, 30.0)
        before = ctx.last_stats()
        assert before["iters"] > 0
        F, mask = rsac.fundamental_ransac(p1, p2, THR, refine=True)
        assert ctx.last_stats() == before
        rsac.fundamental_ransac(p1, p2, THR, refine="lo")
        rsac.fundamental_fit(p1, p2, mask, device=0)
        rsac.fundamental_fit(_dev(p1), _dev(p2), _dev(mask))
        rsac.fundamental_local_opt(p1, p2, F, THR, max_rounds=8)
        rsac.fundamental_lmeds(p1, p2, refine=True)
        rsac.fundamental_lmeds(p1, p2, refine="lo")
        assert ctx.last_stats() == before
    finally:
        ctx.set_timing(False)
