"""The batched fundamental-matrix calls on the GPU (rsac_fundamental_ransac_batched, _lmeds_batched,
_fit_batched_device, _local_opt_batched; k_fm_fit_sums_b, k_fm_fit_finish_b): every comparison is
exact equality, per problem, with the CPU chains composed in tests/fmbatchref.py -- the C oracle's
count loop, fmrobustref's MSAC and LMedS, the host fit and fmfitref's local optimisation.

A batch's kernels are chosen by its largest problem (kLanePts = 256 points: a lane per hypothesis;
up to 512: the wave median; above: the block median), so the batches below put the same small
problems under each of them: a 12-point problem is served by another kernel than in its own call.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fmbatchref as B  # noqa: E402
import fmfitref as FR  # noqa: E402
import pyoracle as O  # noqa: E402
import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402
from rsac import synth  # noqa: E402

pytestmark = pytest.mark.gpu

THR, SEED, CONF = B.THR, B.SEED, B.CONF
LANE = [(9, 0, 1), (12, .25, 5), (64, .3, 2), (256, .3, 8)]
WAVE = [(12, .25, 5), (257, .3, 8), (300, .5, 4)]
BLOCK = [(12, .25, 5), (257, .3, 8), (1025, .3, 6)]
REFINE = [(64, .3, 2), (4097, .5, 4), (257, .3, 8)]  # the middle problem has two ranges
TABLE = dict(FR.TABLE)


def _np(m):
    return m.cpu().numpy() if hasattr(m, "cpu") else np.asarray(m)


def _dev(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device="cuda", dtype=dtype)


def _lists(keys):
    pts = [B.points(k) for k in keys]
    return [p[0] for p in pts], [p[1] for p in pts]


def _run(rule, keys, budget=None, **kw):
    """the batched call of one rule -> rows of (F, mask, n_inliers[, cost | median])"""
    a, b = _lists(keys)
    if rule == "lmeds":
        return rsac.fundamental_lmeds_batched(a, b, n_iters=budget, **kw)
    if budget is not None:
        kw.update(adaptive=False, max_iters=budget)
    return rsac.fundamental_ransac_batched(a, b, THR, score=rule, **kw)


def _check_rows(rule, rows, refs, what=""):
    assert len(rows) == len(refs)
    for p, (row, ref) in enumerate(zip(rows, refs)):
        tag = (what, rule, p)
        assert B.bits_equal(row[0], ref["F"]), tag
        assert np.array_equal(_np(row[1]), ref["mask"]), tag
        assert row[2] == ref["n_inliers"] == int(ref["mask"].sum()), tag
        if rule == "msac":
            assert row[3] == ref["cost"], tag
        if rule == "lmeds":
            assert row[3] == ref["median"], tag


def _check(rule, keys, budget=None, **kw):
    refs = [B.chain(rule, k, budget) for k in keys]
    if budget is None:  # the chains are the pinned ones
        for k, ref in zip(keys, refs):
            assert B.summary(rule, ref) == B.pinned(rule, k), (rule, k)
    rows = _run(rule, keys, budget, **kw)
    _check_rows(rule, rows, refs, str(keys))
    return rows


# ---------------------------------------------------------------------------------------------
# the three rules under each kernel selection
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["count", "msac", "lmeds"])
@pytest.mark.parametrize("budget", [None, 300], ids=["adaptive", "fixed300"])
def test_lane_batch(rule, budget):
    _check(rule, LANE, budget)


@pytest.mark.parametrize("keys", [WAVE, BLOCK], ids=["wave", "block"])
def test_wave_and_block_batches(keys):
    pre = _check("count", keys)  # the f32 pre-filter on
    exact = _check("count", keys, exact_only=True)
    for a, b in zip(pre, exact):
        assert B.bits_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    _check("msac", keys)
    _check("lmeds", keys)


def test_prefilter_bounds_are_per_problem():
    """a problem and its copy scaled by 4 (exact in f32) in one call: every problem's pre-filter works
    from its own coordinate bounds, and the scaled copy equals the oracle on the scaled points"""
    p1, p2 = B.points((256, .3, 8))
    q1, q2 = B.points((12, .25, 5))
    s1, s2 = p1 * 4.0, p2 * 4.0
    for a, b in ((p1, s1), (p2, s2)):
        assert np.array_equal(a.astype(np.float32) * np.float32(4), b.astype(np.float32))
    refs = [B.count((256, .3, 8)), B.count_of(s1, s2), B.count((12, .25, 5))]
    assert refs[1]["best"] >= 0
    for kw in ({}, dict(exact_only=True)):
        rows = rsac.fundamental_ransac_batched([p1, s1, q1], [p2, s2, q2], THR, **kw)
        _check_rows("count", rows, refs, str(kw))
    # the 257-point twin: the pre-filter kernel itself (a batch above kLanePts)
    p1, p2 = B.points((257, .3, 8))
    s1, s2 = p1 * 4.0, p2 * 4.0
    refs = [B.count((257, .3, 8)), B.count_of(s1, s2), B.count((12, .25, 5))]
    rows = rsac.fundamental_ransac_batched([p1, s1, q1], [p2, s2, q2], THR)
    _check_rows("count", rows, refs, "257")


@pytest.mark.parametrize("H", [33, 257])
def test_hypothesis_count_not_a_multiple_of_32(H):
    """P > 1 and H % 32 != 0: the pre-filter's per-problem count rows are cleared with a pitch, and
    its last tile is short"""
    pre = _check("count", WAVE, H)
    exact = _check("count", WAVE, H, exact_only=True)
    for a, b in zip(pre, exact):
        assert B.bits_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    _check("msac", WAVE, H)


# ---------------------------------------------------------------------------------------------
# refine=True and refine="lo"
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["count", "msac"])
def test_refine_true(rule):
    keys = REFINE if rule == "count" else [(64, .3, 2), (257, .3, 8), (12, .25, 5)]  # (4097's MSAC chain: a minute)
    refs = [B.chain(rule, k) for k in keys]
    plain = _run(rule, keys)
    rows = _run(rule, keys, refine=True)
    for k, ref, r0, r1 in zip(keys, refs, plain, rows):
        p1, p2 = B.points(k)
        assert np.array_equal(r1[1], ref["mask"]) and r1[2:] == r0[2:]  # the RANSAC phase's mask, count, cost
        want = B.host_fit(p1, p2, ref["mask"])
        if want is None:  # 12 points, 8 inliers: no fit, the minimal F stays
            want = ref["F"]
        assert B.bits_equal(r1[0], want), k
        if rule == "count" and k in TABLE and B.summary("count", ref)[0] == TABLE[k][0]:
            assert O.fm_count(r1[0], O.soa_hom(p1, p2), THR) == TABLE[k][2]
    assert not B.bits_equal(rows[0][0], plain[0][0])


def test_refine_lo():
    refs = [B.count(k) for k in REFINE]
    rows = _run("count", REFINE, refine="lo")
    for k, ref, row in zip(REFINE, refs, rows):
        p1, p2 = B.points(k)
        rF, rmask, rcount, rsteps = B.local_opt(p1, p2, ref["F"], THR, 4)
        assert B.bits_equal(row[0], rF) and np.array_equal(row[1], rmask) and row[2] == rcount, k
        if ref["best"] == TABLE[k][0] and TABLE[k][4] <= 4:  # the table's winner, its loop within 4 rounds
            assert (rcount, rsteps) == TABLE[k][3:5]


@pytest.mark.parametrize("cap", [1, 4, 8])
def test_local_opt_batched(cap):
    """the loop itself: rounds and counts against the table, a problem without a model, one that never
    rises, device inputs"""
    keys = [(64, .3, 2), (4097, .5, 4), (257, .3, 8), (1025, .3, 6)]
    a, b = _lists(keys)
    F0 = [FR.winner_from_index(k, TABLE[k][0])[0] for k in keys]
    flat = np.array([[0, 0, 1.0], [0, 0, 0], [0, 0, 0]])  # x2 = 0: fewer than 8 points within 1.5 px
    a, b, F0 = a + [a[2], a[0]], b + [b[2], b[0]], F0 + [flat, None]
    want = [B.local_opt(p1, p2, F, THR, cap) if F is not None else (None, np.zeros(len(p1), bool), 0, 0)
            for p1, p2, F in zip(a, b, F0)]
    for k, w in zip(keys, want):
        _, c0, c1, c8, steps8, _ = TABLE[k]
        if cap == 1:
            assert w[2:] == ((c1, 1) if c1 > c0 else (c0, 0))
        if cap == 8:
            assert w[2:] == (c8, steps8)
    assert want[4][3] == 0 and want[4][2] < 8
    host = rsac.fundamental_local_opt_batched(a, b, F0, THR, max_rounds=cap)
    dev = rsac.fundamental_local_opt_batched([_dev(x) for x in a], [_dev(x) for x in b], F0, THR, max_rounds=cap)
    assert all(r[1].is_cuda for r in dev)
    for p, w in enumerate(want):
        for r in (host[p], dev[p]):
            assert B.bits_equal(r[0], w[0]) and np.array_equal(_np(r[1]), w[1]) and r[2:] == w[2:], (p, cap)


@pytest.mark.parametrize("key", [(64, .3, 2), (1025, .3, 6)], ids=["64", "1025"])
@pytest.mark.parametrize("cap", [1, 8])
def test_one_problem_through_the_batched_door_equals_the_single_door(key, cap):
    """one loop, two fit callables (the batched kernels and the single fit): one range of the fit's
    summation order (64 points) and the first size with a second range (1025)"""
    p1, p2 = B.points(key)
    F0 = FR.winner_from_index(key, TABLE[key][0])[0]
    (bF, bmask, bcount, bsteps), = rsac.fundamental_local_opt_batched([p1], [p2], [F0], THR, max_rounds=cap)
    F, mask, count, steps = rsac.fundamental_local_opt(p1, p2, F0, THR, max_rounds=cap)
    assert B.bits_equal(bF, F) and np.array_equal(bmask, mask)
    assert (bcount, bsteps) == (count, steps) and count == int(mask.sum())


def test_lmeds_refine():
    keys = [(64, .3, 2), (257, .3, 8), (12, .25, 5)]
    refs = [B.lmeds(k) for k in keys]
    rows = _run("lmeds", keys, refine=True)
    for k, ref, row in zip(keys, refs, rows):
        p1, p2 = B.points(k)
        want = B.host_fit(p1, p2, ref["mask"])
        assert B.bits_equal(row[0], ref["F"] if want is None else want), k
        assert np.array_equal(row[1], ref["mask"]) and row[2:] == (ref["n_inliers"], ref["median"])
    rows = _run("lmeds", keys, refine="lo")
    for k, ref, row in zip(keys, refs, rows):
        p1, p2 = B.points(k)
        rF, rmask, rcount, _ = B.local_opt(p1, p2, ref["F"], rsac.lmeds_sigma(ref["median"], k[0], 8), 4)
        assert B.bits_equal(row[0], rF) and np.array_equal(row[1], rmask) and row[2] == rcount, k


# ---------------------------------------------------------------------------------------------
# fundamental_fit_batched
# ---------------------------------------------------------------------------------------------
FIT_SIZES = [7, 8, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 8193]


def _fit_problem(n):
    pr = synth.fundamental_problem(n, 0.0 if n < 20 else 0.3, seed=100 + n)
    return pr["pts1"], pr["pts2"]


def _fit_masks(kind, sizes):
    out = []
    for i, n in enumerate(sizes):
        if kind == "third":
            m = np.arange(n) % 3 != 0
        elif kind in ("eight", "seven"):  # the first four and the last four points (the last range's end)
            m = np.zeros(n, bool)
            m[:4] = m[max(n - 4, 4):] = True
            if kind == "seven":
                m[n - 1] = False
        else:  # "hole": one problem entirely masked out, its neighbours whole
            m = np.full(n, sizes[i] != 4096)
        out.append(m)
    return out


@pytest.mark.parametrize("order", ["rising", "falling"])
def test_fit_batched_equals_host_fit(order):
    """falling: a one-range problem follows a three-range one (8193, 4097, 4096, ...)"""
    sizes = FIT_SIZES if order == "rising" else FIT_SIZES[::-1]
    pts = [_fit_problem(n) for n in sizes]
    a, b = [p[0] for p in pts], [p[1] for p in pts]
    da, db = [_dev(x) for x in a], [_dev(x) for x in b]
    for kind in (None, "third", "eight", "seven", "hole"):
        masks = None if kind is None else _fit_masks(kind, sizes)
        want = [B.host_fit(p1, p2, None if masks is None else masks[i]) for i, (p1, p2) in enumerate(pts)]
        ones = [n if masks is None else int(masks[i].sum()) for i, n in enumerate(sizes)]
        assert [w is None for w in want] == [c < 8 for c in ones], kind
        if kind == "eight":
            assert all(c == 8 for n, c in zip(sizes, ones) if n >= 8)
        got = rsac.fundamental_fit_batched(a, b, masks)
        dgot = rsac.fundamental_fit_batched(da, db, None if masks is None else [_dev(m) for m in masks])
        for i, w in enumerate(want):
            assert B.bits_equal(got[i], w), (kind, sizes[i])
            assert B.bits_equal(dgot[i], w), (kind, sizes[i], "device")


# ---------------------------------------------------------------------------------------------
# the batched call against the single GPU calls, and the residence flags of the C ABI
# ---------------------------------------------------------------------------------------------
MIXED = [(300, .5, 4), (12, .25, 5), (1025, .3, 6), (64, .3, 2)]


@pytest.mark.parametrize("rule", ["count", "msac", "lmeds"])
def test_batched_equals_single_calls(rule):
    a, b = _lists(MIXED)
    rows = _run(rule, MIXED)
    for p, (p1, p2) in enumerate(zip(a, b)):
        if rule == "lmeds":
            F, m, info = rsac.fundamental_lmeds(p1, p2, return_info=True)
            tail = (info.n_inliers, info.median)
        else:
            F, m, info = rsac.fundamental_ransac(p1, p2, THR, max_iters=B.MAX_ITERS, score=rule, return_info=True)
            tail = (info.n_inliers, info.cost) if rule == "msac" else (info.n_inliers,)
        assert B.bits_equal(rows[p][0], F) and np.array_equal(rows[p][1], m) and rows[p][2:] == tail, (rule, p)


def _flat(keys):
    a, b = _lists(keys)
    off = np.zeros(len(keys) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in a])
    return np.ascontiguousarray(np.concatenate(a)), np.ascontiguousarray(np.concatenate(b)), off


@pytest.mark.parametrize("rule", ["count", "refine", "msac", "lmeds"])
def test_device_pointers_equal_host_pointers(rule):
    """the C ABI directly: host pointers, DEVICE_IN | DEVICE_OUT, DEVICE_SOA | DEVICE_OUT"""
    import torch
    a, b, off = _flat(MIXED)
    P, N = len(MIXED), int(off[-1])
    ctx, lib = L.context(0), L.lib()
    base = {"count": L.F_ADAPTIVE, "refine": L.F_ADAPTIVE | L.F_REFINE, "msac": L.F_ADAPTIVE | L.F_MSAC,
            "lmeds": L.F_ADAPTIVE}[rule]

    def call(pa, pb, flags, mptr):
        F, st, ni, med = np.zeros((P, 9)), np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P)
        with ctx.lock:
            if rule == "lmeds":
                L.check(lib.rsac_fundamental_lmeds_batched(ctx.handle, pa, pb, off.ctypes.data, P, B.MAX_ITERS, CONF,
                                                           SEED, flags, F.ctypes.data, st.ctypes.data, ni.ctypes.data,
                                                           med.ctypes.data, mptr, None))
            else:
                L.check(lib.rsac_fundamental_ransac_batched(ctx.handle, pa, pb, off.ctypes.data, P, B.MAX_ITERS, THR,
                                                            CONF, SEED, flags, F.ctypes.data, st.ctypes.data,
                                                            ni.ctypes.data, mptr, None))
            costs = np.zeros(P, np.int64)
            if rule == "msac":
                L.check(lib.rsac_last_costs(ctx.handle, costs.ctypes.data, P))
        return F, st, ni, med, costs

    hmask = np.zeros(N, np.uint8)
    want = call(a.ctypes.data, b.ctypes.data, base, hmask.ctypes.data)
    assert (want[1] == L.OK).all()
    ta, tb = _dev(a), _dev(b)
    sa, sb = _dev(a.T, torch.float32), _dev(b.T, torch.float32)
    for pa, pb, fl in ((ta, tb, L.F_DEVICE_IN), (sa, sb, L.F_DEVICE_SOA)):
        dmask = torch.zeros(N, dtype=torch.uint8, device="cuda")
        got = call(pa.data_ptr(), pb.data_ptr(), base | fl | L.F_DEVICE_OUT, dmask.data_ptr())
        torch.cuda.synchronize()
        for w, g in zip(want, got):
            assert np.array_equal(w.view(np.uint8), g.view(np.uint8)), (rule, fl)
        assert np.array_equal(dmask.cpu().numpy(), hmask), (rule, fl)


# ---------------------------------------------------------------------------------------------
# error paths, statistics
# ---------------------------------------------------------------------------------------------
def _code_and_message(fn, *args):
    with pytest.raises(L.RsacError) as e:
        L.check(fn(*args))
    return e.value.code, str(e.value)


def test_error_paths():
    a, b, off = _flat([(64, .3, 2), (12, .25, 5)])
    short = off.copy()
    ctx, lib = L.context(0), L.lib()
    P, N = 2, int(off[-1])
    F, st, ni, med, mask = np.zeros((P, 9)), np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P), np.zeros(N, np.uint8)

    def ransac(o, flags):
        return _code_and_message(lib.rsac_fundamental_ransac_batched, ctx.handle, a.ctypes.data, b.ctypes.data,
                                 o.ctypes.data, P, 2000, THR, CONF, SEED, flags, F.ctypes.data, st.ctypes.data,
                                 ni.ctypes.data, mask.ctypes.data, None)

    def lmeds(o, flags):
        return _code_and_message(lib.rsac_fundamental_lmeds_batched, ctx.handle, a.ctypes.data, b.ctypes.data,
                                 o.ctypes.data, P, 2000, CONF, SEED, flags, F.ctypes.data, st.ctypes.data,
                                 ni.ctypes.data, med.ctypes.data, mask.ctypes.data, None)

    with ctx.lock:
        short[2] = short[1] + 7
        assert ransac(short, L.F_ADAPTIVE)[0] == L.ETOOFEW
        short[2] = short[1] + 8
        assert lmeds(short, L.F_ADAPTIVE)[0] == L.ETOOFEW
        for flag, name in ((L.F_SAMPLER_OPENCV, "RSAC_F_SAMPLER_OPENCV"), (L.F_LO, "RSAC_F_LO"),
                           (L.F_EPNP, "RSAC_F_EPNP"), (L.F_ASYNC, "RSAC_F_ASYNC")):
            code, msg = ransac(off, L.F_ADAPTIVE | flag)
            assert code == L.EINVAL and name in msg, msg
        for flag, name in ((L.F_REFINE, "RSAC_F_REFINE"), (L.F_MSAC, "RSAC_F_MSAC"), (L.F_LO, "RSAC_F_LO")):
            code, msg = lmeds(off, L.F_ADAPTIVE | flag)
            assert code == L.EINVAL and name in msg, msg
        code, msg = _code_and_message(lib.rsac_fundamental_fit_batched_device, ctx.handle, a.ctypes.data, b.ctypes.data,
                                      off.ctypes.data, P, None, L.F_DEVICE_OUT, F.ctypes.data, st.ctypes.data, None)
        assert code == L.EINVAL and "RSAC_F_DEVICE_OUT" in msg
        cnt, steps = np.zeros(P, np.int32), np.zeros(P, np.int32)
        for rounds, thr, flags, word in ((0, THR, 0, "max_rounds"), (4, 0.0, 0, "threshold"),
                                         (4, THR, L.F_REFINE, "RSAC_F_REFINE")):
            code, msg = _code_and_message(lib.rsac_fundamental_local_opt_batched, ctx.handle, a.ctypes.data,
                                          b.ctypes.data, off.ctypes.data, P, F.ctypes.data, thr, rounds, flags,
                                          F.ctypes.data, cnt.ctypes.data, steps.ctypes.data, mask.ctypes.data, None)
            assert code == L.EINVAL and word in msg, msg
    # rsac_last_costs answers for the last MSAC call's P alone
    rsac.fundamental_ransac_batched(*_lists([(64, .3, 2), (12, .25, 5)]), THR, score="msac")
    costs = np.zeros(3, np.int64)
    with ctx.lock:
        assert lib.rsac_last_costs(ctx.handle, costs.ctypes.data, 2) == L.OK
        assert tuple(costs[:2]) == (B.pinned("msac", (64, .3, 2))[2], B.pinned("msac", (12, .25, 5))[2])
        assert _code_and_message(lib.rsac_last_costs, ctx.handle, costs.ctypes.data, 3)[0] == L.EINVAL
        assert _code_and_message(lib.rsac_last_costs, ctx.handle, costs.ctypes.data, 1)[0] == L.EINVAL


def test_a_problem_without_a_model_reports_a_zero_row():
    """8 collinear correspondences beside a solvable problem: status NO_MODEL, F None, mask zero, and the
    call still succeeds; refine leaves it alone"""
    p1, p2 = B.points((64, .3, 2))
    t = np.arange(8.0)
    line = np.stack([t, 2 * t], 1)
    ref = B.count_of(line, line)
    assert ref["best"] < 0
    for refine in (False, True, "lo"):
        rows = rsac.fundamental_ransac_batched([line, p1], [line, p2], THR, refine=refine)
        assert rows[0][0] is None and not rows[0][1].any() and rows[0][2] == 0
        assert rows[1][0] is not None


def test_timing_figures_reach_last_stats():
    ctx = L.context(0)
    a, b = _lists(WAVE)
    ctx.set_timing(True)
    try:
        rsac.fundamental_ransac_batched(a, b, THR)
        st = ctx.last_stats()
        ref = B.count(WAVE[0])
        assert (st["best_hyp"], st["n_inliers"], st["iters"]) == (ref["best"], ref["n_inliers"], ref["iters"])
        assert st["rounds"] >= 1 and st["hyps_scored"] >= ref["iters"]
        rsac.fundamental_lmeds_batched(a, b)
        st = ctx.last_stats()
        assert st["best_hyp"] == B.lmeds(WAVE[0])["best"] and st["rounds"] == 1
        assert st["hyps_scored"] == rsac.lmeds_num_iters(CONF, B.MAX_ITERS, 8)
        before = ctx.last_stats()
        rsac.fundamental_fit_batched(a, b)
        rsac.fundamental_local_opt_batched(a, b, [np.eye(3)] * 3)
        assert ctx.last_stats() == before
    finally:
        ctx.set_timing(False)
