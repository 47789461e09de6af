"""The seven-point fundamental matrix on the GPU (RSAC_F_FM_7POINT, k_fm_solve_g7).
Every comparison is exact equality of bits: the probe's records against the host solver
(rsac_fm_minimal7, the source the kernel runs) and the host scorers, the drivers against the scans
of tests/fm7ref.py replayed over the probe's records, the batched calls against the single ones.

A sample's subset is the oracle's Philox draw of 7 indices (pyoracle.philox_subset, in draw order:
the order of the rows decides the pivots, so it is part of the bits).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fm7ref as R  # noqa: E402
import pyoracle as O  # noqa: E402
import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

THR, SEED, CONF = 1.5, 0x5EED, 0.99
FAR = 1_000_003


def _bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _np(m):
    return m.cpu().numpy() if hasattr(m, "cpu") else np.asarray(m)


def _pts(n, ratio=0.3, seed=None):
    pr = R.problem(n, ratio, n if seed is None else seed)
    return pr["pts1"], pr["pts2"]


def _probe(p1, p2, samples, begin=0, **kw):
    return rsac.hypotheses("fundamental", p1, p2, hyp_begin=begin, n_hyps=samples, reproj_thresh=THR, seed=SEED,
                           minimal="7pt", **kw)


# ---------------------------------------------------------------------------------------------
# probes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 8, 9, 255, 256, 257, 1025])
def test_probe_equals_host_solver(n):
    p1, p2 = _pts(n)
    seen = set()
    for begin in (0, FAR):
        for samples in (1, 31, 32, 33, 65):  # the edges of the 32-sample block
            status, _, models = _probe(p1, p2, samples, begin)
            assert status.shape == (3 * samples,) and models.shape == (3 * samples, 16)
            for s in range(samples):
                idx = O.philox_subset(SEED, 0, begin + s, n, 7)
                assert idx is not None
                host = rsac.fundamental_minimal7(p1[idx], p2[idx])
                seen.add(len(host))
                for r in range(3):
                    tag = (n, begin, samples, s, r)
                    rec = models[3 * s + r]
                    if r < len(host):
                        assert status[3 * s + r] == 1 and rec[12] == 1.0, tag
                        assert _bits(rec[:9], host[r].ravel()), tag
                    else:
                        assert status[3 * s + r] == 0 and not rec[:9].any() and rec[12] == 0.0, tag
    if n >= 255:  # (7 points: every sample is the same 7 points, so one root count)
        assert {1, 3} <= seen  # one-root and three-root samples


def test_too_few_points_fail_every_draw():
    p1, p2 = _pts(9)
    status, counts, models = _probe(p1[:6], p2[:6], 5)
    assert (status == -1).all() and not counts.any() and not models[:, :9].any() and not models[:, 12].any()


@pytest.mark.parametrize("n", [64, 255, 256, 257, 1025])
def test_counts_costs_and_medians_equal_host(n):
    p1, p2 = _pts(n)
    samples = 33
    status, counts, models = _probe(p1, p2, samples)
    st_e, counts_e, models_e = _probe(p1, p2, samples, exact_only=True)
    st_c, counts_c, models_c, costs = rsac.fundamental_costs(p1, p2, 0, samples, THR, seed=SEED, minimal="7pt")
    st_m, med, models_m = rsac.hypotheses("fundamental", p1, p2, hyp_begin=0, n_hyps=samples, seed=SEED, minimal="7pt",
                                          medians=True)
    for st, mo in ((st_e, models_e), (st_c, models_c), (st_m, models_m)):
        assert np.array_equal(st, status) and _bits(mo[:, :9], models[:, :9])  # (slots 9 .. 11 are not the FM's)
    assert np.array_equal(counts, counts_e) and np.array_equal(counts, counts_c)  # pre-filter == exact
    assert (status == 0).any() and (status == 1).any()
    for h in range(3 * samples):
        if status[h] > 0:
            F = models[h, :9]
            assert (int(counts[h]), int(costs[h])) == rsac.fundamental_cost(p1, p2, F, THR), h
            assert med[h] == rsac.fm_median(p1, p2, F), h
        else:
            assert (counts[h], costs[h], med[h]) == (0, -1, -1.0), h


# ---------------------------------------------------------------------------------------------
# end-to-end replay
# ---------------------------------------------------------------------------------------------
def _rows(p1, p2, samples, score):
    if score == "msac":
        st, cnt, mo, cost = rsac.fundamental_costs(p1, p2, 0, samples, THR, seed=SEED, minimal="7pt")
        return st, cnt, mo, cost
    st, cnt, mo = _probe(p1, p2, samples)
    return st, cnt, mo, None


def _replay(p1, p2, score, max_iters):
    """the fm7ref scan over the probe's records of all max_iters samples -> (best, iters, good, F)"""
    n = len(p1)
    st, cnt, mo, cost = _rows(p1, p2, max_iters, score)
    if score == "msac":
        best, iters, good = R.scan_msac(st, cnt, cost, n, CONF, max_iters)
    else:
        best, iters, good = R.scan_count(st, cnt, n, CONF, max_iters)
    return best, iters, good, mo[best, :9].reshape(3, 3)


def _check_run(p1, p2, score, **kw):
    F, mask, info = rsac.fundamental_ransac(p1, p2, THR, seed=SEED, confidence=CONF, minimal="7pt", score=score,
                                            return_info=True, **kw)
    best, iters, good, Fr = _replay(p1, p2, score, kw.get("max_iters", 100_000))
    assert best >= 0 and F is not None
    assert (info.best_hyp, info.iters, info.n_inliers) == (best, iters, good), (info, best, iters, good)
    assert _bits(F, Fr)
    assert np.array_equal(_np(mask), O.fm_count(Fr, O.soa_hom(p1, p2), THR, mask=True)[1])
    assert int(_np(mask).sum()) == good
    return F, _np(mask), info


@pytest.mark.parametrize("score", ["count", "msac"])
def test_replay_within_the_first_round(score):
    # 10 % outliers: the scan ends inside the first round of 86 samples (the device's scan records
    # under "count")
    _, _, info = _check_run(*_pts(64, .1, 2), score, max_iters=5000)
    assert info.rounds == 1 and info.iters < 86


@pytest.mark.parametrize("score", ["count", "msac"])
def test_replay_into_the_second_round(score):
    # 30 % outliers: 41 of 64 inliers put the bound at 102 samples, past the first round's 86: the
    # device's scan records for round one, the rows for round two
    _, _, info = _check_run(*_pts(64, .3, 2), score, max_iters=5000)
    assert info.rounds == 2 and 86 < info.iters <= 258


@pytest.mark.parametrize("score", ["count", "msac"])
def test_replay_over_several_rounds(score):
    _, _, info = _check_run(*_pts(2000, .7, 4), score)
    assert info.rounds > 2 and info.hyps_scored % 3 == 0 and info.hyps_scored >= 3 * info.iters


@pytest.mark.parametrize("score", ["count", "msac"])
def test_replay_fixed_budget(score):
    _, _, info = _check_run(*_pts(2000, .7, 4), score, adaptive=False, max_iters=100)
    assert info.iters == 100 and info.hyps_scored == 300 and info.rounds == 1


def test_round_size_does_not_change_the_result():
    p1, p2 = _pts(64, .3, 2)
    want = _check_run(p1, p2, "count", max_iters=5000)
    ctx = L.context(0)
    ctx.set_round_size(100)  # not a multiple of 3: a round still covers whole samples (102 records)
    try:
        got = _check_run(p1, p2, "count", max_iters=5000)
    finally:
        ctx.set_round_size(4096)
    assert _bits(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[2].best_hyp, got[2].iters, got[2].n_inliers) == (want[2].best_hyp, want[2].iters, want[2].n_inliers)
    assert got[2].rounds > want[2].rounds and got[2].hyps_scored % 3 == 0


def test_seven_points_run_the_ordinary_loop():
    p1, p2 = _pts(7)
    F, mask, info = rsac.fundamental_ransac(p1, p2, THR, seed=SEED, minimal="7pt", return_info=True, max_iters=50)
    best, iters, good, Fr = _replay(p1, p2, "count", 50)
    assert best >= 0 and good == 7 and (info.best_hyp, info.iters, info.n_inliers) == (best, iters, good)
    assert _bits(F, Fr) and _np(mask).all()
    with pytest.raises(rsac.RsacError):
        rsac.fundamental_ransac(p1[:6], p2[:6], THR, minimal="7pt")


def test_refit_is_the_fit_of_the_winners_mask():
    p1, p2 = _pts(257, .3, 8)
    F0, mask0 = rsac.fundamental_ransac(p1, p2, THR, seed=SEED, minimal="7pt")
    F, mask = rsac.fundamental_ransac(p1, p2, THR, seed=SEED, minimal="7pt", refine=True)
    assert np.array_equal(_np(mask), _np(mask0))
    fit = rsac.fundamental_fit(p1, p2, _np(mask))
    assert fit is not None and _bits(F, fit) and not _bits(F, F0)


# ---------------------------------------------------------------------------------------------
# LMedS and the batched calls
# ---------------------------------------------------------------------------------------------
def _lmeds_reference(p1, p2, samples):
    n = len(p1)
    st, med, mo = rsac.hypotheses("fundamental", p1, p2, hyp_begin=0, n_hyps=samples, seed=SEED, minimal="7pt",
                                  medians=True)
    best, bm = R.scan_lmeds(st, med, samples)
    assert best >= 0
    F = mo[best, :9].reshape(3, 3)
    sigma = rsac.lmeds_sigma(bm, n, 7)
    count, mask = O.fm_count(F, O.soa_hom(p1, p2), sigma, mask=True)
    return best, bm, F, mask, count


@pytest.mark.parametrize("key", [(64, .3, 2), (257, .3, 8)])
def test_lmeds_equals_the_restated_scan(key):
    p1, p2 = _pts(*key)
    samples = rsac.lmeds_num_iters(CONF, 2000, 7)
    assert samples == max(rsac.update_num_iters(CONF, 0.45, 7, 2000), 3)
    F, mask, info = rsac.fundamental_lmeds(p1, p2, confidence=CONF, seed=SEED, minimal="7pt", return_info=True)
    best, bm, Fr, mr, count = _lmeds_reference(p1, p2, samples)
    assert count >= 7 and F is not None
    assert (info.best_hyp, info.iters, info.hyps_scored) == (best, samples, 3 * samples)
    assert info.median == bm and _bits(F, Fr)
    assert np.array_equal(_np(mask), mr) and info.n_inliers == count


def test_lmeds_point_counts():
    p1, p2 = _pts(9)
    with pytest.raises(rsac.RsacError) as e:
        rsac.fundamental_lmeds(p1[:7], p2[:7], minimal="7pt")
    assert e.value.code == L.ETOOFEW
    F, mask, info = rsac.fundamental_lmeds(p1[:8], p2[:8], seed=SEED, minimal="7pt", n_iters=40, return_info=True)
    best, bm, Fr, mr, count = _lmeds_reference(p1[:8], p2[:8], 40)
    assert info.iters == 40 and info.median == bm
    if count >= 7:
        assert _bits(F, Fr) and np.array_equal(_np(mask), mr)
    else:
        assert F is None and not _np(mask).any()
    with pytest.raises(rsac.RsacError):  # the 8-point rule is unchanged: n >= 9
        rsac.fundamental_lmeds(p1[:8], p2[:8])


SIZES = (8, 64, 257, 1025)


@pytest.mark.parametrize("sizes", [(257,), SIZES], ids=["P1", "P4"])
def test_batched_equals_single(sizes):
    pts = [_pts(n) for n in sizes]
    a, b = [p[0] for p in pts], [p[1] for p in pts]
    for kw in (dict(score="count"), dict(score="msac"), dict(score="count", refine=True)):
        rows = rsac.fundamental_ransac_batched(a, b, THR, seed=SEED, minimal="7pt", **kw)
        for (p1, p2), row in zip(pts, rows):
            F, mask, info = rsac.fundamental_ransac(p1, p2, THR, seed=SEED, minimal="7pt", max_iters=2000,
                                                    return_info=True, **kw)
            tag = (len(p1), kw)
            assert (F is None) == (row[0] is None), tag
            assert F is None or _bits(row[0], F), tag
            assert np.array_equal(_np(row[1]), _np(mask)) and row[2] == info.n_inliers, tag
            if kw["score"] == "msac":
                assert row[3] == info.cost, tag
    rows = rsac.fundamental_lmeds_batched(a, b, seed=SEED, minimal="7pt")
    for (p1, p2), row in zip(pts, rows):
        F, mask, info = rsac.fundamental_lmeds(p1, p2, seed=SEED, minimal="7pt", return_info=True)
        assert (F is None) == (row[0] is None), len(p1)
        assert F is None or _bits(row[0], F), len(p1)
        assert np.array_equal(_np(row[1]), _np(mask)) and row[2] == info.n_inliers, len(p1)
        assert row[3] == (info.median if F is not None else -1.0), len(p1)


def test_eight_point_path_is_unchanged():
    p1, p2 = _pts(257, .3, 8)
    ref = O.fm_ransac(p1, p2, THR, CONF, 2000, SEED)
    F, mask, info = rsac.fundamental_ransac(p1, p2, THR, seed=SEED, max_iters=2000, return_info=True)
    assert (info.best_hyp, info.iters, info.n_inliers) == (ref["best"], ref["iters"], ref["n_inliers"])
    assert _bits(F, ref["F"]) and np.array_equal(_np(mask), ref["mask"])
    (Fb, mb, nb), = rsac.fundamental_ransac_batched([p1], [p2], THR, seed=SEED)
    assert _bits(Fb, ref["F"]) and np.array_equal(_np(mb), ref["mask"]) and nb == ref["n_inliers"]


def test_flag_is_refused_outside_the_fundamental_matrix_calls():
    p1, p2 = _pts(64, .3, 2)
    ctx = L.context(0)
    lib = L.lib()
    counts, status = np.zeros(8, np.int32), np.zeros(8, np.int8)
    H, m = np.zeros(9), np.zeros(64, np.uint8)
    with ctx.lock:
        code = lib.rsac_homography_hypotheses(ctx.handle, p1.ctypes.data, p2.ctypes.data, 64, 0, 8, 3.0, SEED,
                                              L.F_FM_7POINT, None, counts.ctypes.data, status.ctypes.data, None, None)
        assert code == L.EINVAL and b"RSAC_F_FM_7POINT" in lib.rsac_last_error()
        code = lib.rsac_homography_ransac(ctx.handle, p1.ctypes.data, p2.ctypes.data, 64, 100, 3.0, 0.99, SEED,
                                          L.F_FM_7POINT, H.ctypes.data, m.ctypes.data, None, None)
        assert code == L.EINVAL and b"RSAC_F_FM_7POINT" in lib.rsac_last_error()
        K, p3 = np.eye(3), np.zeros((64, 3))
        code = lib.rsac_pnp_hypotheses(ctx.handle, p3.ctypes.data, p1.ctypes.data, 64, K.ctypes.data, 0, 8, 30.0, SEED,
                                       L.F_FM_7POINT, None, counts.ctypes.data, status.ctypes.data, None, None)
        assert code == L.EINVAL and b"RSAC_F_FM_7POINT" in lib.rsac_last_error()
        code = lib.rsac_fundamental_fit_device(ctx.handle, p1.ctypes.data, p2.ctypes.data, 64, None, L.F_FM_7POINT,
                                               H.ctypes.data, None)
        assert code == L.EINVAL and b"RSAC_F_FM_7POINT" in lib.rsac_last_error()
