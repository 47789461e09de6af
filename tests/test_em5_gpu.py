"""The five-point essential matrix on the GPU (k_em_solve_g5).  Every comparison but
the last test's angles is exact equality of bits: the probe's records against the host solver
(rsac_em_minimal5, the source the kernel runs) and the host scorers, the drivers against the scans of
tests/em5ref.py replayed over the probe's records, the batched call against the single one.

A sample's subset is the oracle's Philox draw of 5 indices (pyoracle.philox_subset, in draw order:
the order of the rows decides the pivots, so it is part of the bits).
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import em5ref as R  # noqa: E402
import pyoracle as O  # noqa: E402
import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

THR, SEED, CONF = 1.5, 0x5EED, 0.99
RPS = R.RPS


def _bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _np(m):
    return m.cpu().numpy() if hasattr(m, "cpu") else np.asarray(m)


def _pts(n, ratio=0.3, seed=None):
    pr = R.problem(n, ratio, n if seed is None else seed)
    return pr["pts1"], pr["pts2"], pr["K"]


def _K2(K):
    return K * np.array([[1.05, 1.0, 0.98], [1.0, 0.97, 1.01], [1.0, 1.0, 1.0]])


def _probe(p1, p2, K, samples, begin=0, **kw):
    return rsac.hypotheses("essential", p1, p2, K=K, hyp_begin=begin, n_hyps=samples, reproj_thresh=THR, seed=SEED, **kw)


def _check_rows(status, models, p1, p2, K, K2, samples, begin, tag):
    n = len(p1)
    seen = set()
    assert status.shape == (RPS * samples,) and models.shape == (RPS * samples, 16)
    for s in range(samples):
        idx = O.philox_subset(SEED, 0, begin + s, n, 5)
        assert idx is not None
        host = rsac.essential_minimal5(p1[idx], p2[idx], K, K2)
        seen.add(len(host))
        for r in range(RPS):
            rec = models[RPS * s + r]
            if r < len(host):
                assert status[RPS * s + r] == 1 and rec[12] == 1.0, (tag, s, r)
                assert _bits(rec[:9], host[r].ravel()), (tag, s, r)
            else:
                assert status[RPS * s + r] == 0 and not rec[:9].any() and rec[12] == 0.0, (tag, s, r)
    return seen


# ---------------------------------------------------------------------------------------------
# probes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 6, 12, 13, 64, 257, 2049])
def test_probe_equals_host_solver(n):
    p1, p2, K = _pts(n)
    seen = set()
    for begin, samples in ((0, 1), (0, 17), (4096, 17), (0, 512)):
        status, _, models = _probe(p1, p2, K, samples, begin)
        seen |= _check_rows(status, models, p1, p2, K, None, samples, begin, (n, begin, samples))
    if n == 257:
        assert {2, 4, 6} <= seen


def test_probe_two_views_device_and_soa_inputs():
    torch = pytest.importorskip("torch")
    p1, p2, K = _pts(257)
    K2 = _K2(K)
    want = _probe(p1, p2, K, 17, 4096, K2=K2)
    _check_rows(want[0], want[2], p1, p2, K, K2, 17, 4096, "K2")
    d1, d2 = torch.as_tensor(p1, device="cuda"), torch.as_tensor(p2, device="cuda")
    s1 = torch.as_tensor(p1.T.astype(np.float32), device="cuda").contiguous()
    s2 = torch.as_tensor(p2.T.astype(np.float32), device="cuda").contiguous()
    for a, b in ((d1, d2), (s1, s2)):
        got = _probe(a, b, K, 17, 4096, K2=K2)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert _bits(got[2][:, :9], want[2][:, :9])


def test_too_few_points_fail_every_draw():
    p1, p2, K = _pts(12)
    status, counts, models = _probe(p1[:4], p2[:4], K, 5)
    assert (status == -1).all() and not counts.any() and not models[:, :9].any() and not models[:, 12].any()
    with pytest.raises(rsac.RsacError) as e:
        rsac.essential_ransac(p1[:4], p2[:4], K)
    assert e.value.code == L.ETOOFEW


@pytest.mark.parametrize("n", [13, 257, 2049])
def test_counts_and_costs_equal_host(n):
    p1, p2, K = _pts(n)
    samples = 33
    status, counts, models = _probe(p1, p2, K, samples)                          # the f32 pre-filter records
    st_e, counts_e, models_e = _probe(p1, p2, K, samples, exact_only=True)
    st_c, counts_c, models_c, costs = _probe(p1, p2, K, samples, costs=True)
    for st, mo in ((st_e, models_e), (st_c, models_c)):
        assert np.array_equal(st, status) and _bits(mo[:, :9], models[:, :9])
    assert np.array_equal(counts, counts_e) and np.array_equal(counts, counts_c)  # pre-filter == exact
    assert (status == 0).any() and (status == 1).any()
    for h in range(RPS * samples):
        if status[h] > 0:
            assert (int(counts[h]), int(costs[h])) == rsac.fundamental_cost(p1, p2, models[h, :9], THR), h
        else:
            assert (counts[h], costs[h]) == (0, -1), h


# ---------------------------------------------------------------------------------------------
# end-to-end replay
# ---------------------------------------------------------------------------------------------
def _replay(p1, p2, K, score, max_iters):
    """the em5ref scan over the probe's records of all max_iters samples -> (best, iters, good, F)"""
    n = len(p1)
    if score == "msac":
        st, cnt, mo, cost = _probe(p1, p2, K, max_iters, costs=True)
        best, iters, good = R.scan_msac(st, cnt, cost, n, CONF, max_iters)
    else:
        st, cnt, mo = _probe(p1, p2, K, max_iters)
        best, iters, good = R.scan_count(st, cnt, n, CONF, max_iters)
    return best, iters, good, mo[best, :9].reshape(3, 3)


def _check_run(p1, p2, K, score, max_iters=1000, **kw):
    E, mask, F, info = rsac.essential_ransac(p1, p2, K, THR, seed=SEED, confidence=CONF, score=score, max_iters=max_iters,
                                             return_info=True, return_F=True, **kw)
    best, iters, good, Fr = _replay(p1, p2, K, score, max_iters)
    assert best >= 0 and E is not None
    assert (info.best_hyp, info.iters, info.n_inliers) == (best, iters, good), (info, best, iters, good)
    assert _bits(F, Fr) and _bits(E, rsac.essential_from_fundamental(Fr, K))
    assert np.array_equal(_np(mask), O.fm_count(Fr, O.soa_hom(p1, p2), THR, mask=True)[1])
    assert int(_np(mask).sum()) == good
    return E, _np(mask), info


@pytest.mark.parametrize("score", ["count", "msac"])
def test_replay_within_the_first_round(score):
    # 10 % outliers: the scan ends after 9 samples, inside the first round of 26
    _, _, info = _check_run(*_pts(64, .1, 2), score)
    assert info.rounds == 1 and info.iters < 26


@pytest.mark.parametrize("score", ["count", "msac"])
def test_replay_into_the_second_round(score):
    # 30 % outliers: 44 of 64 inliers put the bound at 28 samples, past the first round's 26
    _, _, info = _check_run(*_pts(64, .3, 2), score)
    assert info.rounds == 2 and 26 < info.iters <= 78


@pytest.mark.parametrize("score", ["count", "msac"])
def test_replay_over_several_rounds(score):
    _, _, info = _check_run(*_pts(64, .5, 2), score)
    assert info.rounds > 2 and info.hyps_scored % RPS == 0 and info.hyps_scored >= RPS * info.iters


@pytest.mark.parametrize("score", ["count", "msac"])
def test_replay_fixed_budget(score):
    _, _, info = _check_run(*_pts(64, .5, 2), score, adaptive=False, max_iters=100)
    assert info.iters == 100 and info.hyps_scored == 1000 and info.rounds == 1


def test_round_size_does_not_change_the_result():
    p1, p2, K = _pts(64, .5, 2)
    want = _check_run(p1, p2, K, "count")
    ctx = L.context(0)
    ctx.set_round_size(325)  # not a multiple of 10: a round still covers whole samples (330 records)
    try:
        got = _check_run(p1, p2, K, "count")
    finally:
        ctx.set_round_size(4096)
    assert _bits(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[2].best_hyp, got[2].iters, got[2].n_inliers) == (want[2].best_hyp, want[2].iters, want[2].n_inliers)
    assert got[2].rounds > want[2].rounds and got[2].hyps_scored % RPS == 0


def test_five_points_run_the_ordinary_loop():
    p1, p2, K = _pts(5)
    E, mask, F, info = rsac.essential_ransac(p1, p2, K, THR, seed=SEED, confidence=CONF, max_iters=50, return_info=True,
                                             return_F=True)
    best, iters, good, Fr = _replay(p1, p2, K, "count", 50)
    assert best >= 0 and good == 5 and (info.best_hyp, info.iters, info.n_inliers) == (best, iters, good)
    assert _bits(F, Fr) and _np(mask).all()
    # a winner with fewer than 8 inliers keeps the minimal model under refine=True
    E2, mask2, F2 = rsac.essential_ransac(p1, p2, K, THR, seed=SEED, confidence=CONF, max_iters=50, refine=True,
                                          return_F=True)
    assert _bits(F2, F) and _bits(E2, E) and np.array_equal(_np(mask2), _np(mask))


def test_refit_is_the_fit_of_the_winners_mask():
    p1, p2, K = _pts(257, .3, 8)
    E0, mask0, F0 = rsac.essential_ransac(p1, p2, K, THR, seed=SEED, return_F=True)
    E, mask, F = rsac.essential_ransac(p1, p2, K, THR, seed=SEED, refine=True, return_F=True)
    assert np.array_equal(_np(mask), _np(mask0))
    fit = rsac.fundamental_fit(p1, p2, _np(mask))
    assert fit is not None and _bits(F, fit) and not _bits(F, F0)
    assert _bits(E, rsac.essential_from_fundamental(fit, K)) and _bits(E0, rsac.essential_from_fundamental(F0, K))


# ---------------------------------------------------------------------------------------------
# the batched call, the other paths
# ---------------------------------------------------------------------------------------------
def test_batched_equals_single():
    sizes = (5, 64, 257)
    pts = [_pts(n) for n in sizes]
    a, b = [p[0] for p in pts], [p[1] for p in pts]
    Ks = np.stack([p[2] * np.array([[s, 1, 1], [1, s, 1], [1, 1, 1]]) for p, s in zip(pts, (1.0, 1.1, 0.9))])
    K2s = np.stack([_K2(k) for k in Ks])
    for kw in (dict(score="count"), dict(score="msac"), dict(score="count", refine=True)):
        rows = rsac.essential_ransac_batched(a, b, Ks, THR, K2=K2s, seed=SEED, return_F=True, **kw)
        for p, row in enumerate(rows):
            E, mask, F, info = rsac.essential_ransac(a[p], b[p], Ks[p], THR, K2=K2s[p], seed=SEED, max_iters=500,
                                                     return_info=True, return_F=True, **kw)
            tag = (sizes[p], kw)
            assert (E is None) == (row[0] is None), tag
            assert E is None or (_bits(row[0], E) and _bits(row[3], F)), tag
            assert np.array_equal(_np(row[1]), _np(mask)) and row[2] == info.n_inliers, tag
            if kw["score"] == "msac":
                assert row[4] == info.cost, tag  # rsac_last_costs
    one = rsac.essential_ransac_batched(a, b, Ks[1], THR, seed=SEED)  # one K for every problem
    E = rsac.essential_ransac(a[2], b[2], Ks[1], THR, seed=SEED, max_iters=500)[0]
    assert _bits(one[2][0], E)


def test_eight_and_seven_point_probes_are_unchanged():
    p1, p2, _ = _pts(257, .3, 8)
    status, counts, models = rsac.hypotheses("fundamental", p1, p2, hyp_begin=0, n_hyps=64, reproj_thresh=THR, seed=SEED)
    c8, s8, m8 = O.fm_hypotheses(O.soa_hom(p1, p2), THR, SEED, 64, models=True)
    assert np.array_equal(status, s8) and np.array_equal(counts, c8) and _bits(models[:, :9], m8[:, :9])
    status, counts, models = rsac.hypotheses("fundamental", p1, p2, hyp_begin=0, n_hyps=33, reproj_thresh=THR, seed=SEED,
                                             minimal="7pt")
    for s in range(33):
        host = rsac.fundamental_minimal7(*(p[O.philox_subset(SEED, 0, s, 257, 7)] for p in (p1, p2)))
        for r in range(3):
            if r < len(host):
                assert status[3 * s + r] == 1 and _bits(models[3 * s + r, :9], host[r].ravel())
                assert counts[3 * s + r] == rsac.fundamental_cost(p1, p2, host[r], THR)[0]
            else:
                assert status[3 * s + r] == 0 and not models[3 * s + r, :9].any()


def test_other_flags_are_refused():
    import ctypes as C
    p1, p2, K = _pts(64, .3, 2)
    ctx = L.context(0)
    lib = L.lib()
    k9 = np.ascontiguousarray(K.reshape(9))
    E, m = np.zeros(9), np.zeros(64, np.uint8)
    counts, status = np.zeros(80, np.int32), np.zeros(80, np.int8)
    off = np.array([0, 64], np.int64)
    st1, ni1 = np.zeros(1, np.int32), np.zeros(1, np.int32)
    with ctx.lock:
        for flag in (L.F_FM_7POINT, L.F_LO, L.F_EPNP, L.F_SAMPLER_OPENCV, L.F_ASYNC):
            code = lib.rsac_essential_ransac(ctx.handle, p1.ctypes.data, p2.ctypes.data, 64, k9.ctypes.data, None, 100,
                                             THR, CONF, SEED, flag, E.ctypes.data, None, m.ctypes.data, None, None)
            assert code == L.EINVAL, flag
            code = lib.rsac_essential_ransac_batched(ctx.handle, p1.ctypes.data, p2.ctypes.data, off.ctypes.data, 1,
                                                     k9.ctypes.data, None, 100, THR, CONF, SEED, flag, E.ctypes.data, None,
                                                     st1.ctypes.data, ni1.ctypes.data, m.ctypes.data, None)
            assert code == L.EINVAL, flag
            code = lib.rsac_essential_hypotheses(ctx.handle, p1.ctypes.data, p2.ctypes.data, 64, k9.ctypes.data, None, 0,
                                                 8, THR, SEED, flag, counts.ctypes.data, status.ctypes.data, None, None,
                                                 None)
            assert code == L.EINVAL, flag
        # the internal essential bit is no public flag of the fundamental-matrix calls
        F = np.zeros(9)
        code = lib.rsac_fundamental_ransac(ctx.handle, p1.ctypes.data, p2.ctypes.data, 64, 100, THR, CONF, SEED, 1 << 31,
                                           F.ctypes.data, m.ctypes.data, None, None)
        assert code == L.EINVAL
        code = lib.rsac_fundamental_hypotheses(ctx.handle, p1.ctypes.data, p2.ctypes.data, 64, 0, 8, THR, SEED, 1 << 31,
                                               counts.ctypes.data, status.ctypes.data, None, None)
        assert code == L.EINVAL
    with pytest.raises(rsac.RsacError):
        rsac.essential_ransac(p1, p2, np.zeros((3, 3)))  # a singular K


# ---------------------------------------------------------------------------------------------
# end to end: E and the pose
# ---------------------------------------------------------------------------------------------
def _angle(Ra, Rb):
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(Ra.T @ Rb) - 1.0) / 2.0))))


def test_end_to_end_pose():
    pr = R.problem(2000, 0.5, 3, 0.5)
    p1, p2, K, thr = pr["pts1"], pr["pts2"], pr["K"], 1.0
    E0, mask0, F0 = rsac.essential_ransac(p1, p2, K, thr, seed=SEED, return_F=True)
    E, mask, F = rsac.essential_ransac(p1, p2, K, thr, seed=SEED, refine=True, return_F=True)
    mask = _np(mask)
    # the mask is the winner's: the restatement's mask of the same F, so it holds a false inlier
    # exactly where the restatement's does; the expected count is the host scorer's
    count, want = O.fm_count(F0, O.soa_hom(p1, p2), thr, mask=True)
    assert np.array_equal(mask, want) and np.array_equal(mask, _np(mask0))
    assert int(mask.sum()) == count == rsac.fundamental_cost(p1, p2, F0, thr)[0]
    assert _bits(F, rsac.fundamental_fit(p1, p2, mask)) and _bits(E, rsac.essential_from_fundamental(F, K))
    Rg, tg, front = rsac.recover_pose(p1, p2, K, E, mask)
    # the yardstick: the host-side fit on the true inlier set, through the same projection and pose
    Et = rsac.essential_from_fundamental(rsac.fundamental_fit(p1, p2, pr["inlier"]), K)
    Rt, tt, _ = rsac.recover_pose(p1, p2, K, Et, pr["inlier"])
    got, ref = _angle(Rg, pr["R"]), _angle(Rt, pr["R"])
    print(f"em5 end to end: {int(mask.sum())} in the mask ({int((mask & ~pr['inlier']).sum())} false, "
          f"{int(pr['inlier'].sum())} true inliers), {front} in front; rotation error {got:.4f} deg, "
          f"the fit on the true inliers {ref:.4f} deg")
    assert got <= 2.0 * ref
