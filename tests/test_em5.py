"""The five-point essential matrix without a GPU: the host solver rsac_em_minimal5 and
its root finder rsac_poly_real_roots -- the RSAC_HD source k_em_solve_g5 runs -- against the NumPy
reference of tests/em5ref.py, the pose functions, and the pinned behaviour of the scan in sample
units that the GPU tests replay.

Bounds of test_minimal5_equals_reference, per input: the model bound is 100 x the largest deviation
of the reference's own unpolished eigenvector solution from its polished one over the test's samples,
the median bound 100 x the median of that deviation (the issue's rule).  Measured with these inputs
(300 subsets each; library against the polished reference | reference unpolished against polished):
  (64, 0, 2, 0)      median 4.8e-15, max 5.5e-13 | median 1.2e-13, max 7.9e-8  -> bounds 1.2e-11, 7.9e-6
  (256, 0, 8, 0)     median 6.6e-15, max 2.4e-12 | median 2.1e-13, max 2.7e-4  -> bounds 2.1e-11, 2.7e-2
  (200, .3, 3, .5)   median 1.9e-15, max 2.0e-13 | median 5.1e-15, max 4.5e-9  -> bounds 5.1e-13, 4.5e-7
  (500, .5, 4, .5)   median 1.3e-15, max 1.7e-13 | median 3.0e-15, max 9.0e-10 -> bounds 3.0e-13, 9.0e-8
No sample is left out on any of the four.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import em5ref as R  # noqa: E402
import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402

ULP = 2.0 ** -52
SQ = math.sqrt(0.5)


def test_new_symbols_are_exported():
    lib = L.lib()
    table = {row[0] for row in L.SIGNATURES}
    for name in ("rsac_essential_ransac", "rsac_essential_ransac_batched", "rsac_essential_hypotheses",
                 "rsac_poly_real_roots", "rsac_em_minimal5", "rsac_essential_from_fundamental",
                 "rsac_essential_recover_pose"):
        assert hasattr(lib, name) and name in table, name
    for name in ("essential_ransac", "essential_ransac_batched", "essential_minimal5", "poly_real_roots",
                 "essential_from_fundamental", "recover_pose"):
        assert callable(getattr(rsac, name)) and name in rsac.__all__
    assert callable(rsac.synth.essential_problem)
    assert lib.rsac_abi_version() == 2


# ---------------------------------------------------------------------------------------------
# the root finder
# ---------------------------------------------------------------------------------------------
def _coefficients(real, pairs=()):
    """lowest power first, from real roots and complex pairs (re, im)"""
    c = np.poly(list(real) + [complex(a, b) for a, b in pairs] + [complex(a, -b) for a, b in pairs]).real
    return c[::-1]


@pytest.mark.parametrize("degree", range(1, 11))
def test_poly_real_roots_all_real(degree):
    rng = np.random.default_rng(degree)
    for _ in range(20):
        want = np.sort(rng.choice(np.arange(-12, 13), degree, replace=False) * 0.25 + rng.uniform(-0.05, 0.05, degree))
        c = _coefficients(want) * rng.uniform(0.5, 2.0) * rng.choice([-1.0, 1.0])
        got = rsac.poly_real_roots(c)
        ref = np.sort(np.roots(c[::-1]).real)
        assert len(got) == degree and all(a < b for a, b in zip(got, got[1:])), (want, got)
        # np.roots itself is good to ~1e-9 on ten roots a quarter apart; both are checked against the
        # roots the polynomial was built from, the library no worse than 10 x numpy's own error
        err, err_np = np.abs(got - want).max(), np.abs(ref - want).max()
        assert err <= max(10.0 * err_np, 1e-12), (degree, err, err_np)


def test_poly_real_roots_some_and_none_real():
    rng = np.random.default_rng(11)
    for n_real in range(0, 9, 2):
        for _ in range(20):
            want = np.sort(rng.choice(np.arange(-8, 9), n_real, replace=False) * 0.5)
            pairs = [(rng.uniform(-2, 2), rng.uniform(0.5, 2)) for _ in range((10 - n_real) // 2)]
            c = _coefficients(want, pairs)
            got = rsac.poly_real_roots(c)
            ref = np.roots(c[::-1])
            real = np.sort(ref[np.abs(ref.imag) < 1e-6].real)
            assert len(got) == n_real == len(real), (want, pairs, got)
            assert all(a < b for a, b in zip(got, got[1:]))
            if n_real:
                assert np.abs(got - want).max() <= max(10.0 * np.abs(real - want).max(), 1e-12)


@pytest.mark.parametrize("c,want", [
    ((-6.0, 11.0, -6.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (1.0, 2.0, 3.0)),  # zero leading coefficients
    ((-6.0, 11.0, -6.0, 1.0), (1.0, 2.0, 3.0)),
    ((-4.0, 2.0, 0.0, 0.0, 0.0), (2.0,)),
    ((-1.0, 0.0, 1.0) + (0.0,) * 7 + (1e-320,), (-1.0, 1.0)),  # a leading coefficient whose bound overflows
    ((0.0,) * 11, ()),
    ((5.0,) + (0.0,) * 10, ()),
    ((5.0,), ()),
    ((1.0, 0.0, 1.0), ()),
    ((0.0,) * 9 + (1.0,), (0.0,)),   # x^9: a root of odd multiplicity at 0
    ((0.0,) * 10 + (1.0,), ()),      # x^10: even multiplicity, not reported (include/rsac.h)
    ((float("nan"),) * 11, ()),
])
def test_poly_real_roots_lowers_the_degree(c, want):
    got = rsac.poly_real_roots(c)
    assert len(got) == len(want), got
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-14, (got, want)


# ---------------------------------------------------------------------------------------------
# the solver against the reference
# ---------------------------------------------------------------------------------------------
def _unit_norm_error(F):
    return abs(math.sqrt(math.fsum(float(v) * float(v) for v in F.ravel())) - 1.0)


@pytest.mark.parametrize("key", R.INPUTS)
def test_minimal5_equals_reference(key):
    pr = R.problem(*key)
    K = pr["K"]
    Ki = np.linalg.inv(K)
    left_out, branches, dev, spread, worst_norm, worst_prop = 0, {}, [], [], 0.0, 0.0
    for idx in R.subsets(key[0]):
        p1, p2 = pr["pts1"][idx], pr["pts2"][idx]
        Fs, Es = rsac.essential_minimal5(p1, p2, K, return_E=True)
        pol, raw, w = R.minimal5(p1, p2, K)
        for F, E in zip(Fs, Es):  # the properties every returned model has, whatever the reference says
            worst_norm = max(worst_norm, _unit_norm_error(F), _unit_norm_error(E))
            G = Ki.T @ E @ Ki
            worst_prop = max(worst_prop, R.model_distance(F, G / np.linalg.norm(G)))
        if R.ambiguous(w):  # only the reference's own eigenvalues may excuse a subset
            left_out += 1
            continue
        dist = R.match(Es, pol)
        assert dist is not None, (idx, len(Es), len(pol))
        dev += dist
        spread += [R.model_distance(a, b) for a, b in zip(pol, raw)]
        branches[len(Es)] = branches.get(len(Es), 0) + 1
    dev, spread = np.array(dev), np.array(spread)
    print(f"em5 {key}: library against the polished reference: median {np.median(dev):.3g}, max {dev.max():.3g}; "
          f"reference unpolished against polished: median {np.median(spread):.3g}, max {spread.max():.3g}; "
          f"| |F| - 1 | {worst_norm / ULP:.2f} ulp, |F - K^-T E K^-1| {worst_prop:.3g}, models per sample {branches}, "
          f"left out {left_out}")
    assert left_out <= 0.02 * R.N_SUBSETS
    assert dev.max() <= 100.0 * spread.max()
    assert np.median(dev) <= 100.0 * np.median(spread)
    assert worst_norm <= 4 * ULP
    assert worst_prop <= 1e-12
    assert all(branches.get(k, 0) > 0 for k in (2, 4, 6))


def test_degenerate_samples_give_no_model():
    pr = R.problem(64, 0.0, 2, 0.0)
    K = pr["K"]
    idx = R.subsets(64, 1)[0]
    p1, p2 = pr["pts1"][idx].copy(), pr["pts2"][idx].copy()
    assert len(rsac.essential_minimal5(p1, p2, K)) > 0

    def raw(a, b):
        F, E = np.full(90, np.nan), np.full(90, np.nan)
        n = C.c_int32(-1)
        k9 = np.ascontiguousarray(K.reshape(9))
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert L.lib().rsac_em_minimal5(a.ctypes.data, b.ctypes.data, k9.ctypes.data, None, F.ctypes.data,
                                        E.ctypes.data, C.byref(n)) == L.OK
        return n.value, F, E

    q1, q2 = p1.copy(), p2.copy()
    q1[3], q2[3] = q1[0], q2[0]  # a repeated correspondence: rank 4
    line = np.c_[np.arange(5) * 37.0 + 100.0, np.arange(5) * 11.0 + 50.0]  # five collinear pixels in both views
    nan1 = p1.copy()
    nan1[2, 0] = np.nan
    for a, b in ((q1, q2), (line, line), (nan1, p2), (p1, nan1)):
        n, F, E = raw(a, b)
        assert n == 0 and np.array_equal(F, np.zeros(90)) and np.array_equal(E, np.zeros(90))
        assert rsac.essential_minimal5(a, b, K) == []
    with pytest.raises(ValueError):
        rsac.essential_minimal5(pr["pts1"][:6], pr["pts2"][:6], K)
    with pytest.raises(rsac.RsacError) as e:
        rsac.essential_minimal5(p1, p2, np.zeros((3, 3)))
    assert e.value.code == L.EINVAL


# ---------------------------------------------------------------------------------------------
# pose
# ---------------------------------------------------------------------------------------------
def _sign_rule(E):
    k = int(np.argmax(np.abs(E.ravel())))  # the first maximum in row-major order
    return E.ravel()[k] > 0


def test_essential_from_fundamental():
    pr = R.problem(500, 0.5, 4, 0.5)
    K, F, E_true = pr["K"], pr["F"], pr["E"]
    K2 = K * np.array([[1.1, 1, 0.9], [1, 1.05, 1.02], [1, 1, 1]])
    E = rsac.essential_from_fundamental(F, K)
    assert np.abs(np.linalg.svd(E, compute_uv=False) - [SQ, SQ, 0.0]).max() <= 1e-14 and _sign_rule(E)
    assert np.abs(rsac.essential_from_fundamental(np.linalg.inv(K).T @ E @ np.linalg.inv(K), K) - E).max() <= 1e-14
    # a true E is returned as it is, up to the sign rule
    want = E_true if _sign_rule(E_true) else -E_true
    assert np.abs(E - want).max() <= 1e-12
    # a general F (rank 3) and two different views
    rng = np.random.default_rng(5)
    G = rng.normal(size=(3, 3))
    E2 = rsac.essential_from_fundamental(G, K, K2)
    assert np.abs(np.linalg.svd(E2, compute_uv=False) - [SQ, SQ, 0.0]).max() <= 1e-14 and _sign_rule(E2)
    U, s, Vt = np.linalg.svd(K2.T @ G @ K)
    P = U @ np.diag([SQ, SQ, 0.0]) @ Vt
    assert R.model_distance(E2, P) <= 1e-12 * s[0] / (s[1] - s[2])
    assert rsac.essential_from_fundamental(np.zeros((3, 3)), K) is None


def test_recover_pose_returns_the_scene_pose():
    pr = R.problem(500, 0.5, 4, 0.5)
    K, Rt, t, E = pr["K"], pr["R"], pr["t"], pr["E"]
    for sign in (1.0, -1.0):
        Rg, tg, front, counts = rsac.recover_pose(pr["pts1"], pr["pts2"], K, sign * E, pr["inlier"], return_counts=True)
        assert np.abs(Rg - Rt).max() <= 1e-9 and np.abs(tg - t / np.linalg.norm(t)).max() <= 1e-9
        assert abs(np.linalg.det(Rg) - 1.0) <= 1e-14 and abs(np.linalg.norm(tg) - 1.0) <= 1e-14
        assert front == counts.max() == int(pr["inlier"].sum())
        assert sorted(counts)[-2] < front  # each of the other three has fewer points in front
    # all points: the outliers vote too, the inliers still decide
    assert np.abs(rsac.recover_pose(pr["pts1"], pr["pts2"], K, E)[0] - Rt).max() <= 1e-9
    assert rsac.recover_pose(pr["pts1"], pr["pts2"], K, E, np.zeros(500, bool)) == (None, None, 0)


# ---------------------------------------------------------------------------------------------
# the scan in sample units: the restatement the GPU tests replay, pinned on synthetic rows
# ---------------------------------------------------------------------------------------------
def _rows(n_samples):
    return np.zeros(10 * n_samples, np.int8), np.zeros(10 * n_samples, np.int32), np.zeros(10 * n_samples, np.int64)


def test_scan_winner_in_a_late_slot():
    st, cnt, cost = _rows(300)
    st[:4], cnt[:4], cost[:4] = 1, (5, 20, 50, 4), (900, 500, 100, 1)  # 4 inliers are not eligible
    st[30:33], cnt[30:33], cost[30:33] = 1, (50, 49, 4), (100, 90, 1)  # a tie keeps the earlier
    assert rsac.update_num_iters(0.99, 0.5, 5, 1000) == 145
    assert R.scan_count(st, cnt, 100, 0.99, 1000) == (2, 145, 50)
    assert R.scan_msac(st, cnt, cost, 100, 0.99, 1000) == (31, rsac.update_num_iters(0.99, 0.51, 5, 145), 49)


def test_scan_consumes_the_whole_sample_when_the_bound_falls_inside_it():
    st, cnt, cost = _rows(40)
    # sample 12 = records 120 .. 129: record 121 brings the bound to 2 samples, below the sample the
    # scan is in; the rest of the sample is still looked at, and the scan ends where sample 13 would begin
    st[121:124], cnt[121:124], cost[121:124] = 1, (99, 100, 98), (50, 40, 30)
    assert rsac.update_num_iters(0.99, 0.01, 5, 1000) == 2
    assert R.scan_count(st, cnt, 100, 0.99, 1000) == (122, 13, 100)
    assert R.scan_msac(st, cnt, cost, 100, 0.99, 1000) == (123, 13, 98)
    st[130:133], cnt[130:133] = 1, 100
    cnt[122] = 99
    assert R.scan_count(st, cnt, 100, 0.99, 1000) == (121, 13, 99)


def test_scan_ends_at_a_failed_draw_and_budget_is_in_samples():
    st, cnt, cost = _rows(10)
    st[10:13], cnt[10:13], cost[10:13] = 1, (8, 9, 10), (3, 2, 1)
    st[20:30] = -1
    st[30:40], cnt[30:40] = 1, 90
    assert R.scan_count(st, cnt, 100, 0.99, 1000) == (12, 2, 10)
    assert R.scan_msac(st, cnt, cost, 100, 0.99, 1000) == (12, 2, 10)
    st, cnt, _ = _rows(10)
    st[:], cnt[:] = 1, 5
    cnt[50] = 60
    assert R.scan_count(st, cnt, 100, 0.99, 5) == (0, 5, 5)  # 5 samples = records 0 .. 49
    assert R.scan_count(st, cnt, 100, 0.99, 6)[0] == 50
