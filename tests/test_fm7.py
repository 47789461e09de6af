"""The seven-point fundamental matrix without a GPU: the host solver
rsac_fm_minimal7 and its root finder rsac_cubic_real_roots -- the RSAC_HD source k_fm_solve_g7
runs -- against the NumPy reference of tests/fm7ref.py, and the pinned behaviour of the scan in
sample units that the GPU tests replay.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fm7ref as R  # noqa: E402
import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402

F_BOUND = 1e-9     # model against reference, Frobenius norm up to sign (the issue's bound: ~300 x the
                   # 3.3e-12 worst deviation of an independent f64 prototype from the same reference)
DET_BOUND = 1e-15
ULP = 2.0 ** -52


def test_new_symbols_are_exported():
    lib = L.lib()
    table = {row[0] for row in L.SIGNATURES}
    for name in ("rsac_cubic_real_roots", "rsac_fm_minimal7"):
        assert hasattr(lib, name) and name in table, name
    for name in ("fundamental_minimal7", "cubic_real_roots"):
        assert callable(getattr(rsac, name)) and name in rsac.__all__
    assert L.F_FM_7POINT == 1 << 14
    assert lib.rsac_abi_version() == 2


def _unit_norm_error(F):
    return abs(math.sqrt(math.fsum(float(v) * float(v) for v in F.ravel())) - 1.0)


def _match(models, ref):
    """each library model to its nearest reference model up to sign -> (distances, a bijection?)"""
    dist, used = [], []
    for F in models:
        d = [min(np.linalg.norm(F - G), np.linalg.norm(F + G)) for G in ref]
        k = int(np.argmin(d))
        dist.append(d[k])
        used.append(k)
    return dist, len(set(used)) == len(used)


@pytest.mark.parametrize("key", R.INPUTS)
def test_minimal7_equals_reference(key):
    pr = R.problem(*key)
    left_out, one_root, three_roots, worst, worst_det, worst_norm = 0, 0, 0, 0.0, 0.0, 0.0
    for idx in R.subsets(key[0]):
        p1, p2 = pr["pts1"][idx], pr["pts2"][idx]
        models = rsac.fundamental_minimal7(p1, p2)
        ref, roots = R.minimal7(p1, p2)
        # the properties every returned model has, whatever the reference says
        for F in models:
            worst_norm = max(worst_norm, _unit_norm_error(F))
            worst_det = max(worst_det, abs(R.det3(F)))
        lam = R.root_parameters(models, p1, p2)
        assert all(a < b for a, b in zip(lam, lam[1:])), (idx, lam)
        dist, bijection = _match(models, ref) if len(models) == len(ref) else ([], False)
        if not bijection or max(dist, default=0.0) > F_BOUND:
            # only a (near-)double root of the reference's own cubic may excuse a subset
            assert R.near_double_root(roots), (idx, len(models), len(ref), dist)
            left_out += 1
            continue
        worst = max(worst, max(dist, default=0.0))
        one_root += len(models) == 1
        three_roots += len(models) == 3
    print(f"fm7 {key}: worst |F - F_ref| {worst:.3g}, worst |det| {worst_det:.3g}, worst | |F| - 1 | "
          f"{worst_norm / ULP:.2f} ulp, one root {one_root}, three roots {three_roots}, left out {left_out}")
    assert worst_norm <= 4 * ULP
    assert worst_det <= DET_BOUND
    assert left_out <= 0.02 * R.N_SUBSETS
    assert one_root > 0 and three_roots > 0  # both branches of the cubic
    assert one_root + three_roots + left_out == R.N_SUBSETS


def test_degenerate_samples_give_no_model():
    pr = R.problem(64, 0.3, 2)
    idx = R.subsets(64, 1)[0]
    p1, p2 = pr["pts1"][idx].copy(), pr["pts2"][idx].copy()
    p1[3], p2[3] = p1[0], p2[0]  # two identical correspondences: rank 6
    assert rsac.fundamental_minimal7(p1, p2) == []
    # 7 coincident points: no normalisation, nothing written but zeros
    q = np.repeat(pr["pts1"][:1], 7, axis=0)
    F = np.full(27, np.nan)
    n = C.c_int32(-1)
    assert L.lib().rsac_fm_minimal7(q.ctypes.data, q.ctypes.data, F.ctypes.data, C.byref(n)) == L.OK
    assert n.value == 0 and np.array_equal(F, np.zeros(27))
    with pytest.raises(ValueError):
        rsac.fundamental_minimal7(pr["pts1"][:8], pr["pts2"][:8])


@pytest.mark.parametrize("c,want,tol", [
    ((-6.0, 11.0, -6.0, 1.0), (1.0, 2.0, 3.0), 1e-12),   # (x - 1)(x - 2)(x - 3)
    ((-1.0, 0.0, 0.0, 1.0), (1.0,), 1e-15),              # x^3 - 1: one real root
    ((-1.0, 0.0, 1.0, 0.0), (-1.0, 1.0), 0.0),           # x^2 - 1, c3 = 0
    ((-4.0, 2.0, 0.0, 0.0), (2.0,), 0.0),                # 2x - 4, c3 = c2 = 0
    ((0.0, 0.0, 0.0, 0.0), (), 0.0),
    ((5.0, 0.0, 0.0, 0.0), (), 0.0),
    ((0.0, 0.0, 0.0, 1.0), (0.0,), 0.0),                 # x^3: a root at 0
    ((-1.0, 1.0, 0.0, 1e-30), (1.0,), 1e-15),            # wide coefficient ratio
    ((1.0, 0.0, 1.0, 0.0), (), 0.0),                     # x^2 + 1
    ((6.0, 11.0, 6.0, 1.0), (-3.0, -2.0, -1.0), 1e-12),
    ((6.0, -11.0, 6.0, -1.0), (1.0, 2.0, 3.0), 1e-12),   # a negative leading coefficient
])
def test_cubic_real_roots(c, want, tol):
    got = rsac.cubic_real_roots(c)
    assert len(got) == len(want), got
    assert all(a <= b for a, b in zip(got, got[1:]))
    for g, w in zip(got, want):
        assert abs(g - w) <= tol, (got, want)


def test_cubic_real_roots_against_numpy():
    rng = np.random.default_rng(7)
    for _ in range(2000):
        c = rng.normal(size=4) * 10.0 ** rng.integers(-3, 4, 4)
        ref = np.roots(c[::-1])
        if R.near_double_root(ref):
            continue
        real = np.sort(ref[np.abs(ref.imag) < 1e-9 * np.maximum(1.0, np.abs(ref))].real)
        got = rsac.cubic_real_roots(c)
        assert len(got) == len(real), (c, got, ref)
        assert all(a < b for a, b in zip(got, got[1:]))
        np.testing.assert_allclose(got, real, rtol=1e-9, atol=1e-12)


# --- the scan in sample units: the restatement the GPU tests replay, pinned on synthetic rows ---
def _rows(n_samples):
    return np.zeros(3 * n_samples, np.int8), np.zeros(3 * n_samples, np.int32), np.zeros(3 * n_samples, np.int64)


def test_scan_winner_in_the_third_slot():
    st, cnt, cost = _rows(700)
    st[:3], cnt[:3], cost[:3] = 1, (7, 20, 50), (900, 500, 100)
    st[30:33], cnt[30:33], cost[30:33] = 1, (50, 49, 6), (100, 90, 1)  # a tie keeps the earlier; 6 is not eligible
    # RANSACUpdateNumIters(0.99, 0.5, 7, .) = 587 samples
    assert rsac.update_num_iters(0.99, 0.5, 7, 1000) == 587
    assert R.scan_count(st, cnt, 100, 0.99, 1000) == (2, 587, 50)
    # MSAC: the lower cost wins whatever its count (record 31), and the bound follows its count
    assert R.scan_msac(st, cnt, cost, 100, 0.99, 1000) == (31, rsac.update_num_iters(0.99, 0.51, 7, 587), 49)


def test_scan_consumes_the_whole_sample_when_the_bound_falls_inside_it():
    st, cnt, cost = _rows(40)
    # sample 12 = records 36 .. 38: record 36 brings the bound to 2 samples, below the sample the
    # scan is in; records 37 and 38 are still looked at, and the scan ends where sample 13 would begin
    st[36:39], cnt[36:39], cost[36:39] = 1, (99, 100, 98), (50, 40, 30)
    assert rsac.update_num_iters(0.99, 0.01, 7, 1000) == 2
    assert R.scan_count(st, cnt, 100, 0.99, 1000) == (37, 13, 100)
    assert R.scan_msac(st, cnt, cost, 100, 0.99, 1000) == (38, 13, 98)
    # a bound that ends the scan between samples: 13 samples consumed, none of sample 13's records
    st[39:42], cnt[39:42] = 1, 100
    cnt[37] = 99
    assert R.scan_count(st, cnt, 100, 0.99, 1000) == (36, 13, 99)


def test_scan_ends_at_a_failed_draw():
    st, cnt, cost = _rows(10)
    st[3:6], cnt[3:6], cost[3:6] = 1, (8, 9, 10), (3, 2, 1)
    st[6:9] = -1
    st[9:12], cnt[9:12] = 1, 90
    assert R.scan_count(st, cnt, 100, 0.99, 1000) == (5, 2, 10)
    assert R.scan_msac(st, cnt, cost, 100, 0.99, 1000) == (5, 2, 10)
    med = np.where(st > 0, 5.0, -1.0)
    med[4] = 2.0
    assert R.scan_lmeds(st, med, 10) == (4, 2.0)
    assert R.scan_lmeds(st, med, 1) == (-1, np.finfo(np.float64).max)


def test_scan_budget_is_in_samples():
    st, cnt, _ = _rows(10)
    st[:], cnt[:] = 1, 7
    cnt[15] = 60
    assert R.scan_count(st, cnt, 100, 0.99, 5) == (0, 5, 7)       # 5 samples = records 0 .. 14
    assert R.scan_count(st, cnt, 100, 0.99, 6)[0] == 15
