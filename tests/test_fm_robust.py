"""MSAC and LMedS for the fundamental matrix without a GPU: the host pieces (rsac_fm_err_host,
rsac_fm_cost_host, rsac_fm_median_host -- the RSAC_HD source the k_fm_cost* / k_fm_median* kernels
run -- and the two scans with 8 model points) against tests/fmrobustref.py, the pinned tables, and
the argument checks that must fire before any device work.  Every comparison is exact equality.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fmrobustref as R  # noqa: E402
import lmedsref as LM  # noqa: E402
import msacref as MS  # noqa: E402
import pyoracle as O  # noqa: E402
import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402

THR = R.THR
NEW_C = ("rsac_fundamental_hypotheses_msac", "rsac_fundamental_lmeds", "rsac_fundamental_medians", "rsac_fm_err_host",
         "rsac_fm_cost_host", "rsac_fm_median_host")
NEW_PY = ("fundamental_lmeds", "fundamental_costs", "fundamental_errors", "fundamental_cost", "fm_median")


def _same_f32(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_new_symbols_are_exported():
    lib = L.lib()
    table = {row[0] for row in L.SIGNATURES}
    for name in NEW_C:
        assert hasattr(lib, name) and name in table, name
    for name in NEW_PY:
        assert callable(getattr(rsac, name)) and name in rsac.__all__
    assert lib.rsac_abi_version() == 2


def _check_host_equals_reference(key):
    pr = R.problem(*key)
    H = 8 if key == R.BIG else 64
    status, cnt, cost, med, models = R.hypotheses_case(*key, H)
    soa = O.soa_hom(pr["pts1"], pr["pts2"])
    assert (status > 0).any()
    for h in np.flatnonzero(status > 0):
        F = models[h, :9]
        assert _same_f32(rsac.fundamental_errors(pr["pts1"], pr["pts2"], F), R.fm_err(F, soa)), h
        assert rsac.fundamental_cost(pr["pts1"], pr["pts2"], F, THR) == (int(cnt[h]), int(cost[h])), h
        assert rsac.fm_median(pr["pts1"], pr["pts2"], F) == med[h], h
    return cnt, cost


@pytest.mark.parametrize("key", R.INPUTS)
def test_host_functions_equal_reference(key):
    _check_host_equals_reference(key)


def test_host_cost_64_bit_sum():
    cnt, cost = _check_host_equals_reference(R.BIG)
    assert cost.max() > 2**32  # more than 8192 outliers at Q >= 2^19


def test_error_edge_cases():
    """F = e3 e3^T: a = b = a' = b' = 0, c = r = 1: den == 0 < r^2, the error is +inf, an outlier.
    F = 0: r = den = 0: error 0, an inlier (0 <= T 0), as the count rule has it.
    F of a pure x translation: epipolar lines y2 = y1, den = 2."""
    k = MS.shift(THR)
    Q = int(MS.q(np.array([np.float32(O.thr2(THR))]), k)[0])
    p1 = np.array([[3.0, 5.0], [1.0, 2.0], [float("nan"), 1.0], [4.0, 4.0], [0.0, 1.0]])
    p2 = np.array([[7.0, 5.0], [9.0, 3.0], [2.0, 2.0], [4.0, 4.5], [8.0, 1.0]])
    n = len(p1)
    soa = O.soa_hom(p1, p2)
    Ft = np.array([0.0, 0, 0, 0, 0, -1, 0, 1, 0])
    e = rsac.fundamental_errors(p1, p2, Ft)
    assert _same_f32(e, R.fm_err(Ft, soa))
    assert e[0] == 0 and e[1] == 0.5 and np.isnan(e[2]) and e[3] == 0.125 and e[4] == 0
    ref_e, ref_inl = R.err_inliers(Ft, soa, O.thr2(THR))
    assert list(ref_inl) == [True, True, False, True, True]
    pc = R.point_costs(ref_e, ref_inl, THR)
    assert pc[2] == Q and pc[0] == 0 and 0 < pc[1] < Q
    assert rsac.fundamental_cost(p1, p2, Ft, THR) == (4, int(pc.sum()))
    assert rsac.fm_median(p1, p2, Ft) == LM.median_of_errors(ref_e) == 0.125  # keys 0, 0, .125, .5, NaN
    q1, q2 = np.delete(p1, 2, 0), np.delete(p2, 2, 0)  # without the NaN
    Finf = np.array([0.0, 0, 0, 0, 0, 0, 0, 0, 1])
    e = rsac.fundamental_errors(q1, q2, Finf)
    assert np.isposinf(e).all() and _same_f32(e, R.fm_err(Finf, O.soa_hom(q1, q2)))
    assert rsac.fundamental_cost(q1, q2, Finf, THR) == (0, (n - 1) * Q)
    assert rsac.fm_median(q1, q2, Finf) == float("inf")
    F0 = np.zeros(9)
    e = rsac.fundamental_errors(q1, q2, F0)
    assert (e == 0).all() and _same_f32(e, R.fm_err(F0, O.soa_hom(q1, q2)))
    assert rsac.fundamental_cost(q1, q2, F0, THR) == (n - 1, 0)
    assert rsac.fundamental_cost(p1, p2, F0, THR) == (n - 1, Q)  # the NaN point: r^2 is NaN, an outlier
    assert rsac.fm_median(q1, q2, F0) == 0.0


def _scan_msac(counts, costs, status, n, chunks=None):
    st = L.ScanMsacState()
    L.lib().rsac_scan_msac_init(C.byref(st), R.MAX_ITERS)
    counts = np.ascontiguousarray(counts, np.int32)
    costs = np.ascontiguousarray(costs, np.int64)
    status = np.ascontiguousarray(status, np.int8)
    pos = 0
    for ln in (chunks or [len(status)]):
        a, b, c = counts[pos:pos + ln], costs[pos:pos + ln], status[pos:pos + ln]
        assert L.lib().rsac_scan_msac(C.byref(st), a.ctypes.data, b.ctypes.data, c.ctypes.data, ln, n, 8, R.CONF) == 0
        pos += ln
    return st.best, st.best_cost, st.max_good, st.iter


@pytest.mark.parametrize("row", range(len(R.MSAC_TABLE)))
def test_msac_chain_and_scan_equal_table(row):
    key, want = R.MSAC_TABLE[row]
    r = R.msac_case(*key)
    assert (r["best"], r["cost"], r["n_inliers"], r["iters"], r["count_best"]) == want
    pr = R.problem(*key)
    ref = O.fm_ransac(pr["pts1"], pr["pts2"], THR, R.CONF, R.MAX_ITERS, R.SEED)
    assert (ref["best"], ref["n_inliers"], ref["iters"]) == (r["count_best"], r["count_good"], r["count_iters"])
    cnt, cost, status = r["rows"]
    assert _scan_msac(cnt, cost, status, key[0]) == want[:4]
    assert _scan_msac(cnt, cost, status, key[0], chunks=[100, len(status) - 100]) == want[:4]


def test_msac_and_count_rule_differ_on_the_pinned_input():
    r = R.msac_case(256, .3, 8)
    assert (r["count_best"], r["count_good"], r["count_iters"]) == (88, 155, 253)
    assert (r["best"], r["n_inliers"], r["cost"], r["iters"]) == (179, 152, 75610670, 253)


def test_lmeds_num_iters():
    assert L.lib().rsac_lmeds_num_iters(0.99, 8, 2000) == 548 == R.num_iters()
    assert rsac.lmeds_num_iters(0.99, 2000, 8) == 548


@pytest.mark.parametrize("row", range(len(R.LMEDS_TABLE)))
def test_lmeds_chain_and_scan_equal_table(row):
    key, want = R.LMEDS_TABLE[row]
    n = key[0]
    r = R.lmeds_case(*key)
    assert (r["best"], r["median"], r["n_inliers"]) == want and r["iters"] == 548
    for chunks in ([548], [100, 448]):
        sc, pos = rsac.LmedsScan(548), 0
        for ln in chunks:
            sc.step(r["status"][pos:pos + ln], r["medians"][pos:pos + ln])
            pos += ln
        assert (sc.best, sc.best_median, sc.iter, sc.done) == (want[0], want[1], 548, True)
    assert rsac.lmeds_sigma(want[1], n, 8) == R.sigma(want[1], n)
    if key in R.LMEDS_INPUTS:  # the estimator must be worth comparing with: >= 95 % of the true inliers kept
        true = R.problem(*key)["inlier"]
        assert int((r["mask"] & true).sum()) >= 0.95 * int(true.sum())


def test_python_argument_checks_fire_before_device_work():
    pr = R.problem(12, .25, 5)
    a, b = pr["pts1"], pr["pts2"]
    with pytest.raises(ValueError, match="score"):
        rsac.fundamental_ransac(a, b, THR, score="bogus")
    with pytest.raises(ValueError, match="score"):
        rsac.fundamental_ransac(a, b, THR, score=None)
    with pytest.raises(ValueError, match="length"):
        rsac.fundamental_lmeds(a, b[:5])
    with pytest.raises(ValueError, match="n_iters"):
        rsac.fundamental_lmeds(a, b, n_iters=0)
    with pytest.raises(ValueError, match="length"):
        rsac.fundamental_costs(a, b[:5])
    with pytest.raises(NotImplementedError, match="medians"):
        rsac.hypotheses("pnp", np.zeros((12, 3)), a, np.eye(3), medians=True)
    with pytest.raises(ValueError, match="Philox"):
        rsac.hypotheses("fundamental", a, b, n_hyps=2, subsets=np.zeros((2, 4), np.int32), medians=True)
    with pytest.raises(NotImplementedError, match="costs"):
        rsac.hypotheses("fundamental", a, b, costs=True)
    for f in (rsac.fundamental_errors, rsac.fm_median):
        with pytest.raises(ValueError, match="length"):
            f(a, b[:5], np.eye(3))
    with pytest.raises(ValueError, match="length"):
        rsac.fundamental_cost(a, b[:5], np.eye(3), THR)


def test_host_entry_points_reject_bad_arguments():
    cnt, cost, med = C.c_int32(0), C.c_int64(0), C.c_double(0)
    F = np.zeros(9)
    s, d = np.zeros((4, 2)), np.zeros((4, 2))
    e = np.ones(4, np.float32)
    lib = L.lib()
    for thr in (0.0, float("nan"), float("inf"), 1e30, 1e-30):  # thr2 = 0, NaN or inf as a float
        assert lib.rsac_fm_cost_host(s.ctypes.data, d.ctypes.data, 4, F.ctypes.data, thr, C.byref(cnt),
                                     C.byref(cost)) == L.EINVAL, thr
        assert b"threshold" in lib.rsac_last_error()
    assert lib.rsac_fm_cost_host(None, None, 4, F.ctypes.data, THR, C.byref(cnt), C.byref(cost)) == L.EINVAL
    assert lib.rsac_fm_cost_host(s.ctypes.data, d.ctypes.data, 4, F.ctypes.data, THR, C.byref(cnt), None) == L.EINVAL
    assert lib.rsac_fm_cost_host(s.ctypes.data, d.ctypes.data, 4, None, THR, C.byref(cnt), C.byref(cost)) == L.EINVAL
    assert lib.rsac_fm_cost_host(s.ctypes.data, d.ctypes.data, 4, F.ctypes.data, THR, C.byref(cnt),
                                 C.byref(cost)) == L.OK
    assert (cnt.value, cost.value) == (4, 0)
    assert lib.rsac_fm_cost_host(None, None, 0, F.ctypes.data, THR, C.byref(cnt), C.byref(cost)) == L.OK
    assert (cnt.value, cost.value) == (0, 0)
    assert lib.rsac_fm_err_host(s.ctypes.data, d.ctypes.data, 4, F.ctypes.data, None) == L.EINVAL
    assert lib.rsac_fm_err_host(s.ctypes.data, d.ctypes.data, -1, F.ctypes.data, e.ctypes.data) == L.EINVAL
    assert lib.rsac_fm_err_host(s.ctypes.data, d.ctypes.data, 4, F.ctypes.data, e.ctypes.data) == L.OK and (e == 0).all()
    assert lib.rsac_fm_median_host(s.ctypes.data, d.ctypes.data, 0, F.ctypes.data, C.byref(med)) == L.EINVAL
    assert lib.rsac_fm_median_host(s.ctypes.data, d.ctypes.data, 4, F.ctypes.data, None) == L.EINVAL
    assert lib.rsac_fm_median_host(s.ctypes.data, d.ctypes.data, 4, F.ctypes.data, C.byref(med)) == L.OK
    assert med.value == 0.0
