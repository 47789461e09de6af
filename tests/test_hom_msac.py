"""MSAC scoring for homographies without a GPU: the host pieces (rsac_hom_cost_host -- the RSAC_HD
source k_hom_cost / k_hom_cost_lane run -- and rsac_scan_msac with model_points = 4, the scan
run_loop calls) against the composition of tests/hmsacref.py, the pinned table, and the Python
interface's argument checks.  Every comparison is exact equality.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hmsacref as M  # noqa: E402
import lmedsref as LM  # noqa: E402
import msacref as MS  # noqa: E402
import pyoracle as O  # noqa: E402
import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402

THR = M.THR
ROWS = range(len(M.TABLE))


def _scan(counts, costs, status, n, conf, max_iters, chunks=None):
    st = L.ScanMsacState()
    L.lib().rsac_scan_msac_init(C.byref(st), int(max_iters))
    counts = np.ascontiguousarray(counts, np.int32)
    costs = np.ascontiguousarray(costs, np.int64)
    status = np.ascontiguousarray(status, np.int8)
    pos = 0
    for ln in (chunks or [len(status)]):
        a, b, c = counts[pos:pos + ln], costs[pos:pos + ln], status[pos:pos + ln]
        assert L.lib().rsac_scan_msac(C.byref(st), a.ctypes.data, b.ctypes.data, c.ctypes.data, ln, n, 4, conf) == 0
        pos += ln
    return st.best, st.best_cost, st.max_good, st.iter


def test_new_symbols_are_exported():
    lib = L.lib()
    assert hasattr(lib, "rsac_homography_hypotheses_msac") and hasattr(lib, "rsac_hom_cost_host")
    for name in ("homography_costs", "homography_cost"):
        assert callable(getattr(rsac, name)) and name in rsac.__all__


@pytest.mark.parametrize("row", ROWS)
def test_hom_cost_host_equals_reference(row):
    (sampler, key), _ = M.TABLE[row]
    pr = M.problem(*key)
    status, cnt, cost, models = M.hypotheses_case(*key, 64, sampler)
    assert (status > 0).any()
    for h in np.flatnonzero(status > 0):
        assert rsac.homography_cost(pr["src"], pr["dst"], models[h, :9], THR) == (int(cnt[h]), int(cost[h])), h


def test_hom_cost_host_64_bit_sum():
    pr = M.problem(*M.BIG)
    status, cnt, cost, models = M.hypotheses_case(*M.BIG, 64, "philox")
    h = int(np.argmax(cost))
    assert cost[h] > 2**32 and cnt[h] < 8  # a near-all-outlier model: more than 8192 points at Q = 2^19
    for h in np.flatnonzero(status > 0):
        assert rsac.homography_cost(pr["src"], pr["dst"], models[h, :9], THR) == (int(cnt[h]), int(cost[h])), h


def test_hom_cost_zero_denominator_costs_Q():
    """h6 x + h7 y + 1 == 0: the error is +inf (a finite numerator) or NaN (0 * inf); neither passes
    e <= thr2, so the point costs Q."""
    k = MS.shift(THR)
    Q = int(MS.q(np.array([np.float32(O.thr2(THR))]), k)[0])
    assert (k, Q) == (13, 524288)
    H = np.array([1.0, 0, 0, 0, 1, 0, 1, 0, 1])  # denominator x + 1
    src = np.array([[0.0, 0.0], [1.0, 2.0], [-1.0, 3.0], [-1.0, 0.0], [0.5, 0.25]])
    dst = np.array([[0.0, 0.0], [0.5, 1.0], [7.0, 7.0], [0.0, 0.0], [0.5, 1.0 / 6.0 + 0.5]])
    soa = O.soa_hom(src, dst)
    e = LM.hom_err(H, soa)
    assert e[0] == 0 and e[1] == 0 and np.isinf(e[2]) and np.isnan(e[3])  # point 3: ex = -1 * inf, ey = 0 * inf
    inl, pc = MS.point_costs(e, THR)
    assert list(inl) == [True, True, False, False, True] and pc[2] == pc[3] == Q and 0 < pc[4] < Q
    assert rsac.homography_cost(src, dst, H, THR) == (3, int(pc.sum()))


@pytest.mark.parametrize("row", ROWS)
def test_scan_msac_with_four_model_points_equals_table(row):
    (sampler, key), want = M.TABLE[row]
    n = key[0]
    status, cnt, c, _ = M.hypotheses_case(*key, 256, sampler)
    ref = MS.scan(c, cnt, status, n, 4, M.CONF, M.MAX_ITERS)
    assert ref == want
    assert _scan(cnt, c, status, n, M.CONF, M.MAX_ITERS) == ref
    assert _scan(cnt, c, status, n, M.CONF, M.MAX_ITERS, chunks=[100, 156]) == ref


@pytest.mark.parametrize("row", ROWS)
def test_chain_equals_table_and_count_rule_differs_where_pinned(row):
    (sampler, key), want = M.TABLE[row]
    r = M.ransac_case(sampler, *key)
    assert (r["best"], r["cost"], r["n_inliers"], r["iters"]) == want
    pr = M.problem(*key)
    ref = O.hom_ransac(pr["src"], pr["dst"], THR, M.CONF, M.MAX_ITERS, M.SEED, sampler=sampler, refine=False)
    assert ref["best"] == r["count_best"] == M.COUNT_BEST.get(row, want[0])


def test_python_argument_checks():
    pr = M.problem(12, .25, 5)
    s, d = pr["src"], pr["dst"]
    with pytest.raises(ValueError, match="score"):
        rsac.homography_ransac(s, d, THR, score="bogus")
    with pytest.raises(ValueError, match="score"):
        rsac.homography_ransac_batched([s], [d], THR, score="bogus")
    with pytest.raises(ValueError, match="score"):
        rsac.location_search(np.zeros((5, 3)), np.ones((5, 2)), np.zeros((2, 3)), score="bogus")
    with pytest.raises(ValueError, match="score"):
        rsac.location_search(np.zeros((5, 3)), np.ones((5, 2)), np.zeros((2, 3)), 75.0, score=None)
    with pytest.raises(NotImplementedError, match="costs"):
        rsac.hypotheses("homography", s, d, costs=True)
    with pytest.raises(ValueError, match="length"):
        rsac.homography_cost(s, d[:5], np.eye(3), THR)


def test_host_entry_point_rejects_bad_arguments():
    cnt, cost = C.c_int32(0), C.c_int64(0)
    H = np.eye(3).reshape(9)
    s, d = np.zeros((4, 2)), np.zeros((4, 2))
    lib = L.lib()
    for thr in (0.0, float("nan"), float("inf"), 1e30, 1e-30):  # thr2 = 0, NaN or inf as a float
        assert lib.rsac_hom_cost_host(s.ctypes.data, d.ctypes.data, 4, H.ctypes.data, thr, C.byref(cnt),
                                      C.byref(cost)) == L.EINVAL, thr
        assert b"threshold" in lib.rsac_last_error()
    assert lib.rsac_hom_cost_host(None, None, 4, H.ctypes.data, THR, C.byref(cnt), C.byref(cost)) == L.EINVAL
    assert lib.rsac_hom_cost_host(s.ctypes.data, d.ctypes.data, 4, H.ctypes.data, THR, C.byref(cnt), None) == L.EINVAL
    assert lib.rsac_hom_cost_host(s.ctypes.data, d.ctypes.data, 4, H.ctypes.data, THR, C.byref(cnt),
                                  C.byref(cost)) == L.OK
    assert (cnt.value, cost.value) == (4, 0)
