"""MSAC scoring without a GPU: the host pieces of the feature (rsac_msac_shift, rsac_pnp_cost_host,
rsac_scan_msac -- the RSAC_HD source the kernel runs and the scan run_loop calls) against the NumPy
restatement of tests/msacref.py, and the Python interface's argument checks.  Every comparison is
exact equality.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import msacref as M  # noqa: E402
import pyoracle as O  # noqa: E402
import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402

THR, SEED = M.THR, M.SEED
INPUTS = [row[0] for row in M.TABLE]


def test_msac_shift():
    thrs = (0.4, 1, 3, 8, 30, 60, 75)
    assert [rsac.msac_shift(t) for t in thrs] == [22, 19, 16, 13, 10, 8, 7]
    assert [M.shift(t) for t in thrs] == [22, 19, 16, 13, 10, 8, 7]
    for t in thrs:  # Q = q(thr2) lies in [2^19, 2^20)
        t2 = np.float32(O.thr2(t))
        assert 2**19 <= int(M.q(np.array([t2]), M.shift(t))[0]) < 2**20


@pytest.mark.parametrize("n,outl,seed", INPUTS + [M.BIG])
def test_pose_cost_equals_reference(n, outl, seed):
    pr = M.problem(n, outl, seed)
    status, cnt, cost, models = M.hypotheses_case(n, outl, seed, 64)
    assert (status > 0).any()
    for h in np.flatnonzero(status > 0):
        assert rsac.pose_cost(pr["points2d"], pr["points3d"], pr["K"], models[h, :12], THR) == \
            (int(cnt[h]), int(cost[h])), h
    if (n, outl, seed) == M.BIG:  # the 64-bit case: the largest cost passes 2^32
        assert int(cost.max()) == 4297588736 and cost.max() > 2**32


def test_pose_cost_degenerate_points():
    """A point at z == 0 projects with 1 / z replaced by 1 (pnp_err), far off any pixel: it costs Q.
    A pose whose projection is NaN (inf * 0) fails e <= thr2 and costs Q as well."""
    K = np.array([[800.0, 0, 320], [0, 800.0, 240], [0, 0, 1]])
    p3 = np.array([[0.0, 0, 5], [1, 0, 5], [0, 1, 5], [1, 1, 0], [2, 1, 5]])
    p2 = np.array([[320.0, 240], [480, 240], [320, 400], [100, 100], [640.5, 400.25]])
    k = M.shift(THR)
    Q = int(M.q(np.array([np.float32(O.thr2(THR))]), k)[0])
    assert (k, Q) == (13, 524288)
    soa, cam = O.soa_pnp(p3, p2), O.cam_from_K(K)
    m = np.r_[np.eye(3).reshape(9), np.zeros(3)]  # identity pose: point 3 has z == 0
    e = M.errors(m[:9], m[9:], soa, cam)
    inl, pc = M.point_costs(e, THR)
    assert list(inl) == [True, True, True, False, True] and pc[3] == Q
    assert 0 < pc[4] < Q  # a fractional inlier error: (0.5^2 + 0.25^2) 2^13
    assert pc[4] == int(0.3125 * 2**13)
    assert rsac.pose_cost(p2, p3, K, m, THR) == (4, int(pc.sum()))
    m_nan = np.r_[np.eye(3).reshape(9), [np.inf, 0.0, np.inf]]  # x = inf, 1 / z = 0: NaN projection
    with np.errstate(invalid="ignore"):
        e = M.errors(m_nan[:9], m_nan[9:], soa, cam)
    assert np.isnan(e).all()
    assert rsac.pose_cost(p2, p3, K, m_nan, THR) == (0, 5 * Q)


def _scan(counts, costs, status, n, mp, conf, max_iters, chunks=None):
    st = L.ScanMsacState()
    L.lib().rsac_scan_msac_init(C.byref(st), int(max_iters))
    counts = np.ascontiguousarray(counts, np.int32)
    costs = np.ascontiguousarray(costs, np.int64)
    status = np.ascontiguousarray(status, np.int8)
    pos = 0
    for ln in (chunks or [len(status)]):
        a, b, c = counts[pos:pos + ln], costs[pos:pos + ln], status[pos:pos + ln]
        assert L.lib().rsac_scan_msac(C.byref(st), a.ctypes.data, b.ctypes.data, c.ctypes.data, ln, n, mp, conf) == 0
        pos += ln
    return st.best, st.best_cost, st.max_good, st.iter, st.niters, st.done


@pytest.mark.parametrize("row", range(len(M.TABLE)))
def test_scan_msac_on_oracle_rows(row):
    (n, outl, seed), (best, cost, count, iters) = M.TABLE[row]
    H = 4096 if row == 5 else 256  # row 6 of the table leaves the first 256 hypotheses
    status, cnt, c, _ = M.hypotheses_case(n, outl, seed, H)
    ref = M.scan(c, cnt, status, n, 4, 0.99, 5000)
    assert ref == (best, cost, count, iters)
    assert _scan(cnt, c, status, n, 4, 0.99, 5000)[:4] == ref
    assert _scan(cnt, c, status, n, 4, 0.99, 5000, chunks=[100, H - 100])[:4] == ref


def test_count_rule_differs_where_the_issue_says():
    for row, count_best in M.COUNT_BEST.items():
        (n, outl, seed), (best, _, _, _) = M.TABLE[row]
        pr = M.problem(n, outl, seed)
        ref = O.pnp_ransac(pr["points3d"], pr["points2d"], pr["K"], THR, 0.99, 5000, SEED)
        assert ref["best"] == count_best != best


def test_scan_msac_constructed_rows():
    n, mp, conf = 100, 4, 0.99
    # equal costs: the earlier index stays
    cnt, cost, st = [50, 50, 50], [700, 700, 700], [1, 1, 1]
    assert _scan(cnt, cost, st, n, mp, conf, 3)[:4] == M.scan(cost, cnt, st, n, mp, conf, 3) == (0, 700, 50, 3)
    # a cheaper hypothesis with count <= model_points - 1 is ignored (also as the first candidate)
    cnt, cost, st = [3, 60, 3, 2], [10, 900, 5, 1], [1, 1, 1, 1]
    assert _scan(cnt, cost, st, n, mp, conf, 4)[:4] == M.scan(cost, cnt, st, n, mp, conf, 4) == (1, 900, 60, 4)
    # a cheaper hypothesis with fewer inliers replaces the best; the bound does not rise
    cnt, cost, st = [90, 40, 40], [5000, 4000, 4500], [1, 1, 1]
    hi = O.update_num_iters(conf, (n - 90) / n, mp, 1000)
    assert hi < O.update_num_iters(conf, (n - 40) / n, mp, 1000)  # the count rule's bound for 40 is larger
    r = _scan(cnt, cost, st, n, mp, conf, 1000)
    assert r[:4] == M.scan(cost, cnt, st, n, mp, conf, 1000) == (1, 4000, 40, 3)
    assert r[4] == hi
    # status 0 is skipped, status < 0 ends the scan mid-row
    cnt, cost, st = [50, 0, 60, 70], [900, -1, 800, 100], [1, 0, -1, 1]
    r = _scan(cnt, cost, st, n, mp, conf, 1000)
    assert r[:4] == M.scan(cost, cnt, st, n, mp, conf, 1000) == (0, 900, 50, 2)
    assert r[5] == 1
    # no eligible hypothesis at all
    assert _scan([3, 0], [1, -1], [1, 0], n, mp, conf, 2)[:4] == M.scan([1, -1], [3, 0], [1, 0], n, mp, conf, 2) \
        == (-1, -1, 0, 2)
    # two chunks equal one chunk, wherever the cut falls (random rows, ties included)
    rng = np.random.default_rng(3)
    cnt = rng.integers(0, 40, 400).astype(np.int32)
    cost = rng.integers(1000, 1040, 400).astype(np.int64)
    st = rng.choice([0, 1, 1, 1], 400).astype(np.int8)
    ref = M.scan(cost, cnt, st, n, mp, conf, 400)
    for cut in (1, 7, 200, 399):
        assert _scan(cnt, cost, st, n, mp, conf, 400, chunks=[cut, 400 - cut])[:4] == ref


def test_python_argument_checks():
    pr = M.problem(12, .25, 5)
    a = (pr["points2d"], pr["points3d"], pr["K"])
    with pytest.raises(ValueError, match="score"):
        rsac.pnp_ransac(*a, score="bogus")
    with pytest.raises(ValueError, match="score"):
        rsac.pnp_ransac_batched([a[0]], [a[1]], [a[2]], score="bogus")
    with pytest.raises(ValueError, match="score"):
        rsac.pnp_ransac_batched_flat(a[0], a[1], [0, 12], [a[2]], score="bogus")
    # the unsupported combinations raise before any device work (there is no device here)
    with pytest.raises(NotImplementedError, match="lo"):
        rsac.pnp_ransac(*a, score="msac", lo=True)
    with pytest.raises(NotImplementedError, match="dist"):
        rsac.pnp_ransac(*a, score="msac", dist=[0.1, 0.0, 0.0, 0.0])
    with pytest.raises(NotImplementedError, match="dist"):
        rsac.pnp_ransac_batched([a[0]], [a[1]], [a[2]], score="msac", dist=[0.1, 0.0, 0.0, 0.0])
    with pytest.raises(NotImplementedError, match="score"):
        rsac.pnp_ransac_batched_rows(a[0], a[1], [0, 12], [a[2]], score="msac")
    with pytest.raises(NotImplementedError, match="score"):
        rsac.pnp_ransac_first_round(*a, score="msac")
    with pytest.raises(NotImplementedError, match="score"):
        rsac.estimate_camera_orientation(a[1], a[0], [1000.0], [(36.0, 24.0)], (640, 480), score="msac")
    with pytest.raises(NotImplementedError, match="costs"):
        rsac.hypotheses("homography", a[0], a[0], costs=True)
    info = rsac.RansacInfo(True, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0)
    assert info.cost == -1 and np.isnan(info.cost_px2)


def test_host_entry_points_reject_bad_arguments():
    cnt, cost = C.c_int32(0), C.c_int64(0)
    K = np.eye(3).reshape(9)
    m = np.zeros(12)
    p3, p2 = np.zeros((4, 3)), np.zeros((4, 2))
    lib = L.lib()
    assert lib.rsac_pnp_cost_host(p3.ctypes.data, p2.ctypes.data, 4, K.ctypes.data, m.ctypes.data, 0.0,
                                  C.byref(cnt), C.byref(cost)) == L.EINVAL
    assert b"threshold" in lib.rsac_last_error()
    assert lib.rsac_scan_msac(None, None, None, None, 0, 10, 4, 0.99) == L.EINVAL
