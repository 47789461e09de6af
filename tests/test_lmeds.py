"""LMedS homography without a GPU: the host twin of the median kernel (rsac_hom_median_host, the
source k_hom_median runs), the sigma rule, the scan and the iteration count against the NumPy
restatement of tests/lmedsref.py, and the restatement against the cross-check table.  Every
comparison is equality (a NaN median compares as NaN).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lmedsref as M  # noqa: E402
import pyoracle as O  # noqa: E402
import rsac  # noqa: E402
import rsac.cv2compat as cv2c  # noqa: E402

ROWS = range(len(M.TABLE))
DBL_MAX = sys.float_info.max


def _same(a, b):
    """equality of medians, NaN equal to NaN"""
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


@pytest.mark.parametrize("row", ROWS)
def test_restatement_reproduces_the_table(row):
    key, (best, median, ones) = M.TABLE[row]
    ref = M.lmeds_case(*key)
    assert (ref["status"] == 1).all() and len(ref["status"]) == 55 and ref["iters"] == 55
    assert (ref["best"], ref["median"], int(ref["mask"].sum())) == (best, median, ones)


def test_first_row_sits_at_the_sigma_floor_with_repeated_medians():
    ref = M.lmeds_case(*M.TABLE[0][0])
    assert M.sigma(ref["median"], 5) == 0.001
    med = ref["medians"]
    assert sum(med[i] in med[:i] for i in range(len(med))) == 51


def test_lmeds_and_the_count_rule_pick_different_hypotheses():
    # the count rule at 3 px over the same 55 hypotheses: the first hypothesis with the most inliers
    # (with these inputs the two rules agree at 64, 257, 2049 and 5000 points and differ at 5, 12 and 65)
    picks = {}
    for key, (best, _, _) in M.TABLE:
        pr = M.problem(*key)
        soa = O.soa_hom(pr["src"], pr["dst"])
        subs, sst = O.mwc_subsets(key[0], 55, 4, hom=soa)
        counts, status = O.hom_hypotheses(soa, 3.0, M.SEED, 55, subsets=subs, sub_status=sst)
        assert (status == 1).all()
        picks[key[0]] = (best, int(np.argmax(counts)))
    assert picks[64] == (6, 6) and picks[2049] == (31, 31) and picks[257] == (46, 46) and picks[5000] == (1, 1)
    assert picks[5] == (1, 0) and picks[12] == (44, 27) and picks[65] == (8, 35)


@pytest.mark.parametrize("row", ROWS)
def test_host_median_equals_restatement_for_every_model(row):
    key = M.TABLE[row][0]
    pr = M.problem(*key)
    status, med, models, _ = M.hypotheses_case(*key, 55)
    host = [rsac.hom_median(pr["src"], pr["dst"], models[h, :9]) for h in range(55)]
    assert _same(host, med)


IDENT = np.eye(3)
# h6 = -1: the denominator h6 x + h7 y + 1 vanishes at x = 1
POLE = np.array([[1.0, 0, 0], [0, 1, 0], [-1, 0, 1]])


def _offsets(d):
    """points whose error under the identity is exactly d_i^2 (small integers: exact in f32)"""
    d = np.asarray(d, np.float64)
    src = np.zeros((len(d), 2))
    return src, np.c_[d, np.zeros(len(d))]


def _check(src, dst, H):
    got = rsac.hom_median(src, dst, H)
    assert _same(got, M.median_of_errors(M.hom_err(H, O.soa_hom(src, dst))))
    return got


def test_median_odd_even_and_duplicates():
    assert _check(*_offsets([3, 1, 2, 2, 5]), IDENT) == 4.0            # 1 4 4 9 25
    assert _check(*_offsets([5, 1, 3, 2]), IDENT) == 6.5               # 1 4 9 25 -> (4 + 9) / 2
    assert _check(*_offsets([2, 2, 2, 2]), IDENT) == 4.0               # the lower middle equals the upper
    assert _check(*_offsets([1, 2, 2, 3, 3, 3]), IDENT) == 6.5         # 1 4 4 | 9 9 9: the largest key below
    assert _check(*_offsets([1, 1, 2, 2, 2, 3]), IDENT) == 4.0
    assert _check(*_offsets([7]), IDENT) == 49.0
    assert _check(*_offsets([1, 3]), IDENT) == 5.0
    assert _check(*_offsets([0, 0, 0, 0, 0]), IDENT) == 0.0


def test_even_median_adds_in_f32():
    # 1 + 2^24 is not an f32: the f32 sum of the middle keys rounds (to 2^24) before the f64 halving,
    # where an f64 sum would give 2^23 + 0.5
    assert _check(*_offsets([1, 4096]), IDENT) == 2.0**23
    assert _check(*_offsets([0, 1, 4096, 5000]), IDENT) == 2.0**23


def test_median_with_an_infinite_error():
    # x = 1, y = 1 under POLE: both numerators non-zero over a zero denominator -> inf + inf
    src = np.array([[0, 0], [0, 0], [1, 1], [0, 0], [0, 0]], np.float64)
    dst = np.array([[1, 0], [2, 0], [0, 0], [3, 0], [4, 0]], np.float64)
    e = M.hom_err(POLE, O.soa_hom(src, dst))
    assert np.isinf(e[2]) and np.isfinite(np.delete(e, 2)).all()
    assert _check(src, dst, POLE) == 9.0
    # three of five infinite: the median is +inf, below a NaN
    src[0] = src[1] = (1, 1)
    assert _check(src, dst, POLE) == np.inf


def test_a_nan_error_ranks_last():
    # x = 1, y = 0 under POLE: ey = 0 * inf = NaN
    src = np.array([[1, 0], [0, 0], [0, 0], [1, 1]], np.float64)
    dst = np.array([[0, 0], [1, 0], [2, 0], [0, 0]], np.float64)
    e = M.hom_err(POLE, O.soa_hom(src, dst))
    assert np.isnan(e[0]) and np.isinf(e[3])
    assert _check(src, dst, POLE) == np.inf               # 1 4 | inf NaN -> (4 + inf) / 2
    assert _check(src[:3], dst[:3], POLE) == 4.0          # 1 4 NaN
    assert np.isnan(_check(src[[0, 3]], dst[[0, 3]], POLE))  # inf NaN: the f32 sum is NaN


def test_more_than_half_nan_gives_a_nan_median_that_never_wins():
    src = np.array([[1, 0], [1, 0], [1, 0], [0, 0], [0, 0]], np.float64)
    dst = np.array([[0, 0], [0, 0], [0, 0], [1, 0], [2, 0]], np.float64)
    med = _check(src, dst, POLE)
    assert np.isnan(med)
    sc = rsac.LmedsScan(3).step([1, 1, 1], [med, 5.0, med])
    assert (sc.best, sc.best_median, sc.iter, sc.done) == (1, 5.0, 3, True)
    sc = rsac.LmedsScan(2).step([1, 1], [med, med])
    assert (sc.best, sc.best_median) == (-1, DBL_MAX)


def test_sigma_and_its_floor():
    for med, n in [(4.646750450134277, 64), (0.8609719276428223, 12), (1e-3, 5), (250.0, 100000), (6.5, 6)]:
        assert rsac.lmeds_sigma(med, n) == M.sigma(med, n)
    assert rsac.lmeds_sigma(0.0, 10) == 0.001
    assert rsac.lmeds_sigma(9.313225746154785e-10, 5) == 0.001
    assert rsac.lmeds_sigma(1.0, 5) == 2.5 * 1.4826 * 6.0
    # just above the floor
    m = (0.0011 / (2.5 * 1.4826 * (1 + 5.0 / 96))) ** 2
    assert rsac.lmeds_sigma(m, 100) == M.sigma(m, 100) > 0.001


def _scan_equal(status, med, niters, chunks=None):
    status = np.asarray(status, np.int8)
    med = np.asarray(med, np.float64)
    sc = rsac.LmedsScan(niters)
    if chunks is None:
        sc.step(status, med)
    else:
        i = 0
        for c in chunks:
            sc.step(status[i:i + c], med[i:i + c])
            i += c
    ref = M.scan(status, med, niters)
    assert (sc.best, sc.best_median, sc.iter) == ref
    return sc


def test_scan_rules():
    sc = _scan_equal([1, 1, 1, 1], [3.0, 2.0, 2.0, 2.5], 4)       # ties keep the earlier index
    assert (sc.best, sc.best_median, sc.done) == (1, 2.0, True)
    sc = _scan_equal([0, 1, 0, 1], [-1.0, 7.0, -1.0, 6.0], 4)     # status 0 is skipped (its -1 never wins)
    assert sc.best == 3
    sc = _scan_equal([-1, 1, 1], [-1.0, 1.0, 1.0], 3)             # no subset at hypothesis 0: no model
    assert (sc.best, sc.iter, sc.done) == (-1, 0, True)
    sc = _scan_equal([1, 1, -1, 1], [5.0, 4.0, -1.0, 1.0], 4)     # ... mid-way: the scan ends there
    assert (sc.best, sc.iter, sc.done) == (1, 2, True)
    sc = _scan_equal([1, 1, 1], [np.nan, np.inf, np.nan], 3)      # inf < DBL_MAX is false too
    assert sc.best == -1
    sc = _scan_equal([1, 1, 1, 1], [4.0, 3.0, 2.0, 1.0], 2)       # the budget ends the scan
    assert (sc.best, sc.iter, sc.done) == (1, 2, True)
    sc = _scan_equal([1, 1], [4.0, 3.0], 5)                       # fewer rows than the budget: not done
    assert (sc.best, sc.iter, sc.done) == (1, 2, False)


def test_scan_in_chunks_equals_one_call():
    rng = np.random.default_rng(7)
    for trial in range(20):
        H = int(rng.integers(1, 200))
        status = rng.choice([1, 1, 1, 0], H).astype(np.int8)
        if trial % 4 == 0:
            status[int(rng.integers(0, H))] = -1
        med = np.round(rng.random(H) * 8, 1)  # many ties
        med[rng.random(H) < 0.1] = np.nan
        niters = int(rng.integers(1, 250))
        one = _scan_equal(status, med, niters)
        cuts = sorted(rng.integers(0, H + 1, 3))
        chunks = [cuts[0], cuts[1] - cuts[0], cuts[2] - cuts[1], H - cuts[2]]
        many = _scan_equal(status, med, niters, chunks)
        assert (one.best, one.iter, one.done) == (many.best, many.iter, many.done)


def test_iteration_count_rule():
    assert rsac.lmeds_num_iters(0.995, 2000) == 55 == M.num_iters(0.995, 2000)
    assert rsac.lmeds_num_iters(0.99, 2000) == M.num_iters(0.99, 2000) == 48
    assert rsac.lmeds_num_iters(0.995, 20) == 20                   # capped by max_iters
    assert rsac.lmeds_num_iters(0.01, 2000) == 3                   # RANSACUpdateNumIters gives 0: the max(..., 3)
    assert O.update_num_iters(0.01, 0.45, 4, 2000) == 0
    assert rsac.lmeds_num_iters(0.995, 1) == 3 == M.num_iters(0.995, 1)  # ... also above max_iters


def test_shim_method_table():
    assert (cv2c.LMEDS, cv2c.RANSAC, cv2c.RHO) == (4, 8, 16)
    s = np.random.default_rng(1).random((8, 2))
    with pytest.raises(NotImplementedError, match="RHO"):
        cv2c.findHomography(s, s, cv2c.RHO)


def test_python_argument_checks():
    s = np.zeros((8, 2))
    with pytest.raises(ValueError):
        rsac.homography_lmeds(s, s[:7])
    with pytest.raises(ValueError):
        rsac.hom_median(s, s[:7], np.eye(3))
    assert rsac.RansacInfo(True, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0).median is None
