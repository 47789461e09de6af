"""The least-squares fundamental matrix on the host (rsac_fundamental_fit, no GPU) against the NumPy
restatement of tests/fmfitref.py -- exact equality -- and against an independent np.linalg
reference; the local-optimisation loop restated on the host fit; the pinned table of DESIGN.md
"Fundamental matrix: least-squares refit and local optimisation".

Inputs: synth.fundamental_problem at its default noise.  A masked fit of m points takes, by mask
shape: "ones" -- a problem of m points, no mask; "third" -- the smallest problem whose points with
i % 3 != 0 number m; "winner" -- the problem of 2 m + 16 points at 30 % outliers, the mask of the
oracle's RANSAC winner (500 iterations) cut after its first m ones.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fmfitref as R  # noqa: E402
import pyoracle as O  # noqa: E402
import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402

SIZES = [8, 9, 12, 13, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025]
SHAPES = ["ones", "winner", "third"]
# the largest Frobenius distance (unit norm, up to sign) between the host fit and fit_linalg over
# SIZES x SHAPES, measured with the host twin: 1.586e-13 at (8, "winner") -- the two smallest
# eigenvalues of a fit of 8 noisy points lie close together.  The bound is 100 times that.
LINALG_MEASURED = 1.586e-13
LINALG_BOUND = 100 * LINALG_MEASURED
assert LINALG_BOUND < 1e-6


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


@functools.lru_cache(maxsize=None)
def masked_case(m, shape):
    """-> (key, mask or None) with exactly m masked points"""
    if shape == "ones":
        return (m, 0.0 if m < 64 else .3, 200 + m), None
    if shape == "third":
        n = m
        while int((np.arange(n) % 3 != 0).sum()) < m:
            n += 1
        return (n, 0.0 if m < 64 else .3, 300 + m), np.arange(n) % 3 != 0
    key = (2 * m + 16, .3, 400 + m)
    pr = R.problem(*key)
    mask = O.fm_ransac(pr["pts1"], pr["pts2"], R.THR, R.CONF, 500, R.SEED)["mask"].copy()
    ones = np.flatnonzero(mask)
    assert len(ones) >= m
    mask[ones[m:]] = False
    return key, mask


@functools.lru_cache(maxsize=None)
def fits(m, shape):
    """-> (host fit, restatement, np.linalg reference, rank bound) of one case, computed once"""
    key, mask = masked_case(m, shape)
    pr, soa = R.problem(*key), R.soa_of(key)
    assert (len(soa[0]) if mask is None else int(mask.sum())) == m
    _, (c1x, c1y, s1, c2x, c2y, s2), cnt = R.moment_matrix(soa, mask)
    assert cnt == m
    T1 = np.array([[s1, 0, -s1 * c1x], [0, s1, -s1 * c1y], [0, 0, 1.0]])
    T2 = np.array([[s2, 0, -s2 * c2x], [0, s2, -s2 * c2y], [0, 0, 1.0]])
    return (rsac.fundamental_fit(pr["pts1"], pr["pts2"], mask), R.fit(soa, mask), R.fit_linalg(soa, mask),
            8 * 2.0 ** -52 * np.linalg.cond(T1) * np.linalg.cond(T2))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("m", SIZES)
def test_host_fit_equals_restatement(m, shape):
    Fh, Fr, _, _ = fits(m, shape)
    assert Fh is not None and Fr is not None
    assert _bits_equal(Fh, Fr)
    assert abs(np.linalg.norm(Fh) - 1.0) < 4 * 2.0 ** -52


def test_host_fit_against_linalg():
    worst = 0.0
    for m in SIZES:
        for shape in SHAPES:
            Fh, _, Fl, _ = fits(m, shape)
            d = R.sign_distance(Fh, Fl)
            print(m, shape, "%.3e" % d)
            worst = max(worst, d)
    print("largest distance %.3e, bound %.3e" % (worst, LINALG_BOUND))
    assert worst <= LINALG_BOUND


def test_rank_two():
    """fm_finish removes the smallest right-singular direction of the normalised matrix: Fn v = 0 up
    to a few roundings (8 eps of its norm), and F = T2^T Fn T1 keeps a singular-value ratio of at
    most that times cond(T1) cond(T2)"""
    for m in SIZES:
        for shape in SHAPES:
            Fh, _, _, bound = fits(m, shape)
            s = np.linalg.svd(Fh, compute_uv=False)
            assert s[2] / s[0] <= bound, (m, shape, s[2] / s[0], bound)
            assert s[1] / s[0] > 1e-6  # ... and no more than that is removed


def test_no_model():
    pr = R.problem(64, .3, 2)
    p1, p2 = pr["pts1"], pr["pts2"]
    assert rsac.fundamental_fit(p1[:7], p2[:7]) is None
    m7 = np.zeros(64, bool)
    m7[[0, 9, 18, 27, 36, 45, 63]] = True
    assert rsac.fundamental_fit(p1, p2, m7) is None and R.fit(R.soa_of((64, .3, 2)), m7) is None
    assert rsac.fundamental_fit(p1[:0], p2[:0]) is None
    # all masked points coincident: both mean distances are exactly 0
    q1, q2 = p1.copy(), p2.copy()
    m = np.arange(64) % 2 == 0
    q1[m], q2[m] = q1[0], q2[0]
    assert rsac.fundamental_fit(q1, q2, m) is None and R.fit(O.soa_hom(q1, q2), m) is None
    # ... in one image only
    q2 = p2.copy()
    assert rsac.fundamental_fit(q1, q2, m) is None
    # a NaN / infinite coordinate under the mask
    for bad in (np.nan, np.inf, -np.inf):
        for col in range(4):
            q1, q2 = p1.copy(), p2.copy()
            (q1 if col < 2 else q2)[10, col % 2] = bad
            assert rsac.fundamental_fit(q1, q2) is None, (bad, col)
            assert R.fit(O.soa_hom(q1, q2), None) is None, (bad, col)


def test_nan_outside_the_mask_changes_no_bit():
    key = (257, .3, 8)
    pr = R.problem(*key)
    mask = np.arange(257) % 3 != 0
    want = rsac.fundamental_fit(pr["pts1"], pr["pts2"], mask)
    q1, q2 = pr["pts1"].copy(), pr["pts2"].copy()
    q1[0], q2[3], q1[255, 1], q2[6, 0] = np.nan, np.inf, -np.inf, np.nan
    assert _bits_equal(rsac.fundamental_fit(q1, q2, mask), want)
    assert _bits_equal(R.fit(O.soa_hom(q1, q2), mask), want)


def test_mask_values_are_truth_values():
    pr = R.problem(65, .4, 3)
    mask = np.arange(65) % 3 != 0
    want = rsac.fundamental_fit(pr["pts1"], pr["pts2"], mask)
    assert _bits_equal(rsac.fundamental_fit(pr["pts1"], pr["pts2"], mask.astype(np.uint8) * 255), want)
    assert _bits_equal(rsac.fundamental_fit(pr["pts1"], pr["pts2"], mask.astype(np.float64) * 0.5), want)


@pytest.mark.parametrize("key,want", R.TABLE, ids=[str(k[0]) for k, _ in R.TABLE])
def test_pinned_table(key, want):
    assert R.table_row(key, want[0]) == want
    if key[0] >= 64:
        assert want[2] >= want[1]  # the refit keeps at least the winner's count on these inputs
    r = R.row(key, want[0])
    assert want[3] >= want[2] or want[4] == 0  # an accepted round only ever raises the count
    assert int(r["lo"][R.MAX_ROUNDS][1].sum()) == want[3]


@pytest.mark.parametrize("key,want", R.TABLE, ids=[str(k[0]) for k, _ in R.TABLE])
def test_local_opt_loop_on_the_host_fit(key, want):
    """the loop of rsac_fundamental_local_opt with the library's host fit in place of the restated
    one: the same models, masks, counts and rounds at every cap"""
    pr, soa = R.problem(*key[:3]), R.soa_of(key)
    r = R.row(key, want[0])
    host = lambda s, m: rsac.fundamental_fit(pr["pts1"], pr["pts2"], m)  # noqa: E731
    assert _bits_equal(host(soa, r["mask0"]), r["F1"])
    for cap in (1, 4, 8):
        F, mask, count, steps = R.local_opt(soa, r["F0"], R.THR, cap, host)
        rF, rmask, rcount, rsteps = r["lo"][cap]
        assert (count, steps) == (rcount, rsteps) and steps <= cap
        assert np.array_equal(mask, rmask) and _bits_equal(F, rF)


def test_local_opt_from_a_model_without_support():
    soa = R.soa_of((64, .3, 2))
    F = np.array([[0, 0, 1.0], [0, 0, 0], [0, 0, 0]])  # x2 = 0: no point of the problem is near it
    Fo, mask, count, steps = R.local_opt(soa, F, R.THR, 4)
    assert count < 8 and steps == 0 and _bits_equal(Fo, F)


def test_exports():
    names = {row[0] for row in L.SIGNATURES}
    for name in ("rsac_fundamental_fit", "rsac_fundamental_fit_device", "rsac_fundamental_local_opt"):
        assert name in names and hasattr(L.lib(), name)
    for name in ("fundamental_fit", "fundamental_local_opt"):
        assert name in rsac.__all__ and callable(getattr(rsac, name))
    assert L.lib().rsac_abi_version() == 2


def test_host_abi_codes():
    pr = R.problem(64, .3, 2)
    a, b = np.ascontiguousarray(pr["pts1"]), np.ascontiguousarray(pr["pts2"])
    F = np.full(9, 7.0)
    fit = L.lib().rsac_fundamental_fit
    assert fit(a.ctypes.data, b.ctypes.data, 64, None, F.ctypes.data) == L.OK and abs(np.linalg.norm(F) - 1) < 1e-15
    assert fit(a.ctypes.data, b.ctypes.data, 7, None, F.ctypes.data) == L.NO_MODEL and not F.any()
    assert fit(a.ctypes.data, b.ctypes.data, -1, None, F.ctypes.data) == L.EINVAL
    assert fit(None, b.ctypes.data, 64, None, F.ctypes.data) == L.EINVAL
    assert fit(a.ctypes.data, b.ctypes.data, 64, None, None) == L.EINVAL


def test_bad_arguments_raise_before_any_device_work():
    pr = R.problem(64, .3, 2)
    p1, p2 = pr["pts1"], pr["pts2"]
    for bad in ("lm", "LO", 1, None, 2.0):
        with pytest.raises(ValueError, match="refine"):
            rsac.fundamental_ransac(p1, p2, refine=bad)
        with pytest.raises(ValueError, match="refine"):
            rsac.fundamental_lmeds(p1, p2, refine=bad)
    with pytest.raises(ValueError):
        rsac.fundamental_fit(p1, p2[:63])
    with pytest.raises(ValueError):
        rsac.fundamental_fit(p1, p2, np.ones(63, bool))
    F = np.eye(3)
    for rounds in (0, -1):
        with pytest.raises(ValueError, match="max_rounds"):
            rsac.fundamental_local_opt(p1, p2, F, max_rounds=rounds)
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="reproj_thresh"):
            rsac.fundamental_local_opt(p1, p2, F, thr)
    with pytest.raises(ValueError):
        rsac.fundamental_local_opt(p1, p2, np.eye(4))
    with pytest.raises(ValueError):
        rsac.fundamental_local_opt(p1, p2[:63], F)
