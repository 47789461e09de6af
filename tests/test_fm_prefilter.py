"""Fundamental-matrix f32 Sampson pre-filter, on the CPU: the NumPy
restatement of the band (fmbandref) against the f64 decision of the oracle, on scenes built to sit
on the threshold, on ill-conditioned model families, at the edges of the frame and of the
threshold.  Soundness: a pair the band decides is decided as the f64 test decides it.  Non-vacuity:
the ladder scenes put at least 1 % of all pairs in the band and 1 % just outside it on either side.
The GPU side of the same scenes is test_fm_prefilter_gpu.py.
"""
import functools
from fractions import Fraction

import numpy as np
import pytest

import fmbandref as R
import pyoracle as O

H = 512  # hypotheses per scene (models of O.fm_hypotheses(..., models=True))
_scenes = R.all_scenes


def _names(*kinds):
    return [k for k, v in _scenes().items() if v[3] in kinds]


@functools.lru_cache(maxsize=8)
def _models(name):
    p1, p2, thr, _ = _scenes()[name]
    soa = O.soa_hom(p1, p2)
    _, status, mdl = O.fm_hypotheses(soa, thr, R.SEED, H, models=True)
    F, valid = mdl[:, :9].copy(), mdl[:, 12] != 0
    assert np.array_equal(valid, status > 0)
    return soa, F, valid, float(O.thr2(thr)), R.exact_masks(soa, F, valid, thr)


@functools.lru_cache(maxsize=None)
def _shares(name, mutant=None):
    """The restatement on one scene -> dict: wrong (decisions against the f64 test), und (share of
    undecided pairs), und_valid (the same over the valid models' pairs), near_in / near_out (decided
    inliers with r^2 / (T den) in (0.99, 1), decided outliers in (1, 1.01), shares of all pairs),
    all_in (every pair a decided inlier)."""
    soa, F, valid, T, exact = _models(name)
    d = R.decide(soa, F, valid, T, mutant)
    ratio = R.sampson_ratio(soa, F, T)
    with np.errstate(all="ignore"):
        near_in = float(((d == R.IN) & (ratio > 0.99) & (ratio < 1.0)).mean())
        near_out = float(((d == R.OUT) & (ratio > 1.0) & (ratio < 1.01)).mean())
    return dict(wrong=int((((d == R.IN) & ~exact) | ((d == R.OUT) & exact)).sum()),
                und=float((d == R.UNDECIDED).mean()),
                und_valid=float((d[valid] == R.UNDECIDED).mean()) if valid.any() else float("nan"),
                near_in=near_in, near_out=near_out, all_in=bool((d == R.IN).all()))


# ---------------------------------------------------------------------------------------------
# the restatement's own arithmetic
# ---------------------------------------------------------------------------------------------
def _fma_exact(a, b, c):
    """fmaf by rational arithmetic: the exact a b + c, rounded once to f32 (round to nearest even)"""
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if x == 0:
        return np.float32(0.0)
    lo = np.float32(float(x))                 # a candidate within one f64 + one f32 rounding
    cands = {float(np.nextafter(lo, np.float32(-np.inf))), float(lo), float(np.nextafter(lo, np.float32(np.inf)))}
    cands = [v for v in cands if np.isfinite(v)]
    best = min(cands, key=lambda v: (abs(Fraction(v) - x), int(np.float32(v).view(np.uint32)) & 1))
    return np.float32(best)


def test_fma32_rounds_once():
    rng = np.random.default_rng(1)
    a = rng.normal(size=4000).astype(np.float32)
    b = rng.normal(size=4000).astype(np.float32)
    # c near -a b (cancellation) for most, unrelated for the first 1000
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.normal(size=4000) * 1e-4)).astype(np.float32)
    c[:1000] = rng.normal(size=1000).astype(np.float32) * np.float32(1e-3)
    # double rounding: a b = -2^-25 + 2^-71 and c = 1 - 2^-24, so a b + c lies 2^-71 above the middle
    # of c and its lower neighbour.  The f64 sum loses the 2^-71 and lands on the tie, which rounds to
    # even (the lower neighbour); the fma rounds to c.
    a = np.r_[a, np.float32(-(2.0 ** -13 - 2.0 ** -36))]
    b = np.r_[b, np.float32(2.0 ** -12 + 2.0 ** -35)]
    c = np.r_[c, np.float32(1 - 2.0 ** -24)]
    got = R.fma32(a, b, c)
    want = np.array([_fma_exact(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert got[-1] == c[-1] and naive[-1] != got[-1], "the double-rounding case must tell the two apart"
    # non-finite operands pass through as IEEE has them
    assert np.isnan(R.fma32(np.float32(np.inf), np.float32(0), np.float32(1)))
    assert R.fma32(np.float32(3e38), np.float32(3e38), np.float32(1)) == np.inf
    assert np.isnan(R.fma32(np.float32(np.inf), np.float32(1), np.float32(-np.inf)))


def test_frame_edges_of_the_restatement():
    # zero half-range everywhere: s = 1 (frexp(1.0) = 0.5 * 2^1 -> s = 2); empty problem: centre 0
    one = tuple(np.full(3, v, np.float32) for v in (5.0, 6.0, 7.0, 8.0))
    fr = R.fm_frame(*R.fm_bounds(one))
    assert fr.s == 2.0 and np.array_equal(fr.c, np.float32([5, 6, 7, 8])) and not fr.hb.any()
    empty = tuple(np.zeros(0, np.float32) for _ in range(4))
    fr = R.fm_frame(*R.fm_bounds(empty))
    assert fr.s == 2.0 and not fr.c.any()
    # a NaN poisons coordinate 0 only; 1e31 is past fm_frame's 1e30 (s falls back), 1e29 is not
    nan = tuple(np.float32([1.0, np.nan if k == 3 else 2.0]) for k in range(4))
    lo, hi = R.fm_bounds(nan)
    assert lo[0] == -np.inf and hi[0] == np.inf and lo[3] == 1.0 and hi[3] == 1.0
    assert np.isnan(R.fm_frame(lo, hi).hb[0])
    far = tuple(np.float32([0.0, 1e31 if k == 1 else 1.0]) for k in range(4))
    assert R.fm_frame(*R.fm_bounds(far)).s == 2.0
    far = tuple(np.float32([0.0, 1e29 if k == 1 else 1.0]) for k in range(4))
    assert R.fm_frame(*R.fm_bounds(far)).s == 2.0 ** 96


# ---------------------------------------------------------------------------------------------
# soundness and non-vacuity
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names("ladder", "family"))
def test_ladder_scenes_sound(name):
    r = _shares(name)
    print(f"{name}: undecided {r['und']:.4%}, decided inliers in (0.99, 1) {r['near_in']:.4%}, "
          f"decided outliers in (1, 1.01) {r['near_out']:.4%}, wrong decisions {r['wrong']}")
    assert r["wrong"] == 0


@pytest.mark.parametrize("name", _names("ladder"))
def test_ladder_scenes_are_not_vacuous(name):
    """Conditions on the scene, met by the restatement alone: >= 1 % of all pairs undecided, >= 1 %
    decided inliers with r^2 / (T den) in (0.99, 1), >= 1 % decided outliers in (1, 1.01)."""
    r = _shares(name)
    print(f"{name}: undecided {r['und']:.4%}, decided inliers in (0.99, 1) {r['near_in']:.4%}, "
          f"decided outliers in (1, 1.01) {r['near_out']:.4%}")
    assert r["und"] >= 0.01 and r["near_in"] >= 0.01 and r["near_out"] >= 0.01


@pytest.mark.parametrize("mutant", ["a", "b"])
def test_soundness_check_notices_a_wrong_band(mutant):
    # the band without its margins (Alo = Chi = Th, no beta), and Th = T / s: both must decide pairs
    # of scene A wrongly, or the soundness test above proves nothing
    wrong = _shares("A_1.5", mutant)["wrong"]
    print(f"mutant ({mutant}) of the restatement on scene A, 1.5 px: {wrong} wrong decisions")
    assert wrong > 0


def test_unscaled_record_decides_the_far_point_wrongly():
    # the record as it was (F^ = s^2 F unscaled, no guard on den): under a far point of 1e12 the
    # far point's own den overflows to +inf beside a finite r^2 and reads as a decided inlier
    soa, F, valid, T, exact = _models("C_far_1e+12_y2")
    d = R.decide(soa, F, valid, T, rescale=False)
    hyp, pt = np.nonzero(((d == R.IN) & ~exact) | ((d == R.OUT) & exact))
    print(f"unscaled record, far point 1e12 in y2: {hyp.size} wrong decisions, hypotheses {hyp.tolist()}")
    assert hyp.size > 0 and (pt == len(soa[0]) - 1).all() and (d[hyp, pt] == R.IN).all()


# ---------------------------------------------------------------------------------------------
# frame edges (C) and thresholds (D)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names("finite", "coarse", "degenerate", "threshold"))
def test_edge_scenes_sound(name):
    """Measured shares of undecided pairs (512 hypotheses; DESIGN.md section 9 has the table).
    Under a finite frame that resolves the image the pre-filter must still filter: less than 50 %
    undecided.  The far point 1e6 in y1 / y2 is the hard case (21.2 % / 19.9 %; 96.8 % / 96.5 % with
    eta fixed at 1e-3, where beta = e_r^2 / eta exceeded T den): fm_write_record's per-record eta is
    there for it."""
    kind = _scenes()[name][3]
    r = _shares(name)
    print(f"{name} ({kind}): undecided {r['und']:.4%} of all pairs, {r['und_valid']:.4%} of the valid models' pairs")
    assert r["wrong"] == 0
    if kind == "degenerate":
        # a non-finite or over-range frame: the f64 test decides every pair of every valid model
        assert r["und_valid"] == 1.0
    elif kind == "finite":
        assert r["und"] < 0.5


def test_threshold_edges_by_value():
    # T = thr2 in f32: 1e-30 and 0 give T = 0 (only r = 0 is an inlier), 1e30 and inf give +inf,
    # NaN stays NaN: under an infinite or NaN T the band decides nothing
    for thr, T in ((1e-30, 0.0), (0.0, 0.0), (1e30, np.inf), (float("inf"), np.inf)):
        assert float(O.thr2(thr)) == T
    assert np.isnan(O.thr2(float("nan")))
    for thr in (1e30, float("inf"), float("nan")):
        assert _shares(f"D_thr_{thr!r}")["und_valid"] == 1.0
    # 1e6 px: every pair is a decided inlier
    r = _shares("D_thr_1000000.0")
    assert r["und"] == 0.0 and r["all_in"]
