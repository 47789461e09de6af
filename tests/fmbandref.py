"""Fundamental-matrix f32 Sampson pre-filter: a NumPy restatement of the band and the adversarial
scenes of test_fm_prefilter.py / test_fm_prefilter_gpu.py.

The restatement follows k_fm_bounds, fm_frame, fm_write_record and fm_test_f32 operation for
operation: f64 where the kernel computes in double, np.float32 arithmetic (IEEE, rounded once per
operation) where it computes in float, and fma32 for the fused multiply-adds.  It decides every
(model, point) pair as the kernel would: +1 decided inlier, -1 decided outlier, 0 undecided (the
pair the kernel hands to the exact f64 test).  Its two uses: to prove on the CPU that a scene puts
pairs where the band matters, and to check the band's soundness against the f64 decision.  No GPU
assertion depends on it: there the bar is equality with the all-f64 kernel and the oracle.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import pyoracle as O
from rsac import synth

IN, OUT, UNDECIDED = 1, -1, 0
SEED = 3          # the Philox seed of every hypothesis call on these scenes
LADDER0 = 3000    # scene A: points [LADDER0, N_A) are the ladder
N_A = 3300


# ---------------------------------------------------------------------------------------------
# f32 arithmetic
# ---------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c), rounded once.  The product of two f32 is exact in f64 (48 bits); TwoSum adds c
    and keeps the error; the f64 sum is then made "round to odd" (when the error is not zero and
    the sum's last bit is even, step one ulp towards the error), after which the one rounding to
    f32 is the correct rounding of the exact a b + c (53 >= 24 + 2 bits)."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        p = a * b
        s = np.asarray(p + c)
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & even
        s = np.where(fix, np.nextafter(s, np.copysign(np.inf, err)), s)
        return s.astype(np.float32)


# ---------------------------------------------------------------------------------------------
# k_fm_bounds, fm_frame, fm_write_record, fm_test_f32
# ---------------------------------------------------------------------------------------------
def fm_bounds(soa):
    """k_fm_bounds: minima and maxima of x1 y1 x2 y2 (fminf / fmaxf skip a NaN); a NaN anywhere
    sets coordinate 0 to (-inf, +inf); an empty problem keeps the preset (+inf, -inf)."""
    lo = np.full(4, np.inf, np.float32)
    hi = np.full(4, -np.inf, np.float32)
    nan = False
    for k in range(4):
        v = np.asarray(soa[k], np.float32)
        if v.size:
            with np.errstate(all="ignore"):
                lo[k] = np.fmin(lo[k], np.fmin.reduce(v))
                hi[k] = np.fmax(hi[k], np.fmax.reduce(v))
            nan = nan or bool(np.isnan(v).any())
    if nan:
        lo[0], hi[0] = -np.inf, np.inf
    return lo, hi


class Frame:
    __slots__ = ("c", "inv_s", "s", "hb", "pb")


def fm_frame(lo, hi):
    """fm_frame: centres, the common power-of-two scale, the bounds of |x^| and of |x|."""
    f = Frame()
    f.c = np.zeros(4, np.float32)
    f.pb = np.zeros(4)
    f.hb = np.zeros(4)
    half = np.float64(0)
    with np.errstate(all="ignore"):
        for k in range(4):
            l, h = np.float32(lo[k]), np.float32(hi[k])
            if l <= h:
                f.c[k] = (l + h) * np.float32(0.5)
            pb = np.fmax(np.abs(np.float64(l)), np.abs(np.float64(h)))
            f.pb[k] = pb
            c = np.float64(f.c[k])
            half = np.fmax(half, np.fmax(np.float64(h) - c, c - np.float64(l)))
        _, e = math.frexp(float(half) if (half > 0 and half < 1e30) else 1.0)
        f.s = np.float64(math.ldexp(1.0, e))
        f.inv_s = np.float32(np.float64(1.0) / f.s)
        for k in range(4):
            l, h, c = np.float64(lo[k]), np.float64(hi[k]), np.float64(f.c[k])
            f.hb[k] = np.fmax(h - c, c - l) * (1.0 + 1.2e-7) / f.s
    return f


def fm_records(F, valid, fr, T, mutant=None, rescale=True):
    """fm_write_record for H models at once: F (H, 9) f64, valid (H,) -> records (H, 16) f32.
    mutant: None, or "a" / "b" (the band without its margins; Th = T / s), used only to show that
    the soundness test notices them.  rescale=False: the record as it was before F^ was scaled
    into [0.5, 1) and den guarded against overflow, used only to show the
    pairs that the two are there for."""
    F = np.asarray(F, np.float64).reshape(-1, 9)
    valid = np.asarray(valid).astype(bool)
    H = len(F)
    rec = np.zeros((H, 16), np.float32)
    T = np.float64(T)
    with np.errstate(all="ignore"):
        finite = valid & np.isfinite(F).all(axis=1)
        frame_ok = (fr.hb[0] == fr.hb[0]) and bool((fr.pb[[0, 2]] < 1e30).all()) and (not rescale or bool((fr.pb < 1e30).all()))
        full = finite & frame_ok
        s = fr.s
        c0, c1, c2, c3 = (np.float64(v) for v in fr.c)
        f = [F[:, q] for q in range(9)]
        G = [None] * 9
        for i in range(3):
            G[3 * i] = f[3 * i] * s
            G[3 * i + 1] = f[3 * i + 1] * s
            G[3 * i + 2] = f[3 * i] * c0 + f[3 * i + 1] * c1 + f[3 * i + 2]
        Fh = [None] * 9
        for j in range(3):
            Fh[j] = s * G[j]
            Fh[3 + j] = s * G[3 + j]
            Fh[6 + j] = c2 * G[j] + c3 * G[3 + j] + G[6 + j]
        ab = np.abs
        mx = np.fmax
        ke = np.zeros(H, np.int64)
        if rescale:  # 2^-ke F^ with the largest entry in [0.5, 1)
            fmx = np.zeros(H)
            for q in range(9):
                fmx = mx(fmx, ab(Fh[q]))
            _, ke = np.frexp(np.where((fmx > 0) & (fmx < 1e300), fmx, 1.0))
            Fh = [np.ldexp(v, -ke) for v in Fh]
        X1, Y1, X2, Y2 = fr.hb
        Ar = ab(Fh[0]) * X1 + ab(Fh[1]) * Y1 + ab(Fh[2])
        Br = ab(Fh[3]) * X1 + ab(Fh[4]) * Y1 + ab(Fh[5])
        Cr = ab(Fh[6]) * X1 + ab(Fh[7]) * Y1 + ab(Fh[8])
        A2 = ab(Fh[0]) * X2 + ab(Fh[3]) * Y2 + ab(Fh[6])
        B2 = ab(Fh[1]) * X2 + ab(Fh[4]) * Y2 + ab(Fh[7])
        if rescale:  # den32 could overflow: the record leaves every pair undecided
            full = full & (Ar * Ar + Br * Br + A2 * A2 + B2 * B2 < 1e38)
        P1, Q1, P2, Q2 = fr.pb
        Ap = mx(mx(ab(f[0]) * P1 + ab(f[1]) * Q1 + ab(f[2]), ab(f[3]) * P1 + ab(f[4]) * Q1 + ab(f[5])),
                mx(ab(f[0]) * P2 + ab(f[3]) * Q2 + ab(f[6]), ab(f[1]) * P2 + ab(f[4]) * Q2 + ab(f[7])))
        Rp = (P2 * (ab(f[0]) * P1 + ab(f[1]) * Q1 + ab(f[2])) + Q2 * (ab(f[3]) * P1 + ab(f[4]) * Q1 + ab(f[5]))
              + ab(f[6]) * P1 + ab(f[7]) * Q1 + ab(f[8]))
        u = 5.9604644775390625e-08
        e = 4.1 * u * mx(mx(Ar, Br), mx(mx(A2, B2), Cr)) + 1e-15 * (mx(mx(Ar, Br), mx(A2, B2)) + np.ldexp(s * Ap, -ke))
        er = 7.5 * u * (X2 * Ar + Y2 * Br + Cr) + 1e-15 * np.ldexp(Rp, -ke)
        Th = T / s if mutant == "b" else T / (s * s)
        # eta: 1e-3, or sqrt(rho / 2) up to 0.5 where the error terms are no longer small beside
        # T^ den (rho > 1e-4; den at the box's corner where it is smallest); rescale=False: 1e-3
        dmin = None
        for X, Y, ia, ib, ic, ja, jb, jc in ((X1, Y1, 0, 1, 2, 3, 4, 5), (X2, Y2, 0, 3, 6, 1, 4, 7)):
            part = None
            for sx in (-1.0, 1.0):
                for sy in (-1.0, 1.0):
                    pa = Fh[ia] * (sx * X) + Fh[ib] * (sy * Y) + Fh[ic]
                    pb = Fh[ja] * (sx * X) + Fh[jb] * (sy * Y) + Fh[jc]
                    d = pa * pa + pb * pb
                    part = d if part is None else np.fmin(part, d)
            dmin = part if dmin is None else dmin + part
        rho = (er * er + 4.0 * Th * e * e) / (Th * dmin)
        eta = np.where(rho > 1e-4, np.fmin(0.5, np.sqrt(0.5 * rho)), 1e-3) if rescale else 1e-3 + 0.0 * e
        Alo = Th * (1.0 - 6.0 * u) / ((1.0 + eta) * (1.0 + eta)) * (1.0 - 1e-6)
        b1 = (1.0 + 1.0 / eta) * (er * er + 4.0 * Th * e * e) / (1.0 + eta) * (1.0 + 1e-6)
        Chi = Th * (1.0 + 6.0 * u) / ((1.0 - eta) * (1.0 - eta)) * (1.0 + 1e-6)
        b2 = (er * er / eta + 4.0 * Th * e * e * (1.0 + 1.0 / eta) / (1.0 - eta)) / (1.0 - eta) * (1.0 + 1e-6)
        if mutant == "a":
            Alo = Chi = Th + 0.0 * e
            b1 = b2 = 0.0 * e
        for q in range(9):
            rec[:, q] = Fh[q].astype(np.float32)
        rec[:, 9] = (Alo * (1.0 - 1.2e-7)).astype(np.float32)
        rec[:, 10] = (b1 * (1.0 + 1.2e-7)).astype(np.float32)
        rec[:, 11] = (Chi * (1.0 + 1.2e-7)).astype(np.float32)
        rec[:, 12] = (b2 * (1.0 + 1.2e-7)).astype(np.float32)
    rec[~full] = 0
    rec[~full & valid, 9] = np.nan   # every pair undecided: the f64 test decides
    rec[~full & valid, 11] = np.nan
    rec[~valid, 10] = 1.0            # lo = -1: never an inlier
    rec[~valid, 12] = -1.0           # hi = -1 < r^2 = 0: an outlier
    return rec


def fm_test_f32(rec, x1, y1, x2, y2):
    """fm_test_f32 of records (H, 16) against normalised points (n,) -> (lt, gt), each (H, n)."""
    m = [rec[:, q][:, None] for q in range(13)]
    x1, y1, x2, y2 = (np.asarray(v, np.float32)[None, :] for v in (x1, y1, x2, y2))
    a = fma32(m[0], x1, fma32(m[1], y1, m[2]))
    b = fma32(m[3], x1, fma32(m[4], y1, m[5]))
    c = fma32(m[6], x1, fma32(m[7], y1, m[8]))
    a2 = fma32(m[0], x2, fma32(m[3], y2, m[6]))
    b2 = fma32(m[1], x2, fma32(m[4], y2, m[7]))
    r = fma32(x2, a, fma32(y2, b, c))
    with np.errstate(all="ignore"):
        r2 = r * r
        den = fma32(a, a, fma32(b, b, fma32(a2, a2, b2 * b2)))
        lt = r2 < fma32(m[9], den, -m[10])
        gt = r2 > fma32(m[11], den, m[12])
    return lt, gt


def decide(soa, F, valid, T, mutant=None, rescale=True):
    """The pre-filter's decision of every (model, point) pair: (H, n) int8 of IN / OUT / UNDECIDED.
    soa: the f32 SoA points (pyoracle.soa_hom); F (H, 9) f64; valid (H,); T = thr2 (the f32 value)."""
    lo, hi = fm_bounds(soa)
    fr = fm_frame(lo, hi)
    rec = fm_records(F, valid, fr, T, mutant, rescale)
    with np.errstate(all="ignore"):
        xn = [(np.asarray(soa[k], np.float32) - fr.c[k]) * fr.inv_s for k in range(4)]
    lt, gt = fm_test_f32(rec, *xn)
    # the kernel counts r.lt as an inlier and calls a pair undecided when neither flag is set
    return np.where(lt, IN, np.where(gt, OUT, UNDECIDED)).astype(np.int8)


def exact_masks(soa, F, valid, thr):
    """The f64 decision (orc_fm_count's mask) of every valid model; an invalid model has no inlier."""
    out = np.zeros((len(F), len(soa[0])), bool)
    for h in range(len(F)):
        if valid[h]:
            out[h] = O.fm_count(F[h], soa, thr, mask=True)[1]
    return out


def sampson_ratio(soa, F, T):
    """r^2 / (T den) of every pair in f64 (pixel frame): 1 is the threshold."""
    x1, y1, x2, y2 = (np.asarray(v, np.float64)[None, :] for v in soa)
    f = [np.asarray(F, np.float64).reshape(-1, 9)[:, q][:, None] for q in range(9)]
    with np.errstate(all="ignore"):
        a = f[0] * x1 + f[1] * y1 + f[2]
        b = f[3] * x1 + f[4] * y1 + f[5]
        c = f[6] * x1 + f[7] * y1 + f[8]
        a2 = f[0] * x2 + f[3] * y2 + f[6]
        b2 = f[1] * x2 + f[4] * y2 + f[7]
        r = x2 * a + y2 * b + c
        return r * r / (np.float64(T) * (a * a + b * b + a2 * a2 + b2 * b2))


# ---------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------
def _ladder(pts1, pts2, F, T, first, seed):
    """Move pts2[first:] along the normal of the epipolar line F x1 so that, under F,
    r^2 / den = T (1 + delta), on either side of the line; the sign of delta alternates in pairs, so
    both sides of the threshold get the same number of points.  Two rungs, alternating: delta =
    +-10^U(-5, -2), of which 77 % lies inside the band's +-0.2 % (undecided pairs), and the widened
    rung +-10^U(-2.3, -2), outside the band but within 1 % of the threshold (decided pairs that a
    slightly narrower band would get wrong).  With one rung alone the decided shares stay near
    0.5 % of all pairs: a ladder of a share p of the points reaches p (1 - p)^8 <= 4.3 % of the pairs
    through clean samples, and the three caps of 1 % need about a third of that each."""
    rng = np.random.default_rng(seed)
    m = len(pts1) - first
    low = np.where(np.arange(m) % 2 == 0, -5.0, -2.3)
    delta = np.where((np.arange(m) // 2) % 2 == 0, 1.0, -1.0) * 10.0 ** rng.uniform(low, -2.0, m)
    side = rng.choice([-1.0, 1.0], m)
    x1 = np.c_[pts1[first:], np.ones(m)]
    line = x1 @ F.T                                  # F x1: a b c
    nrm = np.hypot(line[:, 0], line[:, 1])
    nvec = line[:, :2] / nrm[:, None]
    base = pts2[first:].copy()
    r0 = (np.c_[base, np.ones(m)] * line).sum(1)
    t = np.zeros(m)
    for _ in range(20):                              # den depends (weakly) on the moved point
        x2 = np.c_[base + t[:, None] * nvec, np.ones(m)]
        l2 = x2 @ F                                  # F^T x2
        den = line[:, 0] ** 2 + line[:, 1] ** 2 + l2[:, 0] ** 2 + l2[:, 1] ** 2
        t = (side * np.sqrt(T * (1.0 + delta) * den) - r0) / nrm
    out = pts2.copy()
    out[first:] = base + t[:, None] * nvec
    return out


def scene_a(thr):
    """A, the threshold ladder: 3000 exact correspondences and 300 that sit within 1e-5 .. 1e-2
    (relative) of thr^2 under the true F.  (3000 / 3300)^8 = 47 % of the 8-point samples are clean."""
    pr = synth.fundamental_problem(N_A, 0.0, seed=11, noise_px=0.0)
    T = float(O.thr2(thr))
    return pr["pts1"], _ladder(pr["pts1"], pr["pts2"], pr["F"], T, LADDER0, seed=int(thr * 10) + 1)


def _two_views(n, seed, relief, baseline):
    """synth.fundamental_problem's cameras over a tilted plane Z = 80 + 0.3 X + 0.2 Y + relief U(-1, 1);
    the second camera's translation is scaled by `baseline` (0: a pure rotation).  Returns pts1, pts2
    and the unit-norm F of the unscaled translation (with baseline 0 any [e]x H fits: this is one)."""
    rng = np.random.default_rng(seed)
    K = np.array([[1200.0, 0, 960.0], [0, 1200.0, 540.0], [0, 0, 1]])
    X = np.c_[rng.uniform(-30, 30, n), rng.uniform(-20, 20, n), np.zeros(n)]
    X[:, 2] = 80.0 + 0.3 * X[:, 0] + 0.2 * X[:, 1] + relief * rng.uniform(-1, 1, n)
    w = rng.normal(size=3) * 0.08
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R2 = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t2 = np.array([4.0, 0.5, 0.3]) + rng.normal(size=3) * 0.2
    x1 = X @ K.T
    x1 = x1[:, :2] / x1[:, 2:3]
    X2 = X @ R2.T + baseline * t2
    x2 = X2 @ K.T
    x2 = x2[:, :2] / x2[:, 2:3]
    tx = np.array([[0, -t2[2], t2[1]], [t2[2], 0, -t2[0]], [-t2[1], t2[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R2 @ Ki
    return x1, x2, F / np.linalg.norm(F)


# B: name -> (relief, baseline).  On an exact plane (or under a pure rotation) x2 = H x1 for every
# point, every [e]x H is a fundamental matrix of the data, and an 8-point sample picks the epipole e
# from its f32 rounding noise: the models are a three-parameter family.  A moved point at distance
# rho from H x1 then lies rho |sin(angle to e)| from its line, so no ladder sits near the threshold of
# more than a few per cent of such models (the measured shares are in DESIGN.md section 9): the exact
# scenes test soundness and GPU equality on that family.  The "near" scenes keep 0.05 of depth
# relief (0.06 % of the depth; scene A has 80) or 10 % of the baseline, so that the models are an
# ill-conditioned family around one F, and the non-vacuity caps are asserted on those at 60 px,
# where the threshold's 1 % is wider than the family's spread.
SCENES_B = {
    "plane_exact": (0.0, 1.0),
    "rotation_exact": (40.0, 0.0),
    "plane_near": (0.05, 1.0),
    "rotation_near": (40.0, 0.1),
}


def scene_b(name, thr):
    relief, baseline = SCENES_B[name]
    p1, p2, F = _two_views(N_A, 11, relief, baseline)
    return p1, _ladder(p1, p2, F, float(O.thr2(thr)), LADDER0, seed=int(thr * 10) + 2)


COORDS = ("x1", "y1", "x2", "y2")
FAR = (1e6, 1e12, 1e29, 1e31)
NONFINITE = (("pinf", np.inf), ("ninf", -np.inf), ("nan", np.nan))


def _with_point(p1, p2, k, value):
    """One extra point (a copy of point 0) whose coordinate k of x1 y1 x2 y2 holds `value`."""
    q = np.r_[p1[0], p2[0]]
    q[k] = value
    return np.vstack([p1, q[None, :2]]), np.vstack([p2, q[None, 2:]])


def scenes_c():
    """C, the frame edges on scene A at 1.5 px: name -> (pts1, pts2, thr, kind).  kind:
      "finite":   the frame resolves the image; the pre-filter must still filter (< 50 % undecided);
      "coarse":   one far point of 1e12 or 1e29: finite and in range for fm_frame, but an f32 ulp at
                  the frame's centre is wider than the whole image, so every point of the image
                  collapses onto one normalised coordinate (the share is recorded);
      "degenerate": an infinite, NaN or >= 1e30 bound: every valid model's pairs must be undecided."""
    p1, p2 = scene_a(1.5)
    out = {}
    out["offset_2p20"] = (p1 + 2.0 ** 20, p2 + 2.0 ** 20, 1.5, "finite")
    out["image2_x1024"] = (p1, p2 * 1024.0, 1.5, "finite")
    for k, cn in enumerate(COORDS):
        a, b = p1.copy(), p2.copy()
        (a if k < 2 else b)[:, k % 2] = 517.25
        out[f"const_{cn}"] = (a, b, 1.5, "finite")
    out["scale_2p40"] = (p1 * 2.0 ** 40, p2 * 2.0 ** 40, 1.5 * 2.0 ** 40, "finite")
    out["scale_2m40"] = (p1 * 2.0 ** -40, p2 * 2.0 ** -40, 1.5 * 2.0 ** -40, "finite")
    for k, cn in enumerate(COORDS):
        for v in FAR:
            kind = "finite" if v == 1e6 else ("coarse" if v < 1e30 else "degenerate")
            out[f"far_{v:.0e}_{cn}"] = _with_point(p1, p2, k, v) + (1.5, kind)
        for vn, v in NONFINITE:
            out[f"{vn}_{cn}"] = _with_point(p1, p2, k, v) + (1.5, "degenerate")
    return out


THR_D = (1e-30, 1e-6, 1e6, 1e30, 0.0, float("inf"), float("nan"))


def scenes_d():
    """D, the thresholds on scene A's 1.5 px ladder.  thr2 is the f32 of thr^2: 1e-30 and 0 give
    T = 0, 1e30 and inf give T = +inf, NaN gives NaN; the count call takes them all."""
    p1, p2 = scene_a(1.5)
    return {f"thr_{t!r}": (p1, p2, t, "threshold") for t in THR_D}


THR_LADDER = (0.4, 1.5, 60)


@functools.lru_cache(maxsize=None)
def all_scenes():
    """name -> (pts1, pts2, thr, kind), built once per process.  kind: "ladder" (A and the near B
    scenes: the non-vacuity caps hold), "family" (the exact B scenes), then scenes_c's kinds and
    "threshold" (D)."""
    s = {}
    for thr in THR_LADDER:
        s[f"A_{thr}"] = scene_a(thr) + (thr, "ladder")
        for name in SCENES_B:
            s[f"B_{name}_{thr}"] = scene_b(name, thr) + (thr, "ladder" if name.endswith("near") else "family")
    s.update({"C_" + k: v for k, v in scenes_c().items()})
    s.update({"D_" + k: v for k, v in scenes_d().items()})
    return s
