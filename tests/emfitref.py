"""TEST INFRASTRUCTURE -- the independent reference of the calibrated essential-matrix refit and the
restatement of its local optimisation.

reference(pts1, pts2, K, K2, mask, R0, t0): minimises the same sum of squared Sampson residuals as
the library, but is not the library's algorithm: scipy.optimize.least_squares (MINPACK "lm" with
finite differences) over another parameterisation -- a rotation vector composed onto the current
rotation (Rodrigues, sin / cos) and a two-dimensional step in the tangent plane of t from numpy's
QR -- restarted from its own result until the cost stops falling.  Pixels are rounded to f32 like
every library path.  reference_pair runs it from both rotations R_a, R_b of the start's
decomposition: the two parameterise +-E, so they share the minimiser, and the distance between
their results is the reference's own error -- the yardstick of the comparisons.

local_opt(...): the loop of rsac_essential_local_opt on the host refit (rsac.essential_refine) and
the f32 squared Sampson errors (rsac.fundamental_errors) against (float)(thr * thr).

cases(): the twelve (input, start) cases of the tests, computed once per process.
"""
from __future__ import annotations

import functools

import numpy as np
from scipy.optimize import least_squares

import rsac
from rsac import synth

THR = 1.0
INPUTS = [(64, .3, 2, .5), (200, .3, 3, .5), (500, .5, 4, .5), (2000, .5, 2, .5), (2000, .7, 5, .5), (2000, .5, 2, 1.0)]
STARTS = [(1.0, 0), (3.0, 1)]  # (scale s, default_rng seed)


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def rodrigues(w):
    th = float(np.linalg.norm(w))
    if th < 1e-300:
        return np.eye(3)
    k = skew(np.asarray(w) / th)
    return np.eye(3) + np.sin(th) * k + (1.0 - np.cos(th)) * (k @ k)


def f32(p):
    return np.asarray(p, np.float64).astype(np.float32).astype(np.float64)


def residuals(F, x1, x2):
    """the Sampson residuals c / sqrt g of F over homogeneous pixels x1, x2 (n, 3)"""
    a = x1 @ F.T
    b = x2 @ F
    c = np.sum(x2 * a, axis=1)
    g = a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2
    return c / np.sqrt(g)


def cost_of(E, pts1, pts2, K, K2, mask):
    """sum of squared Sampson residuals of K2^-T E K^-1 over the masked f32-rounded points"""
    K2 = K if K2 is None else K2
    m = np.ones(len(pts1), bool) if mask is None else np.asarray(mask, bool)
    x1 = np.c_[f32(pts1)[m], np.ones(m.sum())]
    x2 = np.c_[f32(pts2)[m], np.ones(m.sum())]
    F = np.linalg.inv(K2).T @ np.asarray(E).reshape(3, 3) @ np.linalg.inv(K)
    return float(np.sum(residuals(F, x1, x2) ** 2))


def reference(pts1, pts2, K, K2, mask, R0, t0, max_restarts=20):
    """-> (E at unit norm, cost): least_squares restarted until the cost stops falling"""
    K2 = K if K2 is None else K2
    m = np.ones(len(pts1), bool) if mask is None else np.asarray(mask, bool)
    x1 = np.c_[f32(pts1)[m], np.ones(m.sum())]
    x2 = np.c_[f32(pts2)[m], np.ones(m.sum())]
    Ki1, Ki2t = np.linalg.inv(K), np.linalg.inv(K2).T
    R, t = np.array(R0, float), np.array(t0, float) / np.linalg.norm(t0)

    def pose(p, R, t):
        B = np.linalg.qr(t.reshape(3, 1), mode="complete")[0][:, 1:]  # the tangent plane of t
        tn = t + B @ p[3:]
        return rodrigues(p[:3]) @ R, tn / np.linalg.norm(tn)

    def fun(p, R, t):
        Rn, tn = pose(p, R, t)
        return residuals(Ki2t @ skew(tn) @ Rn @ Ki1, x1, x2)

    best = float(np.sum(fun(np.zeros(5), R, t) ** 2))
    for _ in range(max_restarts):
        sol = least_squares(fun, np.zeros(5), args=(R, t), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15,
                            max_nfev=2000)
        c = float(np.sum(sol.fun ** 2))
        if not c < best:
            break
        best = c
        R, t = pose(sol.x, R, t)
    E = skew(t) @ R
    return E / np.linalg.norm(E), best


def decompose(E):
    """-> (R_a, R_b, t): the two rotations and the unit translation of E = [t]x R (numpy's SVD)"""
    U, _, Vt = np.linalg.svd(np.asarray(E).reshape(3, 3))
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, 1, 0], [-1, 0, 0], [0, 0, 1]])
    return U @ W @ Vt, U @ W.T @ Vt, U[:, 2]


def sign_distance(A, B):
    """Frobenius distance of two unit-norm matrices up to sign"""
    A, B = np.asarray(A).reshape(3, 3), np.asarray(B).reshape(3, 3)
    return float(min(np.linalg.norm(A - B), np.linalg.norm(A + B)))


def reference_pair(pts1, pts2, K, K2, mask, E0):
    """-> (E_ref, cost_ref, spread): the reference from both rotations of E0's decomposition; E_ref
    the one of lower cost, spread the distance of the two results up to sign"""
    Ra, Rb, t = decompose(E0)
    Ea, ca = reference(pts1, pts2, K, K2, mask, Ra, t)
    Eb, cb = reference(pts1, pts2, K, K2, mask, Rb, t)
    return (Ea, ca, sign_distance(Ea, Eb)) if ca <= cb else (Eb, cb, sign_distance(Ea, Eb))


def start_of(pr, s, seed):
    """the true pose perturbed: rotation vector N(0,1) 0.004 s, t + N(0,1) 0.15 s -> E at unit norm"""
    rng = np.random.default_rng(seed)
    R = rodrigues(rng.normal(size=3) * 0.004 * s) @ pr["R"]
    t = pr["t"] + rng.normal(size=3) * 0.15 * s
    E = skew(t) @ R
    return E / np.linalg.norm(E)


def mask_of(pts1, pts2, F, thr=THR):
    """the squared-Sampson rule at thr on the f32 errors"""
    with np.errstate(invalid="ignore"):
        return rsac.fundamental_errors(pts1, pts2, F) <= np.float32(thr * thr)


def manifold_residual(E):
    E = np.asarray(E).reshape(3, 3)
    G = E @ E.T
    return float(np.linalg.norm(2.0 * G @ E - np.trace(G) * E))


@functools.lru_cache(maxsize=None)
def problem(key):
    return synth.essential_problem(*key)


@functools.lru_cache(maxsize=None)
def case(key, start):
    """one case -> dict(pr, E0, mask, E, info, E_ref, cost_ref, spread, cost0)"""
    pr = problem(key)
    p1, p2, K = pr["pts1"], pr["pts2"], pr["K"]
    E0 = start_of(pr, *start)
    mask = mask_of(p1, p2, rsac.essential_to_fundamental(E0, K))
    E, info = rsac.essential_refine(p1, p2, K, E0, mask, return_info=True)
    E_ref, cost_ref, spread = reference_pair(p1, p2, K, None, mask, E0)
    return dict(pr=pr, E0=E0, mask=mask, E=E, info=info, E_ref=E_ref, cost_ref=cost_ref, spread=spread,
                cost0=cost_of(E0, p1, p2, K, None, mask))


def cases():
    return [(key, st) for key in INPUTS for st in STARTS]


def local_opt(pts1, pts2, K, E, thr=THR, max_rounds=4, K2=None):
    """the loop of rsac_essential_local_opt -> (E | None, mask, count, steps, counts of every round tried)"""
    n = len(pts1)
    F = rsac.essential_to_fundamental(E, K, K2)
    if F is None:
        return None, np.zeros(n, bool), 0, 0, []
    E = np.asarray(E, np.float64).reshape(3, 3)
    mask = mask_of(pts1, pts2, F, thr)
    count, steps, trail = int(mask.sum()), 0, []
    trail.append(count)
    while steps < max_rounds and count >= 5:
        En, info = rsac.essential_refine(pts1, pts2, K, E, mask, K2=K2, return_info=True)
        if En is None:
            break
        mn = mask_of(pts1, pts2, info.F, thr)
        cn = int(mn.sum())
        trail.append(cn)
        if not cn > count:
            break
        E, mask, count, steps = En, mn, cn, steps + 1
    return E, mask, count, steps, trail
