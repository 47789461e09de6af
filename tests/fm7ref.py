"""NumPy f64 reference of the seven-point fundamental matrix and of the scans in
sample units, for tests/test_fm7.py (no GPU) and tests/test_fm7_gpu.py.

The solver here is deliberately not the library's algorithm: the null space comes from an SVD, the
cubic's coefficients from interpolating det at four points, the roots from np.roots.  Only
free_columns restates a piece of the library (the pivot order of its elimination), to name the two
entries of the normalised model whose ratio is the library's root parameter.
"""
import numpy as np

import rsac
from rsac import synth

RPS = 3  # records per sample
# the problems and subsets the issue fixes for the solver checks
INPUTS = ((64, 0.3, 2), (256, 0.3, 8), (2000, 0.5, 3), (2000, 0.7, 4))
N_SUBSETS = 600

_problems = {}


def problem(n, ratio, seed):
    """synth.fundamental_problem with the points rounded to f32 (what every path of the library sees)"""
    key = (n, ratio, seed)
    if key not in _problems:
        pr = synth.fundamental_problem(n, ratio, seed)
        pr["pts1"] = pr["pts1"].astype(np.float32).astype(np.float64)
        pr["pts2"] = pr["pts2"].astype(np.float32).astype(np.float64)
        _problems[key] = pr
    return _problems[key]


def subsets(n, count=N_SUBSETS):
    rng = np.random.default_rng(1)
    return [rng.choice(n, 7, replace=False) for _ in range(count)]


def _normalise(p):
    c = p.mean(axis=0)
    d = np.sqrt(((p - c) ** 2).sum(axis=1)).mean()
    s = np.sqrt(2.0) / d
    T = np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])
    return (p - c) * s, T


def _system(p1, p2):
    q1, T1 = _normalise(p1)
    q2, T2 = _normalise(p2)
    u1, v1, u2, v2 = q1[:, 0], q1[:, 1], q2[:, 0], q2[:, 1]
    A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones(7)], axis=1)
    return A, T1, T2


def minimal7(p1, p2):
    """-> (models, roots3): the reference's models (3 x 3, unit norm, one per real root) and all
    three roots of its cubic (complex ones included, for the near-double-root rule)"""
    A, T1, T2 = _system(np.asarray(p1, np.float64), np.asarray(p2, np.float64))
    Vt = np.linalg.svd(A)[2]
    F1, F2 = Vt[7].reshape(3, 3), Vt[8].reshape(3, 3)
    xs = np.array([-1.0, 0.0, 1.0, 2.0])
    dets = np.array([np.linalg.det(F1 + x * F2) for x in xs])
    coef = np.linalg.solve(np.vander(xs, 4), dets)  # highest power first, as np.roots takes them
    roots = np.roots(coef)
    models = []
    for r in roots:
        if abs(r.imag) < 1e-9 * max(1.0, abs(r)):
            F = T2.T @ (F1 + r.real * F2) @ T1
            models.append(F / np.linalg.norm(F))
    return models, roots


def near_double_root(roots, rel=1e-6):
    r = list(roots)
    return any(abs(r[i] - r[j]) < rel * max(1.0, abs(r[i]), abs(r[j])) for i in range(len(r)) for j in range(i))


def free_columns(p1, p2):
    """The library's elimination order on this sample (full pivoting, first maximum in row-major
    order) -> (perm[7], perm[8], T1, T2): model r of the sample is T2^T (g1 + lambda_r g2) T1 up to
    scale with g1[perm7] = g2[perm8] = 1, g1[perm8] = g2[perm7] = 0, so lambda_r is entry perm8 over
    entry perm7 of the normalised model."""
    A, T1, T2 = _system(np.asarray(p1, np.float64), np.asarray(p2, np.float64))
    perm = list(range(9))
    for r in range(7):
        sub = np.abs(A[r:, r:])
        k = int(np.argmax(sub))  # the first maximum of the flattened (row-major) block
        pr, pc = r + k // sub.shape[1], r + k % sub.shape[1]
        A[[r, pr]] = A[[pr, r]]
        A[:, [r, pc]] = A[:, [pc, r]]
        perm[r], perm[pc] = perm[pc], perm[r]
        for i in range(7):
            if i != r:
                A[i, r:] = A[i, r:] - (A[i, r] * (1.0 / A[r, r])) * A[r, r:]
    return perm[7], perm[8], T1, T2


def root_parameters(models, p1, p2):
    c7, c8, T1, T2 = free_columns(p1, p2)
    out = []
    for F in models:
        G = (np.linalg.inv(T2.T) @ F @ np.linalg.inv(T1)).ravel()
        out.append(G[c8] / G[c7])
    return out


def det3(F):
    F = np.asarray(F, np.float64).reshape(3, 3)
    return (F[0, 0] * (F[1, 1] * F[2, 2] - F[1, 2] * F[2, 1]) - F[0, 1] * (F[1, 0] * F[2, 2] - F[1, 2] * F[2, 0]) +
            F[0, 2] * (F[1, 0] * F[2, 1] - F[1, 1] * F[2, 0]))


# ---------------------------------------------------------------------------
# The scans in sample units: rows are hypothesis records, RPS per sample; the bound
# niters counts samples and is tested where a sample begins, so a sample is consumed whole; status
# < 0 ends the scan; a record is eligible iff status > 0 and count > 6.  -> (best record or -1,
# samples consumed, inlier count of the best or 0)
# ---------------------------------------------------------------------------
def scan_count(status, counts, n, confidence, max_iters, rps=RPS, model_points=7):
    niters, best, good, i = max(int(max_iters), 1), -1, 0, 0
    while i < len(status):
        if i % rps == 0 and i // rps >= niters:
            break
        if status[i] < 0:
            break
        c = int(counts[i])
        if status[i] > 0 and c > max(good, model_points - 1):
            best, good = i, c
            niters = rsac.update_num_iters(confidence, (n - c) / n, model_points, niters)
        i += 1
    return best, i // rps, good


def scan_msac(status, counts, costs, n, confidence, max_iters, rps=RPS, model_points=7):
    niters, best, good, best_cost, i = max(int(max_iters), 1), -1, 0, -1, 0
    while i < len(status):
        if i % rps == 0 and i // rps >= niters:
            break
        if status[i] < 0:
            break
        c = int(counts[i])
        if status[i] > 0 and c > model_points - 1 and (best < 0 or int(costs[i]) < best_cost):
            best, good, best_cost = i, c, int(costs[i])
            niters = rsac.update_num_iters(confidence, (n - c) / n, model_points, niters)
        i += 1
    return best, i // rps, good


def scan_lmeds(status, medians, n_samples, rps=RPS):
    """-> (best record or -1, its median): the lowest median strictly, over n_samples samples"""
    best, best_med = -1, np.finfo(np.float64).max
    for i in range(min(len(status), rps * int(n_samples))):
        if status[i] < 0:
            break
        if status[i] > 0 and medians[i] < best_med:
            best, best_med = i, float(medians[i])
    return best, best_med
