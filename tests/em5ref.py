"""NumPy f64 reference of the five-point essential matrix and of the scans in sample
units, for tests/test_em5.py (no GPU) and tests/test_em5_gpu.py.

The solver here is deliberately not the library's algorithm: the null space comes from an SVD, the
10 x 20 constraint matrix from polynomial products over exponent dictionaries, the solutions from the
eigenvectors of the 10 x 10 action matrix of multiplication by x (Stewenius' formulation), and each
real solution is then polished by Gauss-Newton steps on the ten constraints in (x, y, z).
"""
import itertools

import numpy as np

import rsac
from rsac import synth

RPS = 10  # records per sample
# (n, outlier ratio, seed, noise in pixels) of synth.essential_problem: the two noise-free inputs the
# issue names, and two with noise and outliers
INPUTS = ((64, 0.0, 2, 0.0), (256, 0.0, 8, 0.0), (200, 0.3, 3, 0.5), (500, 0.5, 4, 0.5))
N_SUBSETS = 300

_problems = {}


def problem(n, ratio, seed, noise=0.5):
    """synth.essential_problem with the points rounded to f32 (what every path of the library sees)"""
    key = (n, ratio, seed, noise)
    if key not in _problems:
        pr = synth.essential_problem(n, ratio, seed, noise)
        pr["pts1"] = pr["pts1"].astype(np.float32).astype(np.float64)
        pr["pts2"] = pr["pts2"].astype(np.float32).astype(np.float64)
        _problems[key] = pr
    return _problems[key]


def subsets(n, count=N_SUBSETS):
    rng = np.random.default_rng(1)
    return [rng.choice(n, 5, replace=False) for _ in range(count)]


# ---------------------------------------------------------------------------
# polynomials in (x, y, z) as {(i, j, k): coefficient}
# ---------------------------------------------------------------------------
def _pmul(a, b):
    out = {}
    for (ea, ca), (eb, cb) in itertools.product(a.items(), b.items()):
        e = (ea[0] + eb[0], ea[1] + eb[1], ea[2] + eb[2])
        out[e] = out.get(e, 0.0) + ca * cb
    return out


def _padd(a, b, sb=1.0):
    out = dict(a)
    for e, c in b.items():
        out[e] = out.get(e, 0.0) + sb * c
    return out


def _pscale(a, s):
    return {e: s * c for e, c in a.items()}


# degree-lexicographic order: the ten cubic monomials, then the basis x^2 xy xz y^2 yz z^2 x y z 1
MONO = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3),
        (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def rays(p, K):
    return np.c_[p, np.ones(len(p))] @ np.linalg.inv(K).T


def null_space(p1, p2, K1, K2):
    q1, q2 = rays(np.asarray(p1, np.float64), K1), rays(np.asarray(p2, np.float64), K2)
    A = np.stack([np.kron(q2[i], q1[i]) for i in range(5)])
    return np.linalg.svd(A)[2][5:9].reshape(4, 3, 3)  # X, Y, Z, W


def constraint_matrix(N):
    E = [[{(1, 0, 0): N[0][i, j], (0, 1, 0): N[1][i, j], (0, 0, 1): N[2][i, j], (0, 0, 0): N[3][i, j]}
          for j in range(3)] for i in range(3)]
    EEt = [[{} for _ in range(3)] for _ in range(3)]
    for i in range(3):
        for k in range(3):
            for m in range(3):
                EEt[i][k] = _padd(EEt[i][k], _pmul(E[i][m], E[k][m]))
    tr = _padd(_padd(EEt[0][0], EEt[1][1]), EEt[2][2])
    rows = []
    for i in range(3):
        for j in range(3):
            p = {}
            for k in range(3):
                p = _padd(p, _pmul(EEt[i][k], E[k][j]))
            rows.append(_padd(_pscale(p, 2.0), _pmul(tr, E[i][j]), -1.0))
    det = _padd(_padd(_pmul(E[0][0], _padd(_pmul(E[1][1], E[2][2]), _pmul(E[1][2], E[2][1]), -1.0)),
                      _pmul(E[0][1], _padd(_pmul(E[1][0], E[2][2]), _pmul(E[1][2], E[2][0]), -1.0)), -1.0),
                _pmul(E[0][2], _padd(_pmul(E[1][0], E[2][1]), _pmul(E[1][1], E[2][0]), -1.0)))
    rows.append(det)
    return np.array([[r.get(m, 0.0) for m in MONO] for r in rows])


def _residual_jacobian(N, s):
    E = s[0] * N[0] + s[1] * N[1] + s[2] * N[2] + N[3]
    G = E @ E.T
    r = np.r_[(2.0 * G @ E - np.trace(G) * E).ravel(), np.linalg.det(E)]
    J = np.zeros((10, 3))
    cof = np.array([[np.linalg.det(np.delete(np.delete(E, i, 0), j, 1)) * (-1) ** (i + j) for j in range(3)]
                    for i in range(3)])
    for v in range(3):
        D = N[v]
        dG = D @ E.T + E @ D.T
        J[:9, v] = (2.0 * (dG @ E + G @ D) - np.trace(dG) * E - np.trace(G) * D).ravel()
        J[9, v] = (cof * D).sum()
    return r, J


def polish(N, s, steps=8):
    s = np.array(s, np.float64)
    for _ in range(steps):
        r, J = _residual_jacobian(N, s)
        s = s - np.linalg.lstsq(J, r, rcond=None)[0]
    return s


def _unit(E):
    return E / np.linalg.norm(E)


def minimal5(p1, p2, K1, K2=None):
    """-> (polished, raw, eigenvalues): the reference's models E (3 x 3, unit norm, one per real
    eigenvalue, in ascending eigenvalue order) after and before the polish, and all ten eigenvalues
    of the action matrix (complex ones included, for the exclusion rule)"""
    K2 = K1 if K2 is None else K2
    N = null_space(p1, p2, K1, K2)
    M = constraint_matrix(N)
    B = np.linalg.solve(M[:, :10], M[:, 10:])
    At = np.zeros((10, 10))
    At[:6] = -B[:6]
    At[6, 0] = At[7, 1] = At[8, 2] = At[9, 6] = 1.0
    w, V = np.linalg.eig(At)
    raw, pol = [], []
    for k in np.argsort(w.real):
        if w[k].imag != 0.0:
            continue
        v = V[:, k].real
        s = v[6:9] / v[9]
        raw.append(_unit(s[0] * N[0] + s[1] * N[1] + s[2] * N[2] + N[3]))
        sp = polish(N, s)
        pol.append(_unit(sp[0] * N[0] + sp[1] * N[1] + sp[2] * N[2] + N[3]))
    return pol, raw, w


def ambiguous(w, rel=1e-6):
    """the issue's exclusion rule on the reference's own eigenvalues: a near-double pair (relative gap
    < rel) or a nearly real complex pair (|imag| < rel relative)"""
    w = list(w)
    for i in range(len(w)):
        if w[i].imag != 0.0 and abs(w[i].imag) < rel * max(1.0, abs(w[i])):
            return True
        for j in range(i):
            if w[i].imag == 0.0 and w[j].imag == 0.0 and abs(w[i] - w[j]) < rel * max(1.0, abs(w[i]), abs(w[j])):
                return True
    return False


def model_distance(A, B):
    """Frobenius distance of two unit-norm matrices up to sign"""
    A, B = np.asarray(A).reshape(3, 3), np.asarray(B).reshape(3, 3)
    return min(np.linalg.norm(A - B), np.linalg.norm(A + B))


def match(models, ref):
    """one-to-one nearest matching -> the list of distances (None when the nearest map is no bijection)"""
    if len(models) != len(ref):
        return None
    near = [int(np.argmin([model_distance(m, r) for r in ref])) for m in models]
    if sorted(near) != list(range(len(ref))):
        return None
    return [model_distance(m, ref[k]) for m, k in zip(models, near)]


# ---------------------------------------------------------------------------
# The scans in sample units (as §23): rows are hypothesis records, RPS per sample; the
# bound niters counts samples and is tested where a sample begins, so a sample is consumed whole;
# status < 0 ends the scan; a record is eligible iff status > 0 and count > 4.  -> (best record or -1,
# samples consumed, inlier count of the best or 0)
# ---------------------------------------------------------------------------
def scan_count(status, counts, n, confidence, max_iters, rps=RPS, model_points=5):
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


def scan_msac(status, counts, costs, n, confidence, max_iters, rps=RPS, model_points=5):
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
