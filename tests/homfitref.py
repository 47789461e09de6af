"""TEST INFRASTRUCTURE -- the homography refit's reference and the restated local-optimisation loop
(DESIGN.md "Homography: least-squares and LM refit and local optimisation on GPU").

fit(soa, mask): the unchanged CPU oracle's orc_hom_refine (findHomography's normalised least-squares
DLT over the masked points, then ten iterations of OpenCV's LMSolver) -> H (3, 3), or None where it
reports no model (fewer than 4 masked points, a zero deviation sum).

local_opt(soa, H, thr, max_rounds): the loop of rsac_homography_local_opt on the oracle's count
rule (pyoracle.hom_count) and fit() above:
    mask_0 = mask of H at thr, c_0 its count
    round k: H_k = fit(mask_{k-1}); mask_k = mask of H_k; accepted iff c_k > c_{k-1}
    at most max_rounds accepted rounds; c < 4 or a fit without a model ends the loop.

The inputs of the fit tests (case) and of the pinned table (INPUTS) come from
rsac.synth.homography_problem at fixed seeds.

Run as a script it prints TABLE.
"""
from __future__ import annotations

import functools

import numpy as np

import pyoracle as O
from rsac import synth

THR = 3.0
MAX_ROUNDS = 4

# (n, outlier ratio, seed, noise px) of synth.homography_problem; the winner is the oracle's RANSAC
# (OpenCV's sampler, 2000 iterations at most, confidence 0.995) at THR
INPUTS = [(40, 0.3, 11, 1.0), (65, 0.4, 12, 1.5), (200, 0.3, 13, 1.0), (300, 0.5, 14, 2.0), (1025, 0.3, 15, 1.0),
          (2000, 0.5, 16, 1.5)]
# key -> (winner's count, count of the H fitted on the winner's mask, count after <= MAX_ROUNDS rounds, rounds)
TABLE = {
    (40, 0.3, 11, 1.0): (23, 27, 28, 2),
    (65, 0.4, 12, 1.5): (29, 32, 32, 1),
    (200, 0.3, 13, 1.0): (120, 137, 137, 1),
    (300, 0.5, 14, 2.0): (83, 91, 100, 4),  # 4 rounds: the cap
    (1025, 0.3, 15, 1.0): (602, 710, 712, 2),
    (2000, 0.5, 16, 1.5): (651, 817, 872, 4),  # the cap
}


def problem(n, outliers, seed, noise=1.0):
    return synth.homography_problem(n, outliers, seed=seed, noise_px=noise)


def soa_of(key):
    pr = problem(*key)
    return O.soa_hom(pr["src"], pr["dst"])


def fit(soa, mask=None):
    """orc_hom_refine -> H (3, 3) or None"""
    n = len(soa[0])
    m = np.ones(n, np.uint8) if mask is None else np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, np.uint8)
    H = np.zeros(9)
    ok = O.lib().orc_hom_refine(*soa, m, n, H)
    return H.reshape(3, 3) if ok else None


def local_opt(soa, H, thr=THR, max_rounds=MAX_ROUNDS, fit_fn=None):
    """the loop of rsac_homography_local_opt -> (H, mask, count, steps); fit_fn(soa, mask) -> H | None"""
    fit_fn = fit_fn or fit
    H = np.asarray(H, np.float64).reshape(3, 3)
    count, mask = O.hom_count(H, soa, thr, mask=True)
    steps = 0
    while steps < max_rounds and count >= 4:
        Hn = fit_fn(soa, mask)
        if Hn is None:
            break
        cn, mn = O.hom_count(Hn, soa, thr, mask=True)
        if not cn > count:
            break
        H, mask, count, steps = Hn, mn, cn, steps + 1
    return H, mask, count, steps


@functools.lru_cache(maxsize=None)
def row(key):
    """-> dict(H0, mask0, c0, H1, c1, lo={cap: (H, mask, count, steps)}) of one input, computed once"""
    pr, soa = problem(*key), soa_of(key)
    w = O.hom_ransac(pr["src"], pr["dst"], THR, refine=False)
    assert w["best"] >= 0
    H0 = w["H"].copy()
    c0, mask0 = O.hom_count(H0, soa, THR, mask=True)
    assert c0 == w["n_inliers"] and np.array_equal(mask0, w["mask"])
    H1 = fit(soa, mask0)
    c1 = O.hom_count(H1, soa, THR)
    return dict(H0=H0, mask0=mask0, c0=c0, H1=H1, c1=c1,
                lo={cap: local_opt(soa, H0, THR, cap) for cap in range(1, MAX_ROUNDS + 1)})


def table_row(key):
    r = row(key)
    _, _, count, steps = r["lo"][MAX_ROUNDS]
    return (r["c0"], r["c1"], count, steps)


# ---------------------------------------------------------------------------
# inputs of the fit tests
# ---------------------------------------------------------------------------
SIZES = [4, 5, 8, 12, 63, 64, 65, 127, 128, 129, 1000, 4097]
NOISES = [0.0, 0.01, 0.5, 3.0]


def _plant(pr, mask, seed):
    """gross errors under the mask: every seventh masked point's dst moves by hundreds of pixels"""
    rng = np.random.default_rng(seed)
    on = np.arange(len(pr["dst"])) if mask is None else np.flatnonzero(mask)
    hit = on[3::7]
    pr["dst"][hit] += rng.uniform(-300.0, 300.0, (len(hit), 2))


@functools.lru_cache(maxsize=None)
def case(m, shape, noise):
    """-> (src, dst, mask or None) with exactly m masked points (shape "ones": no mask; "third":
    every third point dropped; "chunk": points 64 .. 127 masked out, m >= 128).  noise 3: gross
    errors planted under the mask."""
    seed = 1000 + m + {"ones": 0, "third": 5000, "chunk": 9000}[shape]
    if shape == "ones":
        n, mask = m, None
    elif shape == "third":
        n = m
        while int((np.arange(n) % 3 != 0).sum()) < m:
            n += 1
        mask = np.arange(n) % 3 != 0
    else:
        assert m >= 128
        n = m + 64
        mask = np.ones(n, bool)
        mask[64:128] = False
    pr = problem(n, 0.0, seed, noise)
    if noise >= 3.0:
        _plant(pr, mask, seed)
    assert (n if mask is None else int(mask.sum())) == m
    return pr["src"], pr["dst"], mask


def four_ones(n, noise=0.5):
    """exactly four ones: the first two and the last two points"""
    pr = problem(n, 0.0, 2000 + n, noise)
    mask = np.zeros(n, bool)
    mask[[0, 1, n - 2, n - 1]] = True
    return pr["src"], pr["dst"], mask


def three_ones(n):
    src, dst, mask = four_ones(n)
    mask = mask.copy()
    mask[1] = False
    return src, dst, mask


def equal_x(n, which):
    """all points equal in x, in src or in dst: a zero deviation sum"""
    pr = problem(n, 0.0, 3000 + n, 0.5)
    pr[which][:, 0] = pr[which][0, 0]
    return pr["src"], pr["dst"], None


def translation(n=81):
    """a pure translation of integer coordinates: the DLT is exact, the LM stops on the residuals"""
    g = int(np.ceil(np.sqrt(n)))
    src = np.array([[i % g, i // g] for i in range(n)], np.float64) * 8.0
    return src, src + np.array([5.0, -3.0]), None


def debuglog_blocks():
    """the complete blocks of tests/golden/debuglog_homography.json -> [(src, dst, mask)]"""
    import json
    import os
    d = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "debuglog_homography.json")))
    out = []
    for b in [b for b in d["blocks"] if b["complete"]]:
        M = np.array(b["M"])
        pp2 = np.array(b["pp2"])
        hs = np.c_[pp2, np.ones(len(pp2))] @ M.T
        out.append((hs[:, :2] / hs[:, 2:3], np.array(b["p1"], np.float64), np.array(b["mask"], np.uint8)))
    return out


if __name__ == "__main__":  # PYTHONPATH=oracle:code-reproduction-ransac_amd:tests python tests/homfitref.py
    print("# key -> (winner's count, refitted count, count after <= %d rounds, rounds)" % MAX_ROUNDS)
    for key in INPUTS:
        print(f"    {key}: {table_row(key)},", flush=True)
