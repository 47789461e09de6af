"""TEST INFRASTRUCTURE -- the NumPy restatement of MSAC scoring (DESIGN.md "MSAC scoring").

The models, their status and the refit are the unchanged CPU oracle's (pyoracle); the per-point
error is np_ransac.compute_error (the f32 squared reprojection error of the RANSAC test).  On top:

  k = 19 - ilogb(thr2),  q(e) = floor(e 2^k),  Q = q(thr2)
  cost(h) = sum over the points of (q(e) if e <= thr2 else Q)        [-1, count 0 for status <= 0]
  scan: among status > 0 and count > model_points - 1, in index order within the iteration bound,
        a strictly lower cost replaces the best; then niters = RANSACUpdateNumIters(count).

All integers: the sums are exact whatever the order, so every comparison with the GPU is equality.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import np_ransac as NR
import pyoracle as O
from rsac import synth

THR, SEED = 8.0, 0x5EED
# (n, outlier ratio, seed) -> (best, cost, count, iters) at THR, SEED, max_iters 5000, P3P / Philox
TABLE = [
    ((12, .25, 5), (9, 2006129, 9, 12)),
    ((64, .3, 7), (15, 13246324, 45, 16)),
    ((256, .5, 8), (36, 71431219, 128, 71)),
    ((257, .5, 8), (32, 71827312, 129, 70)),
    ((333, .5, 4), (65, 100180454, 167, 70)),
    ((500, .8, 11), (816, 212232958, 100, 2876)),
    ((2000, .4, 3), (6, 460911079, 1200, 33)),
    ((4097, .5, 8), (14, 1115178168, 2049, 71)),
]
# the count rule's winners where MSAC picks another hypothesis (rows 1, 3, 6 of the table)
COUNT_BEST = {0: 1, 2: 15, 5: 549}
BIG = (8200, .5, 9)  # a cost above 2^32: n >= 8193 at Q = 2^19


def shift(thr):
    """k: costs are in units of 2^-k px^2"""
    t2 = float(np.float32(O.thr2(thr)))
    return 19 - int(math.floor(math.log2(t2)))


def q(e, k):
    """floor(e 2^k) of f32 errors as int64 (the scaling is exact)"""
    s = np.ldexp(np.asarray(e, np.float32), k)
    assert s.dtype == np.float32
    return np.floor(s).astype(np.int64)


def point_costs(e, thr):
    """(inlier flags, per-point costs) of f32 squared errors e"""
    k = shift(thr)
    t2 = np.float32(O.thr2(thr))
    Q = int(q(np.array([t2], np.float32), k)[0])
    e = np.asarray(e, np.float32)
    with np.errstate(invalid="ignore"):
        inl = e <= t2  # False for NaN
    c = np.full(e.shape, Q, np.int64)
    c[inl] = q(e[inl], k)
    return inl, c


def errors(R, t, soa, cam):
    X, Y, Z = (a.astype(np.float64) for a in soa[:3])
    return NR.compute_error(R, t, cam, X, Y, Z, soa[3], soa[4])


def costs(models, status, soa, cam, thr, upto=None):
    """-> (costs int64, counts int32) of the model records; (-1, 0) where status <= 0 (or past upto)"""
    H = len(status) if upto is None else min(upto, len(status))
    c = np.full(len(status), -1, np.int64)
    cnt = np.zeros(len(status), np.int32)
    for h in range(H):
        if status[h] <= 0:
            continue
        inl, pc = point_costs(errors(models[h, :9], models[h, 9:12], soa, cam), thr)
        cnt[h] = int(inl.sum())
        c[h] = int(pc.sum())
    return c, cnt


def scan(cost, cnt, status, n, model_points, conf, max_iters):
    """the literal sequential loop -> (best, best cost (-1 none), count of the best, iterations)"""
    niters = max(int(max_iters), 1)
    best, bc, good, i = -1, -1, 0, 0
    while i < niters and i < len(cost):
        if status[i] < 0:
            break
        if status[i] > 0 and cnt[i] > model_points - 1 and (best < 0 or cost[i] < bc):
            best, bc, good = i, int(cost[i]), int(cnt[i])
            niters = O.update_num_iters(conf, (n - good) / n, model_points, niters)
        i += 1
    return best, bc, good, i


def oracle_rows(p3, p2, K, thr, seed, H, hyp0=0, reference_mode=False):
    """the oracle's unchanged models + the restated costs -> (status, counts, costs, models, soa, cam).
    reference_mode: OpenCV's MWC subsets of 5 points solved by EPnP, through the rvec round trip"""
    soa = O.soa_pnp(p3, p2)
    cam = O.cam_from_K(K)
    kw = {}
    if reference_mode:
        subs, sst = O.mwc_subsets(len(soa[0]), H, s=5)
        kw = dict(subsets=subs, sub_status=sst, minimal="epnp5", rvec=True)
    ocnt, status, models = O.pnp_hypotheses(soa, cam, thr, seed, H, hyp0=hyp0, models=True, **kw)
    return status, ocnt, models, soa, cam


def hypotheses(p3, p2, K, thr, seed, H, hyp0=0):
    """-> (status, counts, costs, models); the counts are checked against the oracle's own"""
    status, ocnt, models, soa, cam = oracle_rows(p3, p2, K, thr, seed, H, hyp0)
    c, cnt = costs(models, status, soa, cam, thr)
    assert np.array_equal(cnt[status > 0], ocnt[status > 0])
    return status, cnt, c, models


def ransac(p3, p2, K, thr, seed, max_iters, conf=0.99, refine=True, reference_mode=False):
    """the whole chain of pnp_ransac(score="msac"): hypotheses, cost scan, mask, refit -> dict"""
    status, ocnt, models, soa, cam = oracle_rows(p3, p2, K, thr, seed, max_iters, reference_mode=reference_mode)
    n = len(soa[0])
    k = 5 if reference_mode else 4
    m = 256  # the scan is sequential: cost the hypotheses it can reach, a growing prefix at a time
    while True:
        c, cnt = costs(models, status, soa, cam, thr, upto=m)
        best, bc, good, iters = scan(c, cnt, status, n, k, conf, max_iters)
        if iters <= m or m >= max_iters:
            break
        m *= 2
    out = dict(best=best, cost=bc, n_inliers=good, iters=iters, R=None, t=None, mask=np.zeros(n, bool))
    if best >= 0:
        R, t = models[best, :9].reshape(3, 3).copy(), models[best, 9:12].copy()
        out["mask"] = point_costs(errors(R, t, soa, cam), thr)[0]
        out["R0"], out["t0"] = R, t
        if refine:
            R, t, _ = O.pnp_refine(soa, out["mask"].astype(np.uint8), cam, R, t)
        out["R"], out["t"] = R, t
    return out


@functools.lru_cache(maxsize=None)
def problem(n, outlier_ratio, seed):
    pr = synth.pnp_problem(n, outlier_ratio, seed=seed)
    for v in pr.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return pr


@functools.lru_cache(maxsize=None)
def hypotheses_case(n, outlier_ratio, seed, H, hyp0=0):
    pr = problem(n, outlier_ratio, seed)
    return hypotheses(pr["points3d"], pr["points2d"], pr["K"], THR, SEED, H, hyp0)


@functools.lru_cache(maxsize=None)
def ransac_case(n, outlier_ratio, seed, max_iters=5000, refine=True, reference_mode=False):
    pr = problem(n, outlier_ratio, seed)
    return ransac(pr["points3d"], pr["points2d"], pr["K"], THR, SEED, max_iters, refine=refine,
                  reference_mode=reference_mode)
