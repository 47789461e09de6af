"""TEST INFRASTRUCTURE -- the NumPy restatement of LMedS PnP (DESIGN.md "LMedS PnP").

It only composes what exists:

  models, status  : the unchanged CPU oracle's (msacref.oracle_rows: Philox P3P, or "reference mode",
                    OpenCV's MWC subsets of 5 points solved by EPnP through the rvec round trip)
  e_i             : msacref.errors (np_ransac.compute_error, the f32 squared reprojection error of
                    the RANSAC test)
  keys, median    : lmedsref.keys / lmedsref.median_of_errors;  -1 for status <= 0
  scan            : lmedsref.scan
  niters          = max(RANSACUpdateNumIters(conf, 0.45, k, max_iters), 3), or the caller's count
  sigma           = max(2.5 * 1.4826 * (1 + 5 / (n - k)) * sqrt(median), 0.001);  mask = e <= f32(sigma^2)
  ok              = the mask has >= k ones; n == 4 (5 in reference mode) is the direct branch of
                    pyoracle.pnp_ransac (model of all the points, mask ones, median 0)
  refit           : pyoracle.pnp_refine / pnp_epnp on the mask

with k = model_points = the sample size (4, or 5 in reference mode).  Every comparison with the
library is equality.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import lmedsref as LM
import msacref as MS
import pyoracle as O

SEED = MS.SEED
CONF, MAX_ITERS = 0.99, 2000
# (n, outlier ratio, seed) -> (best, median, mask ones): synth.pnp_problem, SEED, confidence 0.99,
# max_iters 2000.  P3P + Philox: 48 hypotheses
TABLE = [
    ((12, .25, 5), (21, 2.2502903938293457, 9)),
    ((13, .2, 3), (38, 4.354905128479004, 10)),
    ((64, .3, 7), (39, 3.932668685913086, 45)),
    ((65, .4, 3), (42, 20.53937530517578, 39)),
    ((256, .3, 8), (35, 3.1067776679992676, 179)),
    ((257, .3, 8), (13, 3.9352164268493652, 180)),
    ((333, .4, 4), (39, 17.747896194458008, 200)),
    ((513, .3, 6), (11, 8.98501968383789, 358)),  # (358 of the 359 true inliers; every other row: exactly the true set)
    ((2000, .4, 3), (6, 7.209334373474121, 1200)),
    ((4097, .4, 8), (14, 4.423588752746582, 2458)),
]
# reference mode (MWC 5-point EPnP, rvec round trip): 89 hypotheses
TABLE_REF = [
    ((64, .3, 7), (59, 3.6561169624328613, 45)),
    ((333, .4, 4), (64, 7.885807991027832, 200)),
]
# 80 % outliers (one inlier of five points): P3P fits three of its sample's points exactly, the median
# is 0, sigma its floor of 0.001, and the mask has 3 ones < 4: the call has no model
NO_MODEL = (5, .8, 1)


def model_points(reference_mode=False):
    return 5 if reference_mode else 4


def num_iters(conf=CONF, max_iters=MAX_ITERS, k=4):
    return max(O.update_num_iters(conf, 0.45, k, max_iters), 3)


def sigma(median, n, k=4):
    return max(2.5 * 1.4826 * (1 + 5.0 / (n - k)) * math.sqrt(median), 0.001)


def thr2(median, n, k=4):
    s = sigma(median, n, k)
    return np.float32(s * s)


def median_of_pose(model12, soa, cam):
    return LM.median_of_errors(MS.errors(model12[:9], model12[9:12], soa, cam))


def medians(models, status, soa, cam):
    out = np.full(len(status), -1.0)
    for h in range(len(status)):
        if status[h] > 0:
            out[h] = median_of_pose(models[h], soa, cam)
    return out


def hypotheses(p3, p2, K, H, seed=SEED, hyp0=0, reference_mode=False, subsets=None):
    """-> (status, medians, models, soa, cam) of hypotheses [hyp0, hyp0 + H): the oracle's models, the
    restated medians.  subsets: an explicit (H, 4) table, P3P, scored through the rvec round trip
    (status 1 where the indices are in range)"""
    if subsets is not None:
        soa, cam = O.soa_pnp(p3, p2), O.cam_from_K(K)
        subsets = np.ascontiguousarray(subsets, np.int32)
        ok = ((subsets >= 0) & (subsets < len(soa[0]))).all(axis=1)
        _, status, models = O.pnp_hypotheses(soa, cam, MS.THR, seed, H, subsets=subsets,
                                             sub_status=np.where(ok, 1, -1).astype(np.int8), models=True)
    else:
        status, _, models, soa, cam = MS.oracle_rows(p3, p2, K, MS.THR, seed, H, hyp0, reference_mode)
    return status, medians(models, status, soa, cam), models, soa, cam


def lmeds(p3, p2, K, conf=CONF, max_iters=MAX_ITERS, n_iters=None, seed=SEED, refine=True, reference_mode=False):
    """the whole chain of pnp_lmeds -> dict(best, median, iters, n_inliers, mask, R0, t0 (the winner), R, t)"""
    soa = O.soa_pnp(p3, p2)
    n = len(soa[0])
    k = model_points(reference_mode)
    out = dict(best=-1, median=-1.0, iters=0, n_inliers=0, mask=np.zeros(n, bool), R=None, t=None)
    if n == 4 or n == k:  # solvePnPRansac's count == model_points branch
        kw = dict(sampler="opencv", minimal="epnp5") if reference_mode else {}
        d = O.pnp_ransac(p3, p2, K, MS.THR, conf, max_iters, seed, **kw)
        if d["best"] >= 0:
            out.update(best=0, median=0.0, n_inliers=n, mask=np.ones(n, bool), R=d["R"], t=d["t"], R0=d["R"],
                       t0=d["t"])
        return out
    niters = num_iters(conf, max_iters, k) if n_iters is None else int(n_iters)
    status, med, models, soa, cam = hypotheses(p3, p2, K, niters, seed, 0, reference_mode)
    best, bm, iters = LM.scan(status, med, niters)
    out.update(iters=iters, status=status, medians=med)
    if best < 0:
        return out
    R, t = models[best, :9].reshape(3, 3).copy(), models[best, 9:12].copy()
    with np.errstate(invalid="ignore"):
        mask = MS.errors(R, t, soa, cam) <= thr2(bm, n, k)
    ones = int(mask.sum())
    if ones < k:
        return out
    out.update(best=best, median=bm, n_inliers=ones, mask=mask, R0=R, t0=t)
    m8 = mask.astype(np.uint8)
    if refine in ("epnp", "epnp+lm"):
        Re, te = O.pnp_epnp(soa, m8, cam)
        if Re is not None:
            R, t = Re, te
    if refine in (True, "lm", "epnp+lm"):
        R, t, _ = O.pnp_refine(soa, m8, cam, R, t)
    out.update(R=R, t=t)
    return out


problem = MS.problem


@functools.lru_cache(maxsize=None)
def hypotheses_case(n, outlier_ratio, seed, H, hyp0=0, reference_mode=False):
    pr = problem(n, outlier_ratio, seed)
    return hypotheses(pr["points3d"], pr["points2d"], pr["K"], H, SEED, hyp0, reference_mode)


@functools.lru_cache(maxsize=None)
def lmeds_case(n, outlier_ratio, seed, n_iters=None, refine=True, reference_mode=False):
    pr = problem(n, outlier_ratio, seed)
    return lmeds(pr["points3d"], pr["points2d"], pr["K"], n_iters=n_iters, refine=refine,
                 reference_mode=reference_mode)
