"""TEST INFRASTRUCTURE -- the NumPy restatement of LMedS homography (DESIGN.md "LMedS homography").

The subsets, the minimal models, their status and the refit are the unchanged CPU oracle's
(pyoracle.mwc_subsets / hom_hypotheses / hom_refine).  On top, restated here:

  e_i    = hom_err in np.float32, rsac_math.h's evaluation order:
           ww = 1 / ((h6 x + h7 y) + 1),  ex = ((h0 x + h1 y) + h2) ww - u,  e = ex ex + ey ey
  key_i  = the bits of e_i as uint32, 0x7FC00000 for a NaN of either sign; s = the sorted keys as f32
  median = f64(s[n/2]) for odd n, f64(s[n/2-1] + s[n/2]) * 0.5 for even n (f32 sum); -1 for status <= 0
  scan   : status < 0 ends it, status 0 is skipped, median < best (f64, strict, best from DBL_MAX) wins
  niters = max(RANSACUpdateNumIters(conf, 0.45, 4, max_iters), 3), or the caller's count
  sigma  = max(2.5 * 1.4826 * (1 + 5 / (n - 4)) * sqrt(median), 0.001);  mask = e <= f32(sigma^2)
  ok     = the mask has >= 4 ones; a 4-point problem is the direct branch (model of its points, mask ones)

Every comparison with the library is equality: both sides are built without FMA contraction.
"""
from __future__ import annotations

import functools
import math
import sys

import numpy as np

import pyoracle as O
from rsac import synth

SEED = 0x5EED
CONF, MAX_ITERS = 0.995, 2000
NAN_KEY = 0x7FC00000
# (n, outlier ratio, seed) -> (best, median, mask ones): synth.homography_problem at its default noise,
# MWC default state, confidence 0.995, max_iters 2000 -> 55 hypotheses, all with status 1
TABLE = [
    ((5, 0.0, 1), (1, 9.313225746154785e-10, 4)),
    ((12, 0.25, 5), (44, 0.8609719276428223, 9)),
    ((64, 0.3, 2), (6, 4.646750450134277, 45)),
    ((65, 0.4, 3), (8, 5.4109978675842285, 39)),
    ((257, 0.3, 8), (46, 3.9766979217529297, 180)),
    ((2049, 0.45, 11), (31, 7.449526309967041, 1128)),
    ((5000, 0.3, 4), (1, 6.055174827575684, 3500)),
]


def hom_err(H, soa):
    """f32 squared transfer errors of the model H (>= 8 f64 entries, rounded to f32) over f32 SoA points"""
    h = np.asarray(H, np.float64).reshape(-1)[:8].astype(np.float32)
    x, y, u, v = (np.asarray(a, np.float32) for a in soa)
    one = np.float32(1)
    with np.errstate(all="ignore"):
        ww = one / ((h[6] * x + h[7] * y) + one)
        ex = ((h[0] * x + h[1] * y) + h[2]) * ww - u
        ey = ((h[3] * x + h[4] * y) + h[5]) * ww - v
        e = ex * ex + ey * ey
    assert e.dtype == np.float32
    return e


def keys(e):
    k = np.asarray(e, np.float32).view(np.uint32).copy()
    k[np.isnan(e)] = NAN_KEY
    return k


def median_of_errors(e):
    """the LMedS median (f64) of f32 errors"""
    s = np.sort(keys(e)).view(np.float32)
    n = len(s)
    with np.errstate(all="ignore"):
        if n & 1:
            return float(np.float64(s[n // 2]))
        return float(np.float64(np.float32(s[n // 2 - 1] + s[n // 2])) * 0.5)


def medians(models, status, soa):
    out = np.full(len(status), -1.0)
    for h in range(len(status)):
        if status[h] > 0:
            out[h] = median_of_errors(hom_err(models[h, :9], soa))
    return out


def scan(status, med, niters):
    """the literal sequential loop -> (best, best median (DBL_MAX: none), hypotheses consumed)"""
    best, bm, i = -1, sys.float_info.max, 0
    while i < niters and i < len(status):
        if status[i] < 0:
            break
        if status[i] > 0 and med[i] < bm:
            best, bm = i, float(med[i])
        i += 1
    return best, bm, i


def num_iters(conf=CONF, max_iters=MAX_ITERS):
    return max(O.update_num_iters(conf, 0.45, 4, max_iters), 3)


def sigma(median, n):
    return max(2.5 * 1.4826 * (1 + 5.0 / (n - 4)) * math.sqrt(median), 0.001)


def thr2(median, n):
    s = sigma(median, n)
    return np.float32(s * s)


def hypotheses(src, dst, H, sampler="opencv", seed=SEED, hyp0=0, subsets=None):
    """-> (status, medians, models, soa) of hypotheses [hyp0, hyp0 + H): the oracle's models, the
    restated medians.  subsets: an explicit (H, 4) table (status 1 where the indices are in range)"""
    soa = O.soa_hom(src, dst)
    n = len(soa[0])
    kw = {}
    if subsets is not None:
        subsets = np.ascontiguousarray(subsets, np.int32)
        ok = ((subsets >= 0) & (subsets < n)).all(axis=1)
        kw = dict(subsets=subsets, sub_status=np.where(ok, 1, -1).astype(np.int8))
    elif sampler == "opencv":
        assert hyp0 == 0
        subs, sst = O.mwc_subsets(n, H, 4, hom=soa)
        kw = dict(subsets=subs, sub_status=sst)
    _, status, models = O.hom_hypotheses(soa, 3.0, seed, H, hyp0=hyp0, models=True, **kw)
    return status, medians(models, status, soa), models, soa


def lmeds(src, dst, conf=CONF, max_iters=MAX_ITERS, n_iters=None, sampler="opencv", seed=SEED, refine=True):
    """the whole chain of homography_lmeds -> dict(best, median, iters, mask, H0 (the winner), H)"""
    soa = O.soa_hom(src, dst)
    n = len(soa[0])
    out = dict(best=-1, median=-1.0, iters=0, mask=np.zeros(n, bool), H0=None, H=None, n_inliers=0)
    if n == 4:  # findHomography's direct branch: the model of the four points in input order
        Hm = O.hom_minimal(soa, np.arange(4, dtype=np.int32))
        if Hm is not None:
            out.update(best=0, median=0.0, mask=np.ones(4, bool), H0=Hm, H=Hm, n_inliers=4)
        return out
    niters = num_iters(conf, max_iters) if n_iters is None else int(n_iters)
    status, med, models, _ = hypotheses(src, dst, niters, sampler, seed)
    best, bm, iters = scan(status, med, niters)
    out.update(iters=iters, status=status, medians=med)
    if best < 0:
        return out
    H0 = models[best, :9].reshape(3, 3).copy()
    with np.errstate(invalid="ignore"):
        mask = hom_err(H0, soa) <= thr2(bm, n)
    if int(mask.sum()) < 4:
        return out
    out.update(best=best, median=bm, mask=mask, H0=H0, H=H0, n_inliers=int(mask.sum()))
    if refine:
        out["H"] = O.hom_refine(soa, mask.astype(np.uint8), H0)
    return out


@functools.lru_cache(maxsize=None)
def problem(n, outlier_ratio, seed):
    pr = synth.homography_problem(n, outlier_ratio, seed=seed)
    for v in pr.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return pr


@functools.lru_cache(maxsize=None)
def hypotheses_case(n, outlier_ratio, seed, H, sampler="opencv", hyp0=0):
    pr = problem(n, outlier_ratio, seed)
    return hypotheses(pr["src"], pr["dst"], H, sampler, SEED, hyp0)


@functools.lru_cache(maxsize=None)
def lmeds_case(n, outlier_ratio, seed, n_iters=None, sampler="opencv", refine=True):
    pr = problem(n, outlier_ratio, seed)
    return lmeds(pr["src"], pr["dst"], n_iters=n_iters, sampler=sampler, refine=refine)
