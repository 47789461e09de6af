"""TEST INFRASTRUCTURE -- what a batched fundamental-matrix call must return, per problem, composed
from the existing CPU chains (DESIGN.md "Batched fundamental matrix").  Nothing is restated here:

  count   pyoracle.fm_ransac                     (the unchanged C oracle's loop)
  msac    fmrobustref.msac
  lmeds   fmrobustref.lmeds
  fit     rsac.fundamental_fit on the host, which tests/test_fm_fit.py ties to fmfitref.fit
  lo      fmfitref.local_opt with that fit

The hypotheses of a problem do not depend on its place in a batch (the Philox draw is
init(seed, 0, h)), so problem p of a batch must equal the chain of its own points.  A fixed budget
(adaptive=False, max_iters = H) scores H hypotheses in one round and scans them with the same
sequential scan, so it is the chain at max_iters = H.

EXPECT pins the chains' results at THR, SEED, CONF, MAX_ITERS: (best, inliers[, cost | median], iters).
"""
from __future__ import annotations

import functools

import numpy as np

import fmfitref as FR
import fmrobustref as RR
import pyoracle as O
import rsac

THR, SEED, CONF, MAX_ITERS = RR.THR, RR.SEED, RR.CONF, RR.MAX_ITERS

EXPECT = {
    (9, 0, 1): dict(count=(0, 9, 1), msac=(0, 9, 319895, 1), lmeds=(4, 8, 0.00020017263886984438)),
    (12, .25, 5): dict(count=(19, 8, 116), msac=(19, 8, 2467535, 116), lmeds=(340, 8, 0.01167016476392746)),
    (64, .3, 2): dict(count=(58, 40, 195), msac=(58, 40, 17282167, 195), lmeds=(58, 45, 0.5995156764984131)),
    (256, .3, 8): dict(count=(88, 155, 253), msac=(179, 152, 75610670, 253), lmeds=(421, 177, 0.6645426750183105)),
    (257, .3, 8): dict(count=(193, 155, 261), msac=(193, 155, 74399477, 261), lmeds=(285, 180, 0.4137086570262909)),
    (300, .5, 4): dict(count=(751, 139, 2000), msac=(751, 139, 111034179, 2000), lmeds=(345, 158, 22.071914672851562)),
    (1025, .3, 6): dict(count=(242, 684, 243), msac=(242, 684, 262826218, 243), lmeds=(242, 709, 0.47623342275619507)),
    (4097, .5, 4): dict(count=(792, 1683, 2000), lmeds=(454, 2143, 19.5234375)),  # (its MSAC and LMedS chains: a minute)
}


def points(key):
    pr = RR.problem(*key)
    return pr["pts1"], pr["pts2"]


def count_of(p1, p2, max_iters=MAX_ITERS, thr=THR):
    """the count rule's chain on any points -> dict(F | None, mask, n_inliers, best, iters)"""
    r = O.fm_ransac(p1, p2, thr, CONF, max_iters, SEED)
    if r["best"] < 0:
        r["F"] = None
    return r


@functools.lru_cache(maxsize=None)
def count(key, max_iters=MAX_ITERS):
    return count_of(*points(key), max_iters=max_iters)


@functools.lru_cache(maxsize=None)
def msac(key, max_iters=MAX_ITERS):
    r = RR.msac_case(*key, max_iters=max_iters)
    return dict(F=r["F"], mask=r["mask"], n_inliers=r["n_inliers"], best=r["best"], iters=r["iters"], cost=r["cost"])


@functools.lru_cache(maxsize=None)
def lmeds(key, n_iters=None):
    r = RR.lmeds_case(*key, n_iters=n_iters)
    return dict(F=r["F"], mask=r["mask"], n_inliers=r["n_inliers"], best=r["best"], iters=r["iters"],
                median=r["median"])


def chain(rule, key, budget=None):
    """budget None: the defaults (adaptive count / MSAC at MAX_ITERS, LMedS' 548 hypotheses); an
    integer: that fixed number of hypotheses"""
    if rule == "lmeds":
        return lmeds(key, budget)
    return (count if rule == "count" else msac)(key, MAX_ITERS if budget is None else budget)


def pinned(rule, key):
    """EXPECT's row in the shape of summary()"""
    return EXPECT[key][rule]


def summary(rule, r):
    if rule == "count":
        return (r["best"], r["n_inliers"], r["iters"])
    if rule == "msac":
        return (r["best"], r["n_inliers"], r["cost"], r["iters"])
    return (r["best"], r["n_inliers"], r["median"])


def host_fit(p1, p2, mask=None):
    return rsac.fundamental_fit(p1, p2, mask)


def local_opt(p1, p2, F, thr=THR, max_rounds=4):
    """fmfitref.local_opt with the host fit -> (F, mask, count, steps)"""
    return FR.local_opt(O.soa_hom(p1, p2), F, thr, max_rounds, lambda soa, m: rsac.fundamental_fit(p1, p2, m))


def bits_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))
