"""TEST INFRASTRUCTURE -- the NumPy restatement of MSAC scoring for homographies (DESIGN.md "MSAC
scoring for homographies").  Nothing new is restated here; unchanged pieces are composed:

  models, status, subsets : the CPU oracle's (pyoracle.hom_hypotheses(models=True), mwc_subsets(hom=soa))
  e_i                     : lmedsref.hom_err, the f32 squared transfer error in rsac_math.h's order
  per-point cost, scan    : msacref.point_costs / msacref.scan with model_points = 4
  refit                   : pyoracle.hom_refine on the winner's mask (more than 4 points)
  location search         : pyoracle.location_pos2 / location_errors around the chain above

The counts restated from e_i must equal the oracle's own.  All integers: every comparison with the
library is equality.
"""
from __future__ import annotations

import functools

import numpy as np

import lmedsref as LM
import msacref as MS
import pyoracle as O
from rsac import synth

THR, SEED = 8.0, 0x5EED
CONF, MAX_ITERS = 0.995, 2000
# (sampler, (n, outlier ratio, seed)) -> (best, cost, count, iters) at THR, SEED, CONF, MAX_ITERS on
# synth.homography_problem at its default noise
TABLE = [
    (("opencv", (12, .25, 5)), (16, 2086253, 9, 17)),
    (("opencv", (257, .5, 8)), (41, 72111743, 129, 81)),
    (("opencv", (300, .6, 4)), (199, 99646123, 120, 204)),
    (("philox", (256, .5, 8)), (60, 71177970, 128, 82)),
    (("philox", (300, .6, 4)), (155, 99887495, 119, 211)),
]
# the count rule's winners where MSAC picks another hypothesis (rows 1, 3, 4 of the table)
COUNT_BEST = {1: 16, 3: 0, 4: 164}
# the six inputs of the "what it changes" table (both samplers each)
INPUTS = [(12, .25, 5), (13, .2, 3), (64, .3, 7), (256, .5, 8), (257, .5, 8), (300, .6, 4)]
BIG = (8200, .5, 9)  # a cost above 2^32: n >= 8193 at Q = 2^19


def costs(models, status, soa, thr, upto=None):
    """-> (costs int64, counts int32) of the model records; (-1, 0) where status <= 0 (or past upto)"""
    H = len(status) if upto is None else min(upto, len(status))
    c = np.full(len(status), -1, np.int64)
    cnt = np.zeros(len(status), np.int32)
    for h in range(H):
        if status[h] <= 0:
            continue
        inl, pc = MS.point_costs(LM.hom_err(models[h, :9], soa), thr)
        cnt[h] = int(inl.sum())
        c[h] = int(pc.sum())
    return c, cnt


def oracle_rows(soa, thr, H, sampler="opencv", seed=SEED, hyp0=0, subsets=None):
    """the oracle's unchanged (counts, status, models) of hypotheses [hyp0, hyp0 + H)"""
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
    return O.hom_hypotheses(soa, thr, seed, H, hyp0=hyp0, models=True, **kw)


def hypotheses(src, dst, thr, H, sampler="philox", seed=SEED, hyp0=0, subsets=None):
    """-> (status, counts, costs, models); the counts are checked against the oracle's own"""
    soa = O.soa_hom(src, dst)
    ocnt, status, models = oracle_rows(soa, thr, H, sampler, seed, hyp0, subsets)
    c, cnt = costs(models, status, soa, thr)
    assert np.array_equal(cnt[status > 0], ocnt[status > 0])
    return status, cnt, c, models


def ransac_soa(soa, thr, sampler="opencv", seed=SEED, max_iters=MAX_ITERS, conf=CONF, refine=True):
    """the whole chain of homography_ransac(score="msac") on f32 SoA points -> dict; count_best is the
    count rule's winner over the same rows (pyoracle.scan)"""
    n = len(soa[0])
    out = dict(best=-1, cost=-1, n_inliers=0, iters=0, H0=None, H=None, mask=np.zeros(n, bool), count_best=-1,
               tie=False)
    if n == 4:  # findHomography's direct branch: the model of the four points, every point an inlier
        Hm = O.hom_minimal(soa, np.arange(4, dtype=np.int32))
        if Hm is not None:
            out.update(best=0, n_inliers=4, mask=np.ones(4, bool), H0=Hm, H=Hm, count_best=0)
        return out
    ocnt, status, models = oracle_rows(soa, thr, max_iters, sampler, seed)
    m = 256  # the scan is sequential: cost the hypotheses it can reach, a growing prefix at a time
    while True:
        c, cnt = costs(models, status, soa, thr, upto=m)
        best, bc, good, iters = MS.scan(c, cnt, status, n, 4, conf, max_iters)
        if iters <= m or m >= max_iters:
            break
        m *= 2
    assert np.array_equal(cnt[:iters][status[:iters] > 0], ocnt[:iters][status[:iters] > 0])
    cb, cgood, citers = O.scan(ocnt, status, n, 4, conf, max_iters)
    elig = (status[:citers] > 0) & (ocnt[:citers] == cgood)
    out.update(best=best, cost=bc, n_inliers=good, iters=iters, count_best=cb, count_iters=citers,
               tie=bool(cb >= 0 and elig.sum() > 1))
    if best >= 0:
        H0 = models[best, :9].reshape(3, 3).copy()
        out["mask"] = MS.point_costs(LM.hom_err(H0, soa), thr)[0]
        out["H0"] = out["H"] = H0
        if refine and n > 4:
            out["H"] = O.hom_refine(soa, out["mask"].astype(np.uint8), H0)
    return out


def ransac(src, dst, thr, **kw):
    return ransac_soa(O.soa_hom(src, dst), thr, **kw)


def location(pr, thr, conf=CONF, max_iters=MAX_ITERS):
    """location_search(score="msac") restated -> (per-location dicts of ransac_soa, err (L, 2))"""
    pixels = np.asarray(pr["pixels"], np.float64)
    good = (pixels[:, 0] != 0) | (pixels[:, 1] != 0)
    rows, err = [], np.zeros((len(pr["locations"]), 2))
    for l, loc in enumerate(pr["locations"]):
        pos2 = O.location_pos2(np.asarray(pr["pos3d"], np.float64), np.asarray(loc, np.float64))
        r = ransac_soa(O.soa_hom(pos2[good], pixels[good]), thr, "opencv", max_iters=max_iters, conf=conf)
        if r["best"] >= 0:
            err[l] = O.location_errors(pos2[good], pixels[good], np.linalg.inv(r["H"]), r["mask"], thr)
        rows.append(r)
    return rows, err


@functools.lru_cache(maxsize=None)
def problem(n, outlier_ratio, seed):
    return LM.problem(n, outlier_ratio, seed)


@functools.lru_cache(maxsize=None)
def hypotheses_case(n, outlier_ratio, seed, H, sampler="philox", hyp0=0, thr=THR):
    pr = problem(n, outlier_ratio, seed)
    return hypotheses(pr["src"], pr["dst"], thr, H, sampler, SEED, hyp0)


@functools.lru_cache(maxsize=None)
def ransac_case(sampler, n, outlier_ratio, seed, refine=True, thr=THR):
    pr = problem(n, outlier_ratio, seed)
    return ransac(pr["src"], pr["dst"], thr, sampler=sampler, refine=refine)


@functools.lru_cache(maxsize=None)
def location_case(seed, n_locations, thr=75.0):
    pr = synth.location_problem(seed=seed, n_locations=n_locations)
    rows, err = location(pr, thr)
    return pr, rows, err


def what_it_changes():
    """the figures of DESIGN.md's table, re-derived on the CPU"""
    for thr in (3.0, 8.0, 30.0):
        diff = []
        for sampler in ("opencv", "philox"):
            for key in INPUTS:
                r = ransac_case(sampler, *key, refine=False, thr=thr)
                if r["best"] != r["count_best"]:
                    pr = problem(*key)
                    _, st, mdl = oracle_rows(O.soa_hom(pr["src"], pr["dst"]), thr, MAX_ITERS, sampler, SEED)
                    dm = np.linalg.norm(r["H0"] - pr["H"])
                    dc = np.linalg.norm(mdl[r["count_best"], :9].reshape(3, 3) - pr["H"])
                    diff.append((sampler, key, r["best"], r["count_best"], r["n_inliers"], round(dm, 3), round(dc, 3)))
        print(f"thr {thr}: MSAC and count differ on {len(diff)} of 12")
        for d in diff:
            print("   sampler %s input %s: msac %d count %d (msac inliers %d) |H-H*| msac %.3f count %.3f" % d)
    for seed in (0, 1, 2):
        for L in (40, 458):
            pr, rows, err = location_case(seed, L)
            ties = sum(r["tie"] for r in rows)
            moved = sum(r["best"] != r["count_best"] for r in rows)
            last = max(max(r["iters"], r.get("count_iters", 0)) for r in rows)
            cref = [O.find_homography(pr["pixels"], pr["pos3d"], loc, 75.0) for loc in pr["locations"]]
            cerr = np.array([[r["err1"], r["err2"]] for r in cref])
            print(f"location seed {seed} L {L}: ties {ties}, msac != count {moved}, longest scan {last}, "
                  f"best {O.best_location(err)} err2 {err[O.best_location(err), 1]:.3f} "
                  f"(count rule: best {O.best_location(cerr)} err2 {cerr[O.best_location(cerr), 1]:.3f})")


if __name__ == "__main__":  # PYTHONPATH=oracle:code-reproduction-ransac_amd python tests/hmsacref.py
    what_it_changes()
