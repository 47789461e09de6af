#!/usr/bin/env python
"""LMedS PnP measurement (DESIGN.md "LMedS PnP"): rsac_stats::score_ms of the median kernel against
the exact count kernel on the same hypotheses, 5 warm-up + 30 timed calls per variant, the variants
alternating in one session; median [min, max] per variant and the ratio of the medians.  Also the
wall time of pnp_lmeds against pnp_ransac(score="msac") at 8 px, for orientation.

    python scripts/pnp_lmeds_ab.py [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "code-reproduction-ransac_amd")]

import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402
from rsac import synth  # noqa: E402

WARM, TIMED = 5, 30


def summary(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)))


def alternate(variants):
    """variants: {name: callable -> figure}; -> {name: summary}"""
    out = {k: [] for k in variants}
    for i in range(WARM + TIMED):
        for k, f in variants.items():
            v = f()
            if i >= WARM:
                out[k].append(v)
    return {k: summary(v) for k, v in out.items()}


def last_score_ms(ctx):
    s = L.Stats()
    L.check(L.lib().rsac_last_stats(ctx.handle, C.byref(s)))
    return s.score_ms


def single(n, H, modes=("rows",)):
    pr = synth.pnp_problem(n, 0.4, seed=3)
    a = (pr["points2d"], pr["points3d"], pr["K"])
    ctx = L.context(0)

    def lmeds(budget):
        def f():
            ctx.debug_set(L.DBG_LMEDS_KEYS, budget)
            try:
                return rsac.pnp_lmeds(*a, n_iters=H, refine=False, return_info=True)[3].score_ms
            finally:
                ctx.debug_set(L.DBG_LMEDS_KEYS, 0)
        return f

    def count():
        return rsac.pnp_ransac(*a, H, 8.0, adaptive=False, refine=False, exact_only=True, return_info=True)[3].score_ms

    v = {"count_exact": count}
    for m in modes:
        v["median_" + m] = lmeds(0 if m == "rows" else -1)
    res = alternate(v)
    for m in modes:
        res["ratio_" + m] = res["median_" + m]["median"] / res["count_exact"]["median"]
    return res


def batch(P, n, H):
    pr = synth.pnp_problem(n, 0.25, seed=5)
    Ks = []
    for i in range(P):
        K = np.array(pr["K"])
        K[0, 0] *= 0.7 + 0.025 * i
        K[1, 1] *= 0.7 + 0.025 * i
        Ks.append(K)
    p2, p3 = [pr["points2d"]] * P, [pr["points3d"]] * P
    ctx = L.context(0)
    L.check(L.lib().rsac_set_timing(ctx.handle, 1))
    try:
        def lmeds():
            rsac.pnp_lmeds_batched(p2, p3, Ks, n_iters=H, refine=False)
            return last_score_ms(ctx)

        def count():
            rsac.pnp_ransac_batched(p2, p3, Ks, H, 8.0, adaptive=False, refine=False)
            return last_score_ms(ctx)

        res = alternate({"count_exact": count, "median": lmeds})
    finally:
        L.check(L.lib().rsac_set_timing(ctx.handle, 0))
    res["ratio"] = res["median"]["median"] / res["count_exact"]["median"]
    return res


def wall():
    pr = synth.pnp_problem(10000, 0.4, seed=3)
    a = (pr["points2d"], pr["points3d"], pr["K"])

    def timed(f):
        def g():
            t0 = time.perf_counter()
            f()
            return (time.perf_counter() - t0) * 1e3
        return g

    return alternate({"pnp_lmeds": timed(lambda: rsac.pnp_lmeds(*a)),
                      "pnp_ransac_msac_8px": timed(lambda: rsac.pnp_ransac(*a, 5000, 8.0, score="msac"))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    res = {"score_ms_10000x2000": single(10000, 2000), "score_ms_10000x48": single(10000, 48),
           "score_ms_100000x48": single(100000, 48, ("rows", "recompute")),
           "score_ms_27x12x48": batch(27, 12, 48), "wall_ms_10000": wall()}
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
