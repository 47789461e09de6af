"""A/B of MSAC scoring for homographies (score="msac": k_hom_cost, k_hom_cost_lane) against the count
path (k_hom_score, k_hom_score_lane) on one GPU.  DESIGN.md "MSAC scoring for homographies" cites its
output.

  a  one problem of --points (10k) correspondences, --hyps (2000) hypotheses, fixed budget: score_ms
     (HIP events around the scoring kernel, rsac_stats) of k_hom_score and k_hom_cost<8, 32>.
  b  --problems (458) problems of 12 points, 256 hypotheses each, fixed budget, at 75 px (the location
     search's shape): score_ms of k_hom_score_lane and k_hom_cost_lane through the batched call and
     the context's timing (rsac_set_timing / rsac_last_stats).
  The two paths are interleaved call by call: median and [min, max] of --reps (>= 21) after --warmup.
  End to end (wall clock of the whole call, not gated): homography_ransac and location_search under
  both scores, defaults otherwise (adaptive, refit).

Prints one JSON object; --out FILE also writes it there.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "code-reproduction-ransac_amd"))

import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402
from rsac import synth  # noqa: E402


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def interleaved(count_call, msac_call, reps, warmup):
    for _ in range(warmup):
        count_call()
        msac_call()
    cnt, ms = [], []
    for _ in range(reps):
        cnt.append(count_call())
        ms.append(msac_call())
    out = {"reps": reps, "count": summary(cnt), "msac": summary(ms)}
    out["ratio"] = out["msac"]["median"] / out["count"]["median"]
    return out


def wall_pair(count_fn, msac_fn, reps, warmup):
    """wall-clock ms of the two calls, interleaved (every call returns with its stream synchronised)"""
    def t(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3
    return interleaved(lambda: t(count_fn), lambda: t(msac_fn), reps, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000)
    ap.add_argument("--hyps", type=int, default=2000)
    ap.add_argument("--problems", type=int, default=458)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = max(a.reps, 21)
    out = {}

    pr = synth.homography_problem(a.points, 0.3, seed=0)
    s, d = pr["src"], pr["dst"]

    def score_a(score):
        return lambda: rsac.homography_ransac(s, d, 3.0, max_iters=a.hyps, adaptive=False, refine=False,
                                              return_info=True, score=score)[2].score_ms
    out["a_score_ms"] = dict(points=a.points, hyps=a.hyps, **interleaved(score_a("count"), score_a("msac"), reps,
                                                                         a.warmup))
    out["a_end_to_end_ms"] = wall_pair(lambda: rsac.homography_ransac(s, d, 3.0),
                                       lambda: rsac.homography_ransac(s, d, 3.0, score="msac"), reps, a.warmup)

    probs = [synth.homography_problem(12, 0.25, seed=k) for k in range(1, a.problems + 1)]
    srcs, dsts = [p["src"] for p in probs], [p["dst"] for p in probs]
    ctx = L.context(0)
    ctx.set_timing(True)

    def score_b(score):
        def f():
            rsac.homography_ransac_batched(srcs, dsts, 75.0, max_iters=256, adaptive=False, refine=False, score=score)
            return ctx.last_stats()["score_ms"]
        return f
    out["b_score_ms"] = dict(problems=a.problems, points=12, hyps=256,
                             **interleaved(score_b("count"), score_b("msac"), reps, a.warmup))
    ctx.set_timing(False)

    lp = synth.location_problem(n_locations=a.problems)
    loc = (lp["pos3d"], lp["pixels"], lp["locations"], 75.0)
    out["location_search_end_to_end_ms"] = wall_pair(lambda: rsac.location_search(*loc),
                                                     lambda: rsac.location_search(*loc, score="msac"), reps, a.warmup)
    rc, rm = rsac.location_search(*loc), rsac.location_search(*loc, score="msac")
    out["location_search_end_to_end_ms"].update(
        locations=a.problems, best_count=rc.best, best_msac=rm.best,
        masks_differ=int(np.count_nonzero(np.any(rc.mask != rm.mask, axis=1))))

    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
