"""LMedS homography (k_hom_median / k_hom_median_lane) against the RANSAC counter (k_hom_score /
k_hom_score_lane, unchanged from the parent commit) on the same hypothesis records, on one GPU.
DESIGN.md "LMedS homography" cites its output.

  a   one problem, 10k points, 2000 hypotheses (OpenCV sampler, fixed budget): score_ms of each call
      from HIP events (rsac_stats), the two paths interleaved call by call, median / min / max of
      --reps (21) after --warmup (3) calls of each; then the end-to-end ms of homography_lmeds.
  b   458 problems x 12 points x 55 hypotheses (the location search's shape): the same through the
      batched calls and the context's timing (rsac_set_timing / rsac_last_stats).

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


def interleaved(count_call, lmeds_call, reps, warmup):
    for _ in range(warmup):
        count_call()
        lmeds_call()
    cnt, med = [], []
    for _ in range(reps):
        cnt.append(count_call())
        med.append(lmeds_call())
    out = {"reps": reps, "count_score_ms": summary(cnt), "median_score_ms": summary(med)}
    out["ratio"] = out["median_score_ms"]["median"] / out["count_score_ms"]["median"]
    return out


def wall(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ws = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()  # every call returns with its stream synchronised
        ws.append((time.perf_counter() - t) * 1e3)
    return summary(ws)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000)
    ap.add_argument("--hyps", type=int, default=2000)
    ap.add_argument("--problems", type=int, default=458)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {}

    pr = synth.homography_problem(a.points, 0.3, seed=0)
    s, d = pr["src"], pr["dst"]

    def count_a():
        return rsac.homography_ransac(s, d, 3.0, max_iters=a.hyps, adaptive=False, refine=False,
                                      return_info=True)[2].score_ms

    def lmeds_a():
        return rsac.homography_lmeds(s, d, n_iters=a.hyps, refine=False, return_info=True)[2].score_ms
    out["a"] = dict(points=a.points, hyps=a.hyps, **interleaved(count_a, lmeds_a, a.reps, a.warmup))
    out["a"]["lmeds_end_to_end_ms"] = wall(lambda: rsac.homography_lmeds(s, d, n_iters=a.hyps), a.reps, a.warmup)
    out["a"]["lmeds_opencv_iters_end_to_end_ms"] = wall(lambda: rsac.homography_lmeds(s, d), a.reps, a.warmup)
    out["a"]["ransac_end_to_end_ms"] = wall(lambda: rsac.homography_ransac(s, d, 3.0), a.reps, a.warmup)

    probs = [synth.homography_problem(12, 0.25, seed=k) for k in range(1, a.problems + 1)]
    srcs, dsts = [p["src"] for p in probs], [p["dst"] for p in probs]
    ctx = L.context(0)
    ctx.set_timing(True)

    def count_b():
        rsac.homography_ransac_batched(srcs, dsts, 3.0, max_iters=55, adaptive=False, refine=False)
        return ctx.last_stats()["score_ms"]

    def lmeds_b():
        rsac.homography_lmeds_batched(srcs, dsts, refine=False)
        return ctx.last_stats()["score_ms"]
    out["b"] = dict(problems=a.problems, points=12, hyps=55, **interleaved(count_b, lmeds_b, a.reps, a.warmup))
    ctx.set_timing(False)
    out["b"]["lmeds_end_to_end_ms"] = wall(lambda: rsac.homography_lmeds_batched(srcs, dsts), a.reps, a.warmup)
    out["b"]["ransac_end_to_end_ms"] = wall(lambda: rsac.homography_ransac_batched(srcs, dsts, 75.0), a.reps,
                                            a.warmup)
    ok = sum(r[0] is not None for r in rsac.homography_lmeds_batched(srcs, dsts))
    out["b"]["lmeds_models_found"] = ok

    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
