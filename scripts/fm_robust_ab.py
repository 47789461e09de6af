"""A/B of the fundamental matrix's robust scores (k_fm_cost*, k_fm_median*) against the exact count
kernel (k_fm_score<4, 32> / k_fm_score_lane through exact_only=True: the twin that does the same f64
work without the division) on one GPU.  DESIGN.md "MSAC and LMedS for the fundamental matrix" cites
its output.

  Per shape (points, outlier ratio, hypotheses), fixed budget, one round: score_ms (HIP events around
  the scoring kernel, rsac_stats) of the count, cost and median kernels, the three interleaved call
  by call: median and [min, max] of --reps (>= 21) after --warmup.
  Shapes: 10k x 2000; BASELINE config C4 (50k points, 80 % outliers, 3000); 200 x 548 (lane kernels).
  End to end (wall clock of the whole call): fundamental_ransac under both scores and
  fundamental_lmeds, defaults otherwise (adaptive budget), on the 10k problem.

Prints one JSON object; --out FILE also writes it there.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "code-reproduction-ransac_amd"))

import rsac  # noqa: E402
from rsac import synth  # noqa: E402

SHAPES = [("10k_x_2000", 10_000, 0.5, 2000), ("c4_50k_x_3000", 50_000, 0.8, 3000), ("lane_200_x_548", 200, 0.3, 548)]


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def interleaved(calls, reps, warmup):
    """calls: {name: fn -> ms}; every repetition runs each variant once, in order"""
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    xs = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            xs[k].append(fn())
    out = {k: summary(v) for k, v in xs.items()}
    out["reps"] = reps
    return out


def wall(fn):
    def f():
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = max(a.reps, 21)
    out = {}
    for name, n, outl, H in SHAPES:
        pr = synth.fundamental_problem(n, outl, seed=2)
        p1, p2 = pr["pts1"], pr["pts2"]

        def ransac(**kw):
            return lambda: rsac.fundamental_ransac(p1, p2, 1.5, max_iters=H, adaptive=False, return_info=True,
                                                   **kw)[2].score_ms
        r = interleaved({"count_exact": ransac(exact_only=True), "msac": ransac(score="msac"),
                         "lmeds": lambda: rsac.fundamental_lmeds(p1, p2, n_iters=H, return_info=True)[2].score_ms,
                         "count_prefilter": ransac()}, reps, a.warmup)
        r.update(points=n, hyps=H, ratio_msac=r["msac"]["median"] / r["count_exact"]["median"],
                 ratio_lmeds=r["lmeds"]["median"] / r["count_exact"]["median"])
        out[name + "_score_ms"] = r
        if n == 10_000:
            out["end_to_end_ms"] = interleaved(
                {"count": wall(lambda: rsac.fundamental_ransac(p1, p2, 1.5, max_iters=H)),
                 "msac": wall(lambda: rsac.fundamental_ransac(p1, p2, 1.5, max_iters=H, score="msac")),
                 "lmeds": wall(lambda: rsac.fundamental_lmeds(p1, p2, max_iters=H))}, reps, a.warmup)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
