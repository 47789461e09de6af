"""A/B of MSAC scoring (score="msac", k_pnp_cost) against the exact count path (score="count",
exact_only=True: k_pnp_score<8, 32>) on one GPU.  DESIGN.md "MSAC scoring" cites its output.

  kernel   C2 shape (10k points, 50 % outliers, 100k hypotheses, fixed budget): score_ms of each
           call from HIP events (rsac_stats), the two paths interleaved call by call, median of
           --reps (>= 20) after --warmup (3) calls of each.
  c2       end-to-end ms of pnp_ransac on the C2 problem, adaptive, refine=False.
  c3       end-to-end ms of pnp_ransac_batched_flat on C3 (1024 problems x 2000 points, 1024
           hypotheses each, fixed budget, refine=False), inputs on the device.

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

import torch  # noqa: E402

import rsac  # noqa: E402
from rsac import synth  # noqa: E402


def med(xs):
    return statistics.median(xs)


def kernel_ratio(p2, p3, K, thr, hyps, reps, warmup):
    def call(msac):
        kw = dict(score="msac") if msac else dict(exact_only=True)
        info = rsac.pnp_ransac(p2, p3, K, hyps, thr, adaptive=False, refine=False, return_info=True, **kw)[3]
        torch.cuda.synchronize()
        return info
    for _ in range(warmup):
        call(False)
        call(True)
    cnt, msac = [], []
    for _ in range(reps):
        cnt.append(call(False).score_ms)
        msac.append(call(True).score_ms)
    a, b = med(cnt), med(msac)
    return {"points": int(p3.shape[0]), "hyps": hyps, "reps": reps, "count_exact_score_ms": a, "msac_score_ms": b,
            "ratio": b / a, "count_exact_score_ms_min_max": [min(cnt), max(cnt)],
            "msac_score_ms_min_max": [min(msac), max(msac)]}


def wall(fn, reps, warm_s=0.3):
    t_end = time.perf_counter() + warm_s
    while True:
        fn()
        torch.cuda.synchronize()
        if time.perf_counter() >= t_end:
            break
    ws = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ws.append((time.perf_counter() - t) * 1e3)
    return med(ws)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000)
    ap.add_argument("--hyps", type=int, default=100_000)
    ap.add_argument("--thr", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--c3-problems", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    pr = synth.pnp_problem(a.points, 0.5, seed=0)
    p2 = torch.from_numpy(pr["points2d"]).to(dev)
    p3 = torch.from_numpy(pr["points3d"]).to(dev)
    K = pr["K"]
    out = {"thr": a.thr, "device": torch.cuda.get_device_name(0)}
    out["kernel"] = kernel_ratio(p2, p3, K, a.thr, a.hyps, max(a.reps, 20), a.warmup)

    # the two interleaved, so that clock ramps and neighbours touch both alike
    def c2(msac):
        kw = dict(score="msac") if msac else dict(exact_only=True)
        return lambda: rsac.pnp_ransac(p2, p3, K, a.hyps, a.thr, adaptive=True, refine=False, **kw)
    i0 = rsac.pnp_ransac(p2, p3, K, a.hyps, a.thr, adaptive=True, refine=False, exact_only=True, return_info=True)[3]
    i1 = rsac.pnp_ransac(p2, p3, K, a.hyps, a.thr, adaptive=True, refine=False, score="msac", return_info=True)[3]
    out["c2_adaptive"] = {"count_exact_ms": wall(c2(False), a.reps), "msac_ms": wall(c2(True), a.reps),
                          "count_exact": {"best": i0.best_hyp, "iters": i0.iters, "n_inliers": i0.n_inliers,
                                          "rounds": i0.rounds},
                          "msac": {"best": i1.best_hyp, "iters": i1.iters, "n_inliers": i1.n_inliers,
                                   "rounds": i1.rounds, "cost": i1.cost}}
    out["c2_adaptive"]["count_exact_ms_again"] = wall(c2(False), a.reps)

    P = a.c3_problems
    probs = [synth.pnp_problem(2000, 0.5, seed=s) for s in range(1, P + 1)]
    off = np.zeros(P + 1, np.int64)
    off[1:] = np.cumsum([len(p["points3d"]) for p in probs])
    q2 = torch.from_numpy(np.concatenate([p["points2d"] for p in probs])).to(dev)
    q3 = torch.from_numpy(np.concatenate([p["points3d"] for p in probs])).to(dev)
    Ks = np.stack([p["K"] for p in probs])

    def c3(msac):
        kw = dict(score="msac") if msac else dict(exact_only=True)
        return lambda: rsac.pnp_ransac_batched_flat(q2, q3, off, Ks, 1024, a.thr, adaptive=False, refine=False, **kw)
    rc = c3(False)()
    rm = c3(True)()
    out["c3_fixed"] = {"problems": P, "count_exact_ms": wall(c3(False), 10), "msac_ms": wall(c3(True), 10),
                       "winners_differ": int(np.count_nonzero(np.any(rc[0] != rm[0], axis=(1, 2)))),
                       "mean_inliers_count": float(rc[3].mean()), "mean_inliers_msac": float(rm[3].mean())}
    out["c3_fixed"]["count_exact_ms_again"] = wall(c3(False), 10)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
