"""Timings of the least-squares fundamental matrix (DESIGN.md "Fundamental matrix: least-squares
refit and local optimisation") on one GPU.

    python scripts/fm_fit_ab.py [--parent-tree DIR] [--out profiles/fm_fit/fm_fit_ab.json]

Per shape (10k points x 50 % outliers, BASELINE C4's 50k x 80 %, 200 points x 30 %), calls
interleaved in one loop, 3 warm-ups, then 21 rounds; every figure is the median [min, max] of the
host clock around a call that ends synchronised, in ms, inputs resident on the device:

  fit            fundamental_fit on the winner's mask (device mask)
  fit_host       the host twin on the same mask (points and mask already on the host)
  ransac         fundamental_ransac(refine=False)
  ransac_refine  ... refine=True
  ransac_lo      ... refine="lo"

--parent-tree DIR: a built checkout of the parent commit; its fundamental_ransac is timed on the same
inputs in a process of its own (its package and library), before and after this tree's loop, and the
refit's cost (ransac_refine - ransac, and the fit alone) is reported as a share of it.
Raw rounds go to the output file; one summary line per shape is printed.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [("10k x 50%", 10_000, 0.5, 3), ("C4 50k x 80%", 50_000, 0.8, 2), ("200 x 30%", 200, 0.3, 5)]
WARM, ROUNDS = 3, 21


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v}


def measure(tree, only_ransac):
    sys.path[:0] = [os.path.join(tree, "code-reproduction-ransac_amd")]
    import numpy as np
    import torch
    import rsac
    from rsac import synth

    if rsac.lib().rsac_device_count() < 1:
        raise RuntimeError("fm_fit_ab: no HIP device visible")

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    res = {}
    for name, n, outl, seed in SHAPES:
        pr = synth.fundamental_problem(n, outl, seed=seed)
        p1, p2 = pr["pts1"], pr["pts2"]
        t1, t2 = torch.tensor(p1, device="cuda"), torch.tensor(p2, device="cuda")
        calls = {"ransac": lambda: rsac.fundamental_ransac(t1, t2, 1.5, return_info=True)}
        if not only_ransac:
            F0, dmask, info = calls["ransac"]()
            hmask = dmask.cpu().numpy()
            calls["fit"] = lambda: rsac.fundamental_fit(t1, t2, dmask)
            calls["fit_host"] = lambda: rsac.fundamental_fit(p1, p2, hmask)
            calls["ransac_refine"] = lambda: rsac.fundamental_ransac(t1, t2, 1.5, refine=True, return_info=True)
            calls["ransac_lo"] = lambda: rsac.fundamental_ransac(t1, t2, 1.5, refine="lo", return_info=True)
        ms = {k: [] for k in calls}
        last = {}
        for r in range(WARM + ROUNDS):
            for k, fn in calls.items():
                t, last[k] = timed(fn)
                if r >= WARM:
                    ms[k].append(t)
        row = {k: stats(v) for k, v in ms.items()}
        info = last["ransac"][2]
        row["n"], row["winner"], row["inliers"], row["iters"] = n, info.best_hyp, info.n_inliers, info.iters
        if not only_ransac:
            row["lo_inliers"], row["lo_rounds"] = last["ransac_lo"][2].n_inliers, last["ransac_lo"][2].lo_improvements
            assert np.array_equal(last["fit"], last["fit_host"])
        res[name] = row
    return res


def child(tree):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree], check=True,
                         stdout=subprocess.PIPE, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--worker")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_fit", "fm_fit_ab.json"))
    a = ap.parse_args()
    if a.worker:  # the parent commit's tree, in this process: fundamental_ransac only
        print(json.dumps(measure(a.worker, True)))
        return
    parent = [child(a.parent_tree)] if a.parent_tree else []
    mine = measure(ROOT, False)
    if a.parent_tree:
        parent.append(child(a.parent_tree))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"this": mine, "parent": parent, "warmups": WARM, "rounds": ROUNDS}, f, indent=1)

    def fmt(s):
        return "%.3f [%.3f, %.3f]" % (s["median"], s["min"], s["max"])

    for name, row in mine.items():
        print(f"{name}: winner {row['winner']} inliers {row['inliers']} iters {row['iters']} -> lo "
              f"{row['lo_inliers']} in {row['lo_rounds']} rounds")
        for k in ("fit", "fit_host", "ransac", "ransac_refine", "ransac_lo"):
            print(f"  {k:14s} {fmt(row[k])} ms")
        if parent:
            pm = statistics.median([p[name]["ransac"]["median"] for p in parent])
            print("  parent ransac  " + " | ".join(fmt(p[name]["ransac"]) for p in parent) + " ms")
            print("  refit share of the parent's call: fit alone %.1f %%, refine=True - refine=False %.1f %%" % (
                100 * row["fit"]["median"] / pm, 100 * (row["ransac_refine"]["median"] - row["ransac"]["median"]) / pm))


if __name__ == "__main__":
    main()
