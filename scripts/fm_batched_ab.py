"""Timings of the batched fundamental-matrix calls (DESIGN.md "Batched fundamental matrix") on one GPU.

    python scripts/fm_batched_ab.py [--parent-tree DIR] [--out profiles/fm_batched/fm_batched_ab.json]

The shape: P image pairs of 2000 matches, 30 % outliers, distinct seeds, P in {8, 64, 256}, points
resident on the device as float64 (n, 2) tensors, shapes warmed.  Two modes: adaptive=True and
adaptive=False with max_iters=512, both with refine=True.  Every figure is the median [min, max] of a
host clock around work that ends in a synchronise, in ms.

  batched   fundamental_ransac_batched on the P pairs
  loop      the Python loop of P fundamental_ransac(..., refine=True) calls
  fit_b     fundamental_fit_batched on the winners' masks
  fit_loop  P fundamental_fit calls on the same masks

The calls alternate inside one loop (WARM warm-ups, then ROUNDS rounds), in BLOCKS blocks.
--parent-tree DIR: a built checkout of the parent commit; its loop is timed on the same inputs in a
process of its own before, between and after this tree's blocks (the yardstick: the parent has no
batched call).  Raw rounds go to the output file; one summary per shape is printed, with the spread of
the loop against itself (this tree's and the parent's medians per block).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [8, 64, 256]
MODES = {"adaptive": dict(adaptive=True, max_iters=2000), "fixed512": dict(adaptive=False, max_iters=512)}
N, OUTLIERS, THR = 2000, 0.3, 1.5
WARM, ROUNDS, BLOCKS = 2, 12, 3


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v}


def measure(tree, loop_only):
    sys.path[:0] = [os.path.join(tree, "code-reproduction-ransac_amd")]
    import numpy as np
    import torch
    import rsac
    from rsac import synth

    if rsac.lib().rsac_device_count() < 1:
        raise RuntimeError("fm_batched_ab: no HIP device visible")

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    prs = [synth.fundamental_problem(N, OUTLIERS, seed=1000 + i) for i in range(max(SIZES))]
    t1 = [torch.tensor(p["pts1"], device="cuda") for p in prs]
    t2 = [torch.tensor(p["pts2"], device="cuda") for p in prs]
    res = {}
    for P in SIZES:
        a, b = t1[:P], t2[:P]
        for mode, kw in MODES.items():
            calls = {"loop": lambda: [rsac.fundamental_ransac(a[p], b[p], THR, refine=True, **kw) for p in range(P)]}
            if not loop_only:
                calls["batched"] = lambda: rsac.fundamental_ransac_batched(a, b, THR, refine=True, **kw)
                masks = [r[1] for r in calls["batched"]()]
                calls["fit_b"] = lambda: rsac.fundamental_fit_batched(a, b, masks)
                calls["fit_loop"] = lambda: [rsac.fundamental_fit(a[p], b[p], masks[p]) for p in range(P)]
            ms = {k: [] for k in calls}
            last = {}
            for r in range(WARM + ROUNDS):
                for k, fn in calls.items():
                    t, last[k] = timed(fn)
                    if r >= WARM:
                        ms[k].append(t)
            if not loop_only:  # the same models, masks and fits either way
                for p in range(P):
                    assert np.array_equal(last["loop"][p][0], last["batched"][p][0])
                    assert torch.equal(last["loop"][p][1], last["batched"][p][1])
                    assert np.array_equal(last["fit_b"][p], last["fit_loop"][p])
                    assert np.array_equal(last["fit_b"][p], last["batched"][p][0])
            res[f"P{P}_{mode}"] = {k: stats(v) for k, v in ms.items()}
    return res


def child(tree):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree], check=True,
                         stdout=subprocess.PIPE, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--worker")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_batched", "fm_batched_ab.json"))
    a = ap.parse_args()
    if a.worker:  # the parent commit's tree, in this process: the loop only
        print(json.dumps(measure(a.worker, True)))
        return
    mine, parent = [], []
    for _ in range(BLOCKS):  # parent, this tree, parent, ..., parent: each in a process of its own
        if a.parent_tree:
            parent.append(child(a.parent_tree))
        sub = subprocess.run([sys.executable, os.path.abspath(__file__), "--block"], check=True,
                             stdout=subprocess.PIPE, text=True).stdout
        mine.append(json.loads(sub.strip().splitlines()[-1]))
    if a.parent_tree:
        parent.append(child(a.parent_tree))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"this": mine, "parent": parent, "warmups": WARM, "rounds": ROUNDS, "blocks": BLOCKS}, f, indent=1)

    def pooled(blocks, shape, k):
        v = [x for blk in blocks for x in blk[shape][k]["rounds"]]
        return "%.3f [%.3f, %.3f]" % (statistics.median(v), min(v), max(v)), statistics.median(v)

    for shape in mine[0]:
        print(shape)
        med = {}
        for k in ("batched", "loop", "fit_b", "fit_loop"):
            txt, med[k] = pooled(mine, shape, k)
            print(f"  {k:9s} {txt} ms")
        blocks = [blk[shape]["loop"]["median"] for blk in mine]
        print("  loop medians per block (this tree): " + " ".join("%.3f" % v for v in blocks))
        spread = max(blocks) - min(blocks)
        if parent:
            txt, pm = pooled(parent, shape, "loop")
            pblocks = [blk[shape]["loop"]["median"] for blk in parent]
            print(f"  parent loop {txt} ms; medians per block: " + " ".join("%.3f" % v for v in pblocks))
            spread = max(spread, max(pblocks) - min(pblocks), abs(pm - med["loop"]))
            print("  batched / parent loop = %.3f; margin %.3f ms against a loop spread of %.3f ms" % (
                med["batched"] / pm, pm - med["batched"], spread))
        else:
            print("  batched / loop = %.3f; margin %.3f ms against a loop spread of %.3f ms" % (
                med["batched"] / med["loop"], med["loop"] - med["batched"], spread))


if __name__ == "__main__":
    if "--block" in sys.argv:  # one block of this tree, in a process of its own
        print(json.dumps(measure(ROOT, False)))
    else:
        main()
