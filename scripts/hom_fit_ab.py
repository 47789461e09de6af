"""Timings of the homography refit on the device (DESIGN.md "Homography: least-squares and LM refit
and local optimisation on GPU") on one GPU.

    python scripts/hom_fit_ab.py [--parent-tree DIR] [--out profiles/hom_fit/hom_fit_ab.json]

Per shape, calls interleaved in one loop, 3 warm-ups, then 21 rounds; every figure is the median
[min, max] of the host clock around a call that ends synchronised, in ms:

  loc        rsac.location_search on bench.py's extras.location_search scene (458 locations x 13
             features, 75 px, host arrays)
  10k, 200   homography_ransac on 10 000 points x 50 % / 200 points x 30 % outliers, device tensors,
             with OpenCV's sampler (the default) and with the Philox sampler
  batch      homography_ransac_batched on 64 x 2 000 points x 30 %, host arrays
  sweep      homography_ransac(refine=True) from device tensors at n = 200 .. 100 000 (11 rounds)
  psweep     homography_ransac_batched(refine=True) on 1 .. 128 problems of 12, 200 and 2 000
             points, host arrays (11 rounds)

Per call: refine False / True / "lo"; refine=True both with the host tail (the parent commit's
path: RSAC_DBG_HOM_FIT 1) and with the device fit (2), and by the tree's own policy (0).  The fit
alone: the device fit (homography_fit on device tensors / homography_fit_batched) against the host
twin on the same mask (for the batches a Python loop of host fits, which adds its ctypes calls).

--parent-tree DIR: a built checkout of the parent commit; its calls are timed on the same inputs in
a process of its own, before and after this tree's loop.  Between them this tree runs the parent's
own loop (the calls both trees have, nothing else interleaved) in a third process: what the calls
without refine are compared by, since a call's time depends on what ran before it.  Raw rounds go to the output file; summary
lines are printed.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, ROUNDS, SWEEP_ROUNDS = 3, 21, 11
SINGLES = [("10k x 50%", 10_000, 0.5, 3), ("200 x 30%", 200, 0.3, 5)]
SWEEP = [200, 1000, 4000, 10_000, 40_000, 100_000]
BATCH = (64, 2000, 0.3)
PSWEEP_N, PSWEEP_P = [12, 200, 2000], [1, 2, 4, 8, 16, 32, 64, 128]


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v}


def measure(tree, parent):
    sys.path[:0] = [os.path.join(tree, "code-reproduction-ransac_amd")]
    import numpy as np
    import torch
    import rsac
    from rsac import _lib as L
    from rsac import synth

    if rsac.lib().rsac_device_count() < 1:
        raise RuntimeError("hom_fit_ab: no HIP device visible")
    ctx = L.context(0)

    def mode(m, fn):  # RSAC_DBG_HOM_FIT m around the call (this tree only)
        def run():
            ctx.debug_set(L.DBG_HOM_FIT, m)
            try:
                return fn()
            finally:
                ctx.debug_set(L.DBG_HOM_FIT, 0)
        return run

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    def loop(calls, rounds=ROUNDS):
        ms, last = {k: [] for k in calls}, {}
        for r in range(WARM + rounds):
            for k, fn in calls.items():
                t, last[k] = timed(fn)
                if r >= WARM:
                    ms[k].append(t)
        return {k: stats(v) for k, v in ms.items()}, last

    def variants(calls, name, fn_of_refine, lo=True):
        calls[name] = lambda: fn_of_refine(False)
        calls[name + "_refine"] = lambda: fn_of_refine(True)
        if parent:
            return
        calls[name + "_refine_host"] = mode(1, lambda: fn_of_refine(True))
        calls[name + "_refine_dev"] = mode(2, lambda: fn_of_refine(True))
        if lo:
            calls[name + "_lo"] = lambda: fn_of_refine("lo")

    res = {}
    # the location search of bench.py
    lp = synth.location_problem(seed=0)
    calls = {"loc": lambda: rsac.location_search(lp["pos3d"], lp["pixels"], lp["locations"], 75.0, device=0)}
    if not parent:
        calls["loc_host"] = mode(1, calls["loc"])
        calls["loc_dev"] = mode(2, calls["loc"])
        # the fit alone: 458 twelve-point problems
        prs = [synth.homography_problem(12, 0.2, seed=100 + k, noise_px=2.0) for k in range(len(lp["locations"]))]
        srcs, dsts = [p["src"] for p in prs], [p["dst"] for p in prs]
        masks = [p["inlier"] for p in prs]
        calls["fit"] = lambda: rsac.homography_fit_batched(srcs, dsts, masks)
        calls["fit_host"] = lambda: [rsac.homography_fit(s, d, m) for s, d, m in zip(srcs, dsts, masks)]
    row, last = loop(calls)
    if not parent:
        assert all(np.array_equal(a, b) for a, b in zip(last["fit"], last["fit_host"]))
        assert np.array_equal(last["loc_host"].H, last["loc_dev"].H, equal_nan=True)
    res["loc 458 x 12"] = row
    # single problems from device tensors
    for name, n, outl, seed in SINGLES:
        pr = synth.homography_problem(n, outl, seed=seed)
        ts, td = torch.tensor(pr["src"], device="cuda"), torch.tensor(pr["dst"], device="cuda")
        calls = {}
        for smp in ("opencv", "philox"):
            variants(calls, "ransac_" + smp, lambda rf, smp=smp: rsac.homography_ransac(ts, td, 3.0, sampler=smp, refine=rf,
                                                                                       return_info=True))
        if not parent:
            H0, dmask, info = calls["ransac_opencv"]()
            hmask = dmask.cpu().numpy()
            calls["fit"] = lambda: rsac.homography_fit(ts, td, dmask)
            calls["fit_host"] = lambda: rsac.homography_fit(pr["src"], pr["dst"], hmask)
        row, last = loop(calls)
        info = last["ransac_opencv"][2]
        row["n"], row["inliers"], row["iters"] = n, info.n_inliers, info.iters
        if not parent:
            assert np.array_equal(last["fit"], last["fit_host"])
            assert np.array_equal(last["ransac_opencv_refine_host"][0], last["ransac_opencv_refine_dev"][0])
            li = last["ransac_opencv_lo"][2]
            row["lo_inliers"], row["lo_rounds"] = li.n_inliers, li.lo_improvements
        res[name] = row
    # a batch from host arrays
    P, n, outl = BATCH
    prs = [synth.homography_problem(n, outl, seed=700 + k) for k in range(P)]
    srcs, dsts = [p["src"] for p in prs], [p["dst"] for p in prs]
    calls = {}
    variants(calls, "batched", lambda rf: rsac.homography_ransac_batched(srcs, dsts, 3.0, refine=rf), lo=False)
    if not parent:
        masks = [o[1] for o in calls["batched"]()]
        calls["fit"] = lambda: rsac.homography_fit_batched(srcs, dsts, masks)
        calls["fit_host"] = lambda: [rsac.homography_fit(s, d, m) for s, d, m in zip(srcs, dsts, masks)]
    row, last = loop(calls)
    if not parent:
        assert all(np.array_equal(a, b) for a, b in zip(last["fit"], last["fit_host"]))
        assert all(np.array_equal(a[0], b[0]) for a, b in zip(last["batched_refine_host"], last["batched_refine_dev"]))
    res["batch 64 x 2000"] = row
    # the crossover of the device-input path by size
    if not parent:
        sweep = {}
        for n in SWEEP:
            pr = synth.homography_problem(n, 0.5, seed=40 + n % 97)
            ts, td = torch.tensor(pr["src"], device="cuda"), torch.tensor(pr["dst"], device="cuda")
            calls = {}
            for smp in ("opencv", "philox"):
                fn = lambda smp=smp: rsac.homography_ransac(ts, td, 3.0, sampler=smp, refine=True)  # noqa: E731
                calls[smp + "_host"] = mode(1, fn)
                calls[smp + "_dev"] = mode(2, fn)
            row, last = loop(calls, SWEEP_ROUNDS)
            assert np.array_equal(last["philox_host"][0], last["philox_dev"][0])
            sweep[str(n)] = row
        res["sweep"] = sweep
        # ... and of the batched forms by problem count (host arrays)
        psweep = {}
        for n in PSWEEP_N:
            for P in PSWEEP_P:
                prs = [synth.homography_problem(n, 0.3, seed=900 + k) for k in range(P)]
                srcs, dsts = [p["src"] for p in prs], [p["dst"] for p in prs]
                fn = lambda: rsac.homography_ransac_batched(srcs, dsts, 3.0, refine=True)  # noqa: E731
                row, last = loop({"host": mode(1, fn), "dev": mode(2, fn)}, SWEEP_ROUNDS)
                assert all(np.array_equal(a[0], b[0]) for a, b in zip(last["host"], last["dev"]))
                psweep[f"{P} x {n}"] = row
        res["psweep"] = psweep
    return res


def child(tree):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree], check=True,
                         stdout=subprocess.PIPE, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--worker")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hom_fit", "hom_fit_ab.json"))
    a = ap.parse_args()
    if a.worker:  # the parent commit's tree, in this process
        print(json.dumps(measure(a.worker, True)))
        return
    parent = [child(a.parent_tree)] if a.parent_tree else []
    mine = measure(ROOT, False)
    same_loop = None
    if a.parent_tree:
        same_loop = child(ROOT)  # this tree through the parent's own loop: the calls both trees have
        parent.append(child(a.parent_tree))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"this": mine, "this_parent_loop": same_loop, "parent": parent, "warmups": WARM, "rounds": ROUNDS, "sweep_rounds": SWEEP_ROUNDS}, f,
                  indent=1)

    def fmt(s):
        return "%.3f [%.3f, %.3f]" % (s["median"], s["min"], s["max"])

    for name, row in mine.items():
        if name in ("sweep", "psweep"):
            for n, r in row.items():
                print(f"{name} {n}: " + "  ".join(f"{k} {fmt(v)}" for k, v in r.items()))
            continue
        print(name + ":")
        for k, v in row.items():
            if isinstance(v, dict):
                line = f"  {k:26s} {fmt(v)} ms"
                if parent and k in parent[0][name]:
                    line += "   parent " + " | ".join(fmt(p[name][k]) for p in parent)
                    line += "   this tree in the parent's loop " + fmt(same_loop[name][k])
                print(line)


if __name__ == "__main__":
    main()
