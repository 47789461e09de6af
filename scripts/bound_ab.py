"""Interleaved A/B of librsac builds on one evaluate_range shape (bounded scoring).

    python scripts/bound_ab.py build/ab/a.so build/ab/b.so ... [--points 10000 --outliers 0.5
        --hyps 100000 --rounds 3] [--mode 0|1|2]

As scripts/mf_ab.py: each (round, build) runs in its own process (RSAC_LIB_PATH), in the order
a b c a b c ...  Per run: score_ms (HIP events around the scoring launches, median of --calls
synchronous calls), step_ms (the asynchronous step on one stream, wall time over --steps),
and n1 / S of the last call (0 / 0 on a build without the hooks).  --mode sets RSAC_DBG_BOUND; a
build given as path@mode runs in that mode (the same build forced on and off: a.so@1 a.so@2).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(a):
    sys.path[:0] = [os.path.join(ROOT, "code-reproduction-ransac_amd")]
    import torch
    import rsac
    from rsac import _lib as L
    from rsac import parallel as par
    from rsac import synth
    pr = synth.pnp_problem(a.points, a.outliers, seed=0)
    K = pr["K"]
    ev = par.PnPShard(pr["points2d"], pr["points3d"], K, 30.0, device=0)
    ctx = L.context(0)
    hooks = True
    try:
        ctx.debug_set(L.DBG_BOUND, a.mode)
    except L.RsacError:
        hooks = False  # a build from before the bounded sequence

    def step():
        return rsac.evaluate_range(ev.p2, ev.p3, K, 0, a.hyps, 30.0, with_mask=True, device_result=True)

    t = time.perf_counter()
    while time.perf_counter() - t < 0.5:
        step()
        torch.cuda.synchronize()
    sc = []
    for _ in range(a.calls):
        _, _, info = rsac.evaluate_range(ev.p2, ev.p3, K, 0, a.hyps, 30.0, return_info=True, device=0)
        sc.append(info.score_ms)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        k = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    n1 = ctx.debug_get(L.DBG_BOUND_N1) if hooks else 0
    S = ctx.debug_get(L.DBG_BOUND_SURVIVORS) if hooks else 0
    print(json.dumps({"lib": os.path.basename(os.environ.get("RSAC_LIB_PATH", "")), "mode": a.mode,
                      "score_ms": statistics.median(sc),
                      "step_ms": ms, "n1": n1, "S": S, "key": int(k[0].item())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--points", type=int, default=10_000)
    ap.add_argument("--outliers", type=float, default=0.5)
    ap.add_argument("--hyps", type=int, default=100_000)
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        worker(a)
        return
    res = {lib: [] for lib in a.libs}
    fwd = ["--calls", a.calls, "--steps", a.steps, "--points", a.points, "--outliers", a.outliers, "--hyps", a.hyps]
    for _ in range(a.rounds):
        for lib in a.libs:
            path, _, mode = lib.partition("@")
            env = dict(os.environ, RSAC_LIB_PATH=os.path.abspath(path))
            out = subprocess.run([sys.executable, "-u", __file__, "--worker", "--mode", mode or str(a.mode)] +
                                 [str(x) for x in fwd], env=env,
                                 capture_output=True, text=True, timeout=200)
            if out.returncode != 0:  # a failed run ends the comparison
                print(out.stdout, out.stderr, flush=True)
                sys.exit(out.returncode or 1)
            line = out.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            res[lib].append(json.loads(line))
    keys = {v[0]["key"] for v in res.values()}
    print(f"summary points={a.points} outliers={a.outliers} hyps={a.hyps} mode={a.mode} (median over {a.rounds} "
          f"rounds; min .. max of step_ms); keys agree: {len(keys) == 1}")
    for lib, v in res.items():
        st = [x["step_ms"] for x in v]
        print(f"  {os.path.basename(lib):24s} score_ms {statistics.median(x['score_ms'] for x in v):.4f}  step_ms "
              f"{statistics.median(st):.4f} ({min(st):.4f} .. {max(st):.4f})  n1 {v[-1]['n1']} S {v[-1]['S']}")


if __name__ == "__main__":
    main()
