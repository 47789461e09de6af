"""Measurements for DESIGN.md §23 (7-point against 8-point); raw output to profiles/fm7/ (measure.json; the printed lines are measure.log)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "code-reproduction-ransac_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rsac  # noqa: E402
from rsac import synth  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "fm7")
os.makedirs(OUT, exist_ok=True)
res = {}


def med(v):
    return [statistics.median(v), min(v), max(v)]


# 1. solve and score per 100k samples on C4's 50k points (fixed budget; the call's own HIP events)
pr = synth.fundamental_problem(50_000, 0.8, 2)
p1 = torch.tensor(pr["pts1"], device="cuda")
p2 = torch.tensor(pr["pts2"], device="cuda")
for minimal in ("8pt", "7pt"):
    rows = []
    for rep in range(7):
        F, mask, info = rsac.fundamental_ransac(p1, p2, 1.5, max_iters=100_000, adaptive=False, minimal=minimal,
                                                return_info=True)
        if rep >= 2:
            rows.append((info.solve_ms, info.score_ms, info.hyps_scored, info.n_inliers))
    res[f"c4_fixed100k_{minimal}"] = dict(solve_ms=med([r[0] for r in rows]), score_ms=med([r[1] for r in rows]),
                                          records=rows[0][2], n_inliers=rows[0][3],
                                          score_us_per_record=statistics.median(r[1] for r in rows) * 1e3 / rows[0][2])
    print(minimal, res[f"c4_fixed100k_{minimal}"], flush=True)

# 2. batched pair verification: 256 pairs x 2000 matches
for ratio in (0.5, 0.7):
    prs = [synth.fundamental_problem(2000, ratio, 1000 + k) for k in range(256)]
    a = [torch.tensor(p["pts1"], device="cuda") for p in prs]
    b = [torch.tensor(p["pts2"], device="cuda") for p in prs]
    true_inl = [int(p["inlier"].sum()) for p in prs]
    for max_iters in (2000, 20000):
        for minimal in ("8pt", "7pt"):
            key = f"batched_{ratio}_{max_iters}_{minimal}"
            try:
                t = []
                for rep in range(5):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    rows = rsac.fundamental_ransac_batched(a, b, 1.5, max_iters=max_iters, minimal=minimal)
                    torch.cuda.synchronize()
                    if rep >= 1:
                        t.append((time.perf_counter() - t0) * 1e3)
                found = [r[2] for r in rows]
                hit = [int((r[1].cpu().numpy().astype(bool) & p["inlier"]).sum()) for r, p in zip(rows, prs)]
                iters = []
                for k in range(0, 256, 32):  # samples consumed: the single call on 8 of the pairs (same bits)
                    _, _, info = rsac.fundamental_ransac(a[k], b[k], 1.5, max_iters=max_iters, minimal=minimal,
                                                         return_info=True)
                    iters.append(info.iters)
                res[key] = dict(ms=med(t), mean_found=float(np.mean(found)), mean_true_found=float(np.mean(hit)),
                                mean_true=float(np.mean(true_inl)), no_model=sum(r[0] is None for r in rows),
                                reached=sum(h >= 0.9 * ti for h, ti in zip(hit, true_inl)), samples_of_8=iters)
            except Exception as e:  # a buffer over the resident budget is a finding, not a crash
                res[key] = dict(error=str(e))
            print(key, res[key], flush=True)

json.dump(res, open(os.path.join(OUT, "measure.json"), "w"), indent=1)
