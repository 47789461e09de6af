"""Measurements for DESIGN.md §24 (five-point essential matrix against the 7- and 8-point fundamental
matrix); raw output to profiles/essential5/ (measure.json; the printed lines are measure.log)."""
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

OUT = os.path.join(ROOT, "profiles", "essential5")
os.makedirs(OUT, exist_ok=True)
res = {}


def med(v):
    return [statistics.median(v), min(v), max(v)]


def run(mode, p1, p2, K, **kw):
    if mode == "5pt":
        return rsac.essential_ransac(p1, p2, K, 1.5, return_info=True, **kw)[-1]
    return rsac.fundamental_ransac(p1, p2, 1.5, minimal=mode, return_info=True, **kw)[-1]


# 1. solve and score at fixed budgets of 2000 and 100k samples on 2000 points at 50 % outliers (the
# call's own HIP events); exact_only leaves the f32 pre-filter out, as a third row per mode
pr = synth.essential_problem(2000, 0.5, 3)
p1 = torch.tensor(pr["pts1"], device="cuda")
p2 = torch.tensor(pr["pts2"], device="cuda")
for samples in (2000, 100_000):
    for mode in ("8pt", "7pt", "5pt"):
        rows = []
        for rep in range(7):
            info = run(mode, p1, p2, pr["K"], max_iters=samples, adaptive=False, confidence=0.99)
            if rep >= 2:
                rows.append((info.solve_ms, info.score_ms, info.hyps_scored, info.n_inliers))
        key = f"fixed_{samples}_{mode}"
        solve, score = statistics.median(r[0] for r in rows), statistics.median(r[1] for r in rows)
        res[key] = dict(solve_ms=med([r[0] for r in rows]), score_ms=med([r[1] for r in rows]), records=rows[0][2],
                        n_inliers=rows[0][3], solve_ns_per_sample=solve * 1e6 / samples,
                        score_ns_per_sample=score * 1e6 / samples, score_ns_per_record=score * 1e6 / rows[0][2])
        print(key, res[key], flush=True)
# the share of records that hold a model (the probe's status over 2000 samples)
st = rsac.hypotheses("essential", p1, p2, K=pr["K"], n_hyps=2000, reproj_thresh=1.5)[0]
res["records_with_model_of_10"] = float((st > 0).mean() * 10)
print("models per sample", res["records_with_model_of_10"], flush=True)

# 2. batched pair verification: 256 pairs x 2000 matches, equal confidence, adaptive, cap 2000 samples
for ratio in (0.3, 0.5, 0.7):
    prs = [synth.essential_problem(2000, ratio, 1000 + k) for k in range(256)]
    a = [torch.tensor(p["pts1"], device="cuda") for p in prs]
    b = [torch.tensor(p["pts2"], device="cuda") for p in prs]
    true_inl = [int(p["inlier"].sum()) for p in prs]
    for mode in ("8pt", "7pt", "5pt"):
        key = f"batched_{ratio}_{mode}"
        try:
            t = []
            for rep in range(4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if mode == "5pt":
                    rows = rsac.essential_ransac_batched(a, b, prs[0]["K"], 1.5, max_iters=2000, confidence=0.99)
                else:
                    rows = rsac.fundamental_ransac_batched(a, b, 1.5, max_iters=2000, confidence=0.99, minimal=mode)
                torch.cuda.synchronize()
                if rep >= 1:
                    t.append((time.perf_counter() - t0) * 1e3)
            found = [r[2] for r in rows]
            hit = [int((r[1].cpu().numpy().astype(bool) & p["inlier"]).sum()) for r, p in zip(rows, prs)]
            iters = [run(mode, a[k], b[k], prs[k]["K"], max_iters=2000, confidence=0.99).iters for k in range(0, 256, 32)]
            res[key] = dict(ms=med(t), mean_found=float(np.mean(found)), mean_true_found=float(np.mean(hit)),
                            mean_true=float(np.mean(true_inl)), no_model=sum(r[0] is None for r in rows),
                            reached=sum(h >= 0.9 * ti for h, ti in zip(hit, true_inl)), samples_of_8=iters)
        except Exception as e:  # a buffer over the resident budget is a finding, not a crash
            res[key] = dict(error=str(e))
        print(key, res[key], flush=True)

json.dump(res, open(os.path.join(OUT, "measure.json"), "w"), indent=1)
