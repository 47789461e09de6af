"""Measurements for DESIGN.md §25 (the calibrated essential-matrix refit and its local optimisation);
raw output to profiles/essential_fit/ (measure.json; the printed lines are measure.log)."""
import ctypes as C
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
from rsac import _lib as L  # noqa: E402
from rsac import synth  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "essential_fit")
os.makedirs(OUT, exist_ok=True)
res = {}
THR = 1.0


def med(v):
    return [statistics.median(v), min(v), max(v)]


def start_of(pr, seed, s=1.0):
    """the true pose perturbed as tests/emfitref.py perturbs it -> E at unit norm"""
    rng = np.random.default_rng(seed)
    w = rng.normal(size=3) * 0.004 * s
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx) @ pr["R"]
    t = pr["t"] + rng.normal(size=3) * 0.15 * s
    E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
    return E / np.linalg.norm(E)


def mask_of(pr, E):
    with np.errstate(invalid="ignore"):
        return rsac.fundamental_errors(pr["pts1"], pr["pts2"], rsac.essential_to_fundamental(E, pr["K"])) <= np.float32(THR * THR)


def refine_events(prs, Es, masks):
    """rsac_essential_refine_batched_device on f32 SoA device points and device masks between two HIP
    events on the call's stream: the uploads of the start models, k_em_refine and the records' copy;
    -> (device ms, wall ms) of 5 timed calls after 2 warm-ups, problems without a model"""
    P = len(prs)
    off = np.zeros(P + 1, np.int64)
    off[1:] = np.cumsum([len(p["pts1"]) for p in prs])
    a = torch.tensor(np.concatenate([p["pts1"] for p in prs]).T.copy(), device="cuda", dtype=torch.float32)
    b = torch.tensor(np.concatenate([p["pts2"] for p in prs]).T.copy(), device="cuda", dtype=torch.float32)
    m = torch.tensor(np.concatenate(masks), device="cuda")
    K = np.ascontiguousarray(np.stack([p["K"].reshape(9) for p in prs]))
    Ein = np.ascontiguousarray(np.stack([E.reshape(9) for E in Es]))
    Eo, st = np.zeros((P, 9)), np.zeros(P, np.int32)
    ctx = L.context(0)
    stream = torch.cuda.current_stream()
    dev, wall = [], []
    for rep in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        with ctx.lock:
            L.check(L.lib().rsac_essential_refine_batched_device(
                ctx.handle, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), off.ctypes.data, P, K.ctypes.data, None,
                C.c_void_p(m.data_ptr()), Ein.ctypes.data, L.F_DEVICE_SOA, Eo.ctypes.data, None, None, None, None,
                st.ctypes.data, C.c_void_p(stream.cuda_stream)))
        e1.record(stream)
        torch.cuda.synchronize()
        if rep >= 2:
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(e0.elapsed_time(e1))
    return dev, wall, int((st != L.OK).sum())


# 1. the refit: P problems of 2000 matches at 50 % outliers, one of 50k; the host refit beside it
for P, n in ((1, 2000), (64, 2000), (256, 2000), (1, 50000)):
    prs = [synth.essential_problem(n, 0.5, 1000 + k) for k in range(P)]
    Es = [start_of(p, k) for k, p in enumerate(prs)]
    masks = [mask_of(p, p["E"]) for p in prs]  # a winner's mask: the true model's at 1 px
    dev, wall, no_model = refine_events(prs, Es, masks)
    host = []
    for rep in range(7):
        t0 = time.perf_counter()
        for p, E, mk in zip(prs[:8], Es, masks):
            rsac.essential_refine(p["pts1"], p["pts2"], p["K"], E, mk)
        if rep >= 2:
            host.append((time.perf_counter() - t0) * 1e3 / min(P, 8))
    key = f"refine_P{P}_n{n}"
    res[key] = dict(device_ms=med(dev), wall_ms=med(wall), host_ms_per_problem=med(host),
                    mean_masked=float(np.mean([mk.sum() for mk in masks])), no_model=no_model)
    print(key, res[key], flush=True)

# 2. one NumPy problem of 2000 matches through the Python call: the host route against device=0
pr = synth.essential_problem(2000, 0.5, 2)
E0 = start_of(pr, 0)
mk = mask_of(pr, pr["E"])
for route, kw in (("host", {}), ("device", dict(device=0))):
    t = []
    for rep in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rsac.essential_refine(pr["pts1"], pr["pts2"], pr["K"], E0, mk, **kw)
        if rep >= 2:
            t.append((time.perf_counter() - t0) * 1e3)
    res[f"numpy_route_{route}"] = dict(ms=med(t), masked=int(mk.sum()))
    print("numpy route", route, res[f"numpy_route_{route}"], flush=True)

# 3. pair verification (§24's table at 1 px): 256 pairs x 2000 matches, adaptive, confidence 0.99, cap
# 2000 samples, device tensors, host clock around the call and a synchronise, 3 timed calls after a warm-up
for ratio in (0.3, 0.5, 0.7):
    prs = [synth.essential_problem(2000, ratio, 1000 + k) for k in range(256)]
    a = [torch.tensor(p["pts1"], device="cuda") for p in prs]
    b = [torch.tensor(p["pts2"], device="cuda") for p in prs]
    true_inl = [int(p["inlier"].sum()) for p in prs]
    for mode in (False, True, "pose", "lo"):
        key = f"batched_{ratio}_{mode}"
        t = []
        for rep in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = rsac.essential_ransac_batched(a, b, prs[0]["K"], THR, max_iters=2000, confidence=0.99, refine=mode)
            torch.cuda.synchronize()
            if rep >= 1:
                t.append((time.perf_counter() - t0) * 1e3)
        # the inliers at 1 px of the E returned (its own F), of which true
        found, hit = [], []
        for r, p in zip(rows, prs):
            inl = mask_of(p, r[0]) if r[0] is not None else np.zeros(len(p["pts1"]), bool)
            found.append(int(inl.sum()))
            hit.append(int((inl & p["inlier"]).sum()))
        res[key] = dict(ms=med(t), mean_found=float(np.mean(found)), mean_true_found=float(np.mean(hit)),
                        mean_true=float(np.mean(true_inl)), no_model=sum(r[0] is None for r in rows),
                        reached=sum(h >= 0.9 * ti for h, ti in zip(hit, true_inl)),
                        mean_mask=float(np.mean([int(r[2]) for r in rows])))
        print(key, res[key], flush=True)

json.dump(res, open(os.path.join(OUT, "measure.json"), "w"), indent=1)
