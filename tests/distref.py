"""Helper of test_distortion*.py (TEST INFRASTRUCTURE, not a test): NumPy restatements of the lens
distortion contract (DESIGN.md "Lens distortion") and the reference chain built on the unchanged
CPU oracle.

The two sequences are element-wise float64 ufuncs applied in the contract's order, so nothing is
fused; astype(np.float32) stands where the contract rounds.  kd = (k1, k2, p1, p2, k3, k4, k5, k6),
missing entries zero; the rational factor is present exactly when 8 coefficients were passed.
"""
import functools

import numpy as np

import pyoracle as O
from rsac import synth

D5 = (-0.28, 0.09, 0.0008, -0.0005, -0.01)
D8 = (0.12, -0.05, 0.0008, -0.0005, 0.01, 0.3, -0.02, 0.004)


def kd8(dist):
    d = np.zeros(8)
    dist = np.asarray(dist, np.float64).reshape(-1)
    assert dist.size in (4, 5, 8)
    d[:dist.size] = dist
    return d, dist.size == 8


def project(R, t, cam, dist, X, Y, Z):
    """cvProjectPoints2's sequence on float64 arrays X, Y, Z -> (pu, pv) float64"""
    kd, rational = kd8(dist)
    k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(v) for v in kd)
    R = np.asarray(R, np.float64).reshape(9)
    t = np.asarray(t, np.float64).reshape(3)
    fx, fy, cx, cy = (np.float64(v) for v in cam)
    X, Y, Z = (np.asarray(a, np.float64) for a in (X, Y, Z))
    with np.errstate(all="ignore"):
        x = R[0] * X + R[1] * Y; x = x + R[2] * Z; x = x + t[0]
        y = R[3] * X + R[4] * Y; y = y + R[5] * Z; y = y + t[1]
        z = R[6] * X + R[7] * Y; z = z + R[8] * Z; z = z + t[2]
        iz = np.where(z != 0.0, 1.0 / z, 1.0)
        x = x * iz
        y = y * iz
        r2 = x * x + y * y
        r4 = r2 * r2
        r6 = r4 * r2
        a1 = 2.0 * x * y
        a2 = r2 + 2.0 * x * x
        a3 = r2 + 2.0 * y * y
        cdist = 1.0 + k1 * r2 + k2 * r4 + k3 * r6
        if rational:
            icdist2 = 1.0 / (1.0 + k4 * r2 + k5 * r4 + k6 * r6)
            xd = x * cdist * icdist2 + p1 * a1 + p2 * a2
            yd = y * cdist * icdist2 + p1 * a3 + p2 * a1
        else:
            xd = x * cdist + p1 * a1 + p2 * a2
            yd = y * cdist + p1 * a3 + p2 * a1
        pu = xd * fx + cx
        pv = yd * fy + cy
    return pu, pv


def err2(R, t, cam, dist, soa):
    """the RANSAC test's float32 squared error of every point of the f32 SoA (X, Y, Z, U, V)"""
    X, Y, Z, U, V = soa
    pu, pv = project(R, t, cam, dist, X.astype(np.float64), Y.astype(np.float64), Z.astype(np.float64))
    with np.errstate(all="ignore"):
        dx = U - pu.astype(np.float32)
        dy = V - pv.astype(np.float32)
        e1 = dx * dx
        e2 = dy * dy
        e = e1 + e2
    assert e.dtype == np.float32
    return e


def reproj(R, t, cam, dist, p3, p2):
    """f64 projection and L2 error of f64 AoS points (no rounding) -> (proj n x 2, err n)"""
    p3 = np.asarray(p3, np.float64).reshape(-1, 3)
    p2 = np.asarray(p2, np.float64).reshape(-1, 2)
    pu, pv = project(R, t, cam, dist, p3[:, 0], p3[:, 1], p3[:, 2])
    with np.errstate(all="ignore"):
        dx = p2[:, 0] - pu
        dy = p2[:, 1] - pv
        e = np.sqrt(dx * dx + dy * dy)
    return np.stack([pu, pv], axis=1), e


def undistort(cam, dist, u, v):
    """cvUndistortPoints' five rounds on float64 arrays u, v (the f32-rounded pixels)
    -> (x, y, took_exit): took_exit marks the points a negative icd sent back to (x0, y0)"""
    kd, _ = kd8(dist)
    k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(v_) for v_ in kd)
    fx, fy, cx, cy = (np.float64(v_) for v_ in cam)
    u = np.asarray(u, np.float64)
    v = np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        ifx = 1.0 / fx
        ify = 1.0 / fy
        x0 = (u - cx) * ifx
        y0 = (v - cy) * ify
        x = x0.copy()
        y = y0.copy()
        stop = np.zeros(x.shape, bool)
        for _ in range(5):
            r2 = x * x + y * y
            icd = (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            dX = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            dY = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            xn = (x0 - dX) * icd
            yn = (y0 - dY) * icd
            stop = stop | (icd < 0.0)
            x = np.where(stop, x0, xn)
            y = np.where(stop, y0, yn)
    return x, y, stop


def ideal_pixels(cam, dist, u, v):
    """(Uu, Vu) float32: the ideal pixels the minimal solvers and the refit read"""
    fx, fy, cx, cy = (np.float64(v_) for v_ in cam)
    x, y, _ = undistort(cam, dist, u, v)
    return (x * fx + cx).astype(np.float32), (y * fy + cy).astype(np.float32)


def soa_pair(p3, p2, K, dist):
    """soa = the oracle's f32 SoA of the raw points; soa_i = the same with U, V replaced by the
    restated ideal pixels"""
    soa = O.soa_pnp(p3, p2)
    cam = O.cam_from_K(K)
    Uu, Vu = ideal_pixels(cam, dist, soa[3].astype(np.float64), soa[4].astype(np.float64))
    return soa, soa[:3] + (np.ascontiguousarray(Uu), np.ascontiguousarray(Vu)), cam


def count_models(models, status, cam, dist, soa, thr, upto=None):
    """inlier counts of the model records under the distorted test; 0 where status <= 0"""
    t2 = np.float32(O.thr2(thr))
    H = len(status) if upto is None else min(upto, len(status))
    counts = np.zeros(len(status), np.int32)
    for h in range(H):
        if status[h] > 0:
            counts[h] = int(np.count_nonzero(err2(models[h, :9], models[h, 9:12], cam, dist, soa) <= t2))
    return counts


def hypotheses(p3, p2, K, dist, thr, seed, H, hyp0=0, **kw):
    """the chain's per-hypothesis outputs: models and status from the oracle on the ideal pixels,
    counts from the distorted test on the raw pixels -> (status, counts, models)"""
    soa, soa_i, cam = soa_pair(p3, p2, K, dist)
    _, status, models = O.pnp_hypotheses(soa_i, cam, thr, seed, H, hyp0=hyp0, models=True, **kw)
    return status, count_models(models, status, cam, dist, soa, thr), models


def ransac(p3, p2, K, dist, thr, seed, max_iters, conf=0.99, refine=True, reference_mode=False):
    """the whole chain of pnp_ransac(dist=): hypotheses, scan, mask, refit -> dict.
    reference_mode: OpenCV's MWC subsets of 5 points solved by EPnP, models through the rvec round
    trip (sampler="opencv", minimal="epnp5": what the solvePnPRansac shim runs)"""
    soa, soa_i, cam = soa_pair(p3, p2, K, dist)
    n = len(soa[0])
    k = 5 if reference_mode else 4
    kw = {}
    if reference_mode:
        subs, sst = O.mwc_subsets(n, max_iters, s=5)
        kw = dict(subsets=subs, sub_status=sst, minimal="epnp5", rvec=True)
    _, status, models = O.pnp_hypotheses(soa_i, cam, thr, seed, max_iters, models=True, **kw)
    # the scan is sequential: count the hypotheses it can reach, a growing prefix at a time
    m = 256
    while True:
        counts = count_models(models, status, cam, dist, soa, thr, upto=m)
        best, good, iters = O.scan(counts, status, n, k, conf, max_iters)
        if iters <= m or m >= max_iters:  # the scan consumed counted hypotheses only
            break
        m *= 2
    out = dict(best=best, n_inliers=good, iters=iters, R=None, t=None, mask=np.zeros(n, bool))
    if best >= 0:
        R, t = models[best, :9].reshape(3, 3).copy(), models[best, 9:12].copy()
        out["mask"] = err2(R, t, cam, dist, soa) <= np.float32(O.thr2(thr))
        out["R0"], out["t0"] = R, t
        if refine:
            R, t, _ = O.pnp_refine(soa_i, out["mask"].astype(np.uint8), cam, R, t)
        out["R"], out["t"] = R, t
    return out


@functools.lru_cache(maxsize=None)
def distorted_problem(n, outlier_ratio, seed, dist):
    """synth.pnp_problem without noise, its inlier pixels replaced by the restated distorted
    projection of the true pose + N(0, 0.5) px (all x draws first, then all y)"""
    pr = synth.pnp_problem(n, outlier_ratio, seed=seed, noise_px=0.0)
    cam = O.cam_from_K(pr["K"])
    p3 = pr["points3d"]
    pu, pv = project(pr["R"], pr["t"], cam, dist, p3[:, 0], p3[:, 1], p3[:, 2])
    rng = np.random.default_rng(seed + 100)
    nx = rng.normal(0.0, 0.5, size=n)
    ny = rng.normal(0.0, 0.5, size=n)
    px = pr["points2d"].copy()
    inl = pr["inlier"]
    px[inl, 0] = pu[inl] + nx[inl]
    px[inl, 1] = pv[inl] + ny[inl]
    pr = dict(pr)
    pr["points2d"] = px
    for v in pr.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return pr


@functools.lru_cache(maxsize=None)
def ransac_case(n, outlier_ratio, seed, dist, thr=8.0, max_iters=5000, refine=True):
    pr = distorted_problem(n, outlier_ratio, seed, dist)
    return ransac(pr["points3d"], pr["points2d"], pr["K"], dist, thr, 0x5EED, max_iters, refine=refine)
