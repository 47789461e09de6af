"""Python entry points over the C ABI (librsac.so).

``pnp_ransac(points2D, points3D, K, n_iters, reproj_thresh) -> (R, t, inlier_mask)``
is the north-star entry point: it replaces the RANSAC loop that
``cv2.solvePnPRansac`` runs for the reference (main_v1.py:497-502,
testpro-K.py:72-75, testpro.py:536-541, test_pro.py:515-520).
``homography_ransac`` replaces ``cv2.findHomography(..., cv2.RANSAC, thr)``
(main_v1.py:312, process.py:200).  The batched forms replace the Python loops
around those calls (main_v1.py:274-284, testpro-K.py:58-75).

Inputs may be numpy arrays (host, float64 as the reference holds them) or
torch tensors on the GPU (float64 AoS, used in place).  Results for GPU
inputs keep the mask on the GPU.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib as L


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


class _In:
    """Marshalled input: pointer + whether it is on the device + keepalive."""

    def __init__(self, a, cols: int):
        self.device = False
        self.torch = False
        if _is_torch(a):
            import torch
            self.torch = True
            if a.dtype == torch.float64 and a.dim() == 2 and a.shape[1] == cols and a.is_contiguous():
                t = a  # already the (n, cols) float64 layout: no view or copy (the common GPU call)
            else:
                t = a.reshape(-1, cols).to(torch.float64).contiguous()
            self.device = t.is_cuda
            if not self.device:
                t = t.numpy()
            self.keep = t
            self.n = t.shape[0]
            self.ptr = t.data_ptr() if self.device else t.ctypes.data
            self.dev_index = a.device.index if self.device else None
        else:
            arr = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, cols))
            self.keep = arr
            self.n = arr.shape[0]
            self.ptr = arr.ctypes.data
            self.dev_index = None


def _stream_of(inp: _In):
    if inp.device:
        import torch
        # torch's raw getter returns the handle without building a Stream object (0.06 against
        # 1.7 us per call, scripts/py_overhead.py); the public form where a build lacks it
        raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        if raw is not None:
            return C.c_void_p(raw(inp.dev_index))
        return C.c_void_p(torch.cuda.current_stream(inp.keep.device).cuda_stream)
    return C.c_void_p(0)


def _device_of(inp: _In, device):
    if device is not None:
        return int(device)
    if inp.dev_index is not None:
        return int(inp.dev_index)
    return 0


class _Soa:
    """A device-resident float32 SoA point set, shape (2, n): rows x and y (RSAC_F_DEVICE_SOA)."""

    soa = True

    def __init__(self, a):
        t = a.contiguous()
        self.device = True
        self.torch = True
        self.keep = t
        self.n = t.shape[1]
        self.ptr = t.data_ptr()
        self.dev_index = a.device.index


def _hom_in(a):
    """_In for 2D points, or _Soa for a float32 device tensor of shape (2, n), n != 2"""
    if _is_torch(a) and a.is_cuda and a.dim() == 2 and a.shape[0] == 2 and a.shape[1] != 2:
        import torch
        if a.dtype == torch.float32:
            return _Soa(a)
    return _In(a, 2)


def _in_flags(inp) -> int:
    if getattr(inp, "soa", False):
        return L.F_DEVICE_SOA
    return L.F_DEVICE_IN if inp.device else 0


def _flags(adaptive, refine, sampler, exact_only=False, minimal="p3p", rvec=None):
    f = 0
    # rvec (PnP): each minimal model's rotation through Rodrigues(Rodrigues(R)) before it is scored,
    # as OpenCV's PnPRansacCallback keeps the model as (rvec, tvec) (main_v1.py:497, testpro-K.py:72);
    # default: on with OpenCV's sampler (the reference's own mode), off for Philox
    if (sampler == "opencv") if rvec is None else rvec:
        f |= L.F_RVEC_ROUNDTRIP
    # minimal: "p3p" (4-point samples, SOLVEPNP_P3P: this project's benchmark kernel, north_star's)
    # or "epnp5" (5-point samples solved by EPnP: solvePnPRansac's default SOLVEPNP_ITERATIVE
    # kernel, model_points 5 -- what the reference's calls run, main_v1.py:497, testpro-K.py:72)
    if minimal == "epnp5":
        f |= L.F_MINIMAL_EPNP5
    elif minimal != "p3p":
        raise ValueError(f"minimal must be 'p3p' or 'epnp5', got {minimal!r}")
    if adaptive:
        f |= L.F_ADAPTIVE
    # refine: True / "lm" -> LM from the minimal model; "epnp" -> EPnP on the inliers (solvePnPRansac
    # with SOLVEPNP_P3P); "epnp+lm" -> EPnP, then LM from it
    if refine is True or refine == "lm":
        f |= L.F_REFINE
    elif refine == "epnp":
        f |= L.F_EPNP
    elif refine == "epnp+lm":
        f |= L.F_EPNP | L.F_REFINE
    elif refine not in (False, None):
        raise ValueError(f"refine must be True/False, 'lm', 'epnp' or 'epnp+lm', got {refine!r}")
    if sampler == "opencv":
        f |= L.F_SAMPLER_OPENCV
    elif sampler != "philox":
        raise ValueError(f"sampler must be 'philox' or 'opencv', got {sampler!r}")
    if exact_only:
        f |= L.F_EXACT_ONLY
    return f


def _mask_buffer(inp: _In, n: int):
    if inp.device:
        import torch
        # bool storage is one byte holding 0 / 1: the ABI's uint8 mask, no reinterpreting view after
        m = torch.empty(max(n, 1), dtype=torch.bool, device=inp.keep.device)
        return m, m.data_ptr(), L.F_DEVICE_OUT
    m = np.zeros(max(n, 1), np.uint8)
    return m, m.ctypes.data, 0


def _finish_mask(m, n):
    # uint8 0/1 -> bool without a copy (torch: reinterpret the bytes, unless already bool)
    if _is_torch(m):
        import torch
        m = m if m.shape[0] == n else m[:n]
        return m if m.dtype == torch.bool else m.view(dtype=torch.bool)
    return m[:n].view(np.bool_)


@dataclass
class RansacInfo:
    ok: bool
    n_inliers: int
    best_hyp: int
    iters: int
    hyps_scored: int
    rounds: int
    gpu_ms: float
    solve_ms: float
    score_ms: float
    lo_improvements: int = 0
    cost: int = -1  # score="msac": the winner's truncated cost in units of 2**-msac_shift(thr) px^2 (-1: none)
    cost_px2: float = float("nan")  # ... in px^2
    median: float | None = None  # the LMedS calls: the winner's median squared error in px^2 (-1.0: none)


def _info(code, st: L.Stats) -> RansacInfo:
    return RansacInfo(ok=code == L.OK, n_inliers=st.n_inliers, best_hyp=st.best_hyp, iters=st.iters,
                      hyps_scored=st.hyps_scored, rounds=st.rounds, gpu_ms=st.gpu_ms, solve_ms=st.solve_ms,
                      score_ms=st.score_ms, lo_improvements=st.lo_improvements)


def _score_flag(score, what: str, *, lo=False, dist=None, supported: bool = True) -> int:
    """score="count" (inlier count, OpenCV's rule) or "msac" (lowest truncated cost; DESIGN.md "MSAC
    scoring") -> the flag bits; the combinations MSAC is not built for raise before any device work"""
    if score == "count":
        return 0
    if score != "msac":
        raise ValueError(f"score must be 'count' or 'msac', got {score!r}")
    if not supported:
        raise NotImplementedError(f"{what}: score='msac' is not built for this entry point (pnp_ransac, "
                                  "pnp_ransac_batched, pnp_ransac_batched_flat, homography_ransac, "
                                  "homography_ransac_batched, location_search and fundamental_ransac take it)")
    if lo:
        raise NotImplementedError(f"{what}: score='msac' with lo=True (LO-RANSAC on the cost) is not built")
    if _dist_arg(dist)[0] is not None:
        raise NotImplementedError(f"{what}: score='msac' with dist (lens distortion) is not built")
    return L.F_MSAC


def _last_costs(ctx, P: int) -> np.ndarray:
    costs = np.full(P, -1, np.int64)
    L.check(L.lib().rsac_last_costs(ctx.handle, costs.ctypes.data, P))
    return costs


def msac_shift(thr: float) -> int:
    """k of the MSAC cost at reprojection threshold thr: costs are in units of 2**-k px^2 (host-only)"""
    return int(L.lib().rsac_msac_shift(float(thr)))


def pose_cost(points2D, points3D, K, model12, thr: float):
    """(inlier count, MSAC cost) of one pose (R 9 row-major, t 3) on the host: the arithmetic the GPU
    kernel runs (rsac_pnp_cost_host), no device needed"""
    P3 = np.ascontiguousarray(np.asarray(points3D, np.float64).reshape(-1, 3))
    P2 = np.ascontiguousarray(np.asarray(points2D, np.float64).reshape(-1, 2))
    if P3.shape[0] != P2.shape[0]:
        raise ValueError("points3D and points2D differ in length")
    m12 = np.ascontiguousarray(np.asarray(model12, np.float64).reshape(-1)[:12])
    cnt, cost = C.c_int32(0), C.c_int64(-1)
    L.check(L.lib().rsac_pnp_cost_host(P3.ctypes.data, P2.ctypes.data, P3.shape[0], _K9(K).ctypes.data,
                                       m12.ctypes.data, float(thr), C.byref(cnt), C.byref(cost)))
    return int(cnt.value), int(cost.value)


def _K9(K) -> np.ndarray:
    K = np.ascontiguousarray(np.asarray(K, dtype=np.float64).reshape(3, 3))
    return K.reshape(9).copy()


def _dist_arg(dist):
    """Lens distortion coefficients -> (float64 array, length), or (None, 0) for None / empty /
    all-zero coefficients, which take the pinhole path (bit for bit today's results).  OpenCV's
    order (k1, k2, p1, p2[, k3[, k4, k5, k6]]); 12 and 14 (thin prism, tilt) are not built."""
    if dist is None:
        return None, 0
    d = np.ascontiguousarray(np.asarray(dist, dtype=np.float64).reshape(-1))
    if d.size == 0 or not np.any(d != 0):
        return None, 0
    if d.size in (12, 14):
        raise NotImplementedError(f"{d.size} distortion coefficients (thin prism / tilt terms) are not supported: "
                                  "pass 4, 5 or 8")
    if d.size not in (4, 5, 8):
        raise ValueError(f"distortion coefficients: 4, 5 or 8 expected, got {d.size}")
    return d, int(d.size)


def _no_dist(dist, what: str):
    """the entry points lens distortion is not built for: non-zero coefficients raise"""
    if _dist_arg(dist)[0] is not None:
        raise NotImplementedError(f"{what} with dist (lens distortion) is not built: undistort the points first "
                                  "(rsac.undistort_points(..., ideal=True)) or use the single-problem call")


def pnp_ransac(points2D, points3D, K, n_iters: int = 5000, reproj_thresh: float = 30.0, *,
               confidence: float = 0.99, seed: int = 0x5EED, sampler: str = "philox", adaptive: bool = True,
               refine: bool = True, device=None, return_info: bool = False, exact_only: bool = False,
               lo: bool = False, minimal: str = "p3p", rvec=None, dist=None, score: str = "count"):
    """RANSAC PnP on the GPU: (points2D, points3D, K, n_iters, reproj_thresh) -> (R, t, inlier_mask).

    score: "count" (default: the hypothesis with the most inliers, OpenCV's rule) or "msac" (the one
    with the lowest truncated cost, DESIGN.md "MSAC scoring"; info.cost / info.cost_px2 carry it).

    dist: lens distortion coefficients (4, 5 or 8, OpenCV's order) of the camera the raw
    points2D come from: every point is undistorted once, the minimal solves and the final solve
    run on the ideal pixels, and the inlier test compares the raw pixels with the distorted
    projection (DESIGN.md "Lens distortion").  None or zeros: the pinhole call.

    Defaults follow the reference call (iterationsCount=5000, reprojectionError=30,
    confidence=0.99; main_v1.py:497-502).  ``R`` is 3x3, ``t`` (3,) with
    x_cam = R X + t; ``inlier_mask`` is the RANSAC-phase mask (OpenCV's
    convention).  On failure R and t are None and the mask is all False.
    lo=True runs LO-RANSAC (local optimisation at every new best; BASELINE.json C5).
    minimal="epnp5" samples 5 points and solves them with EPnP (OpenCV's default
    SOLVEPNP_ITERATIVE kernel; RANSACUpdateNumIters with model_points 5).
    rvec (default: sampler == "opencv"): score each minimal model as Rodrigues(Rodrigues(R)), the
    rotation OpenCV's computeError projects with.  4 points (5 under minimal="epnp5") take
    solvePnPRansac's count == model_points branch: one minimal solve on all points, every index
    an inlier, no final solve.
    """
    msac = _score_flag(score, "pnp_ransac", lo=lo, dist=dist)
    p3 = _In(points3D, 3)
    p2 = _In(points2D, 2)
    if p3.n != p2.n:
        raise ValueError(f"points3D ({p3.n}) and points2D ({p2.n}) differ in length")
    if p3.device != p2.device:
        raise ValueError("points3D and points2D must both be host arrays or both GPU tensors")
    n = p3.n
    ctx = L.context(_device_of(p3, device))
    flags = _flags(adaptive, refine, sampler, exact_only, minimal, rvec) | (L.F_LO if lo else 0) | msac
    if p3.device:
        flags |= L.F_DEVICE_IN
    d, nd = _dist_arg(dist)
    if d is not None and lo:
        raise NotImplementedError("pnp_ransac: lo=True with dist (LO-RANSAC with lens distortion) is not built")
    K9 = _K9(K)
    R = np.zeros(9)
    t = np.zeros(3)
    mask, mptr, mflag = _mask_buffer(p3, n)
    flags |= mflag
    st = L.Stats()
    with ctx.lock:
        if d is not None:
            code = L.check(L.lib().rsac_pnp_ransac_dist(ctx.handle, C.c_void_p(p3.ptr), C.c_void_p(p2.ptr), n,
                                                        K9.ctypes.data, d.ctypes.data, nd, int(n_iters),
                                                        float(reproj_thresh), float(confidence),
                                                        int(seed) & (2**64 - 1), flags, R.ctypes.data, t.ctypes.data,
                                                        C.c_void_p(mptr), C.byref(st) if return_info else None,
                                                        _stream_of(p3)))
        else:
            code = L.check(L.lib().rsac_pnp_ransac(ctx.handle, C.c_void_p(p3.ptr), C.c_void_p(p2.ptr), n,
                                                   K9.ctypes.data, int(n_iters), float(reproj_thresh),
                                                   float(confidence), int(seed) & (2**64 - 1), flags, R.ctypes.data,
                                                   t.ctypes.data, C.c_void_p(mptr),
                                                   C.byref(st) if return_info else None, _stream_of(p3)))
        cost = int(_last_costs(ctx, 1)[0]) if msac and return_info else -1
    m = _finish_mask(mask, n)
    out = (R.reshape(3, 3), t, m) if code == L.OK else (None, None, m)
    if not return_info:
        return out
    info = _info(code, st)
    if msac:
        info.cost = cost
        info.cost_px2 = cost / 2.0 ** msac_shift(reproj_thresh) if cost >= 0 else float("nan")
    return out + (info,)


def pnp_ransac_first_round(points2D, points3D, K, n_iters: int = 5000, reproj_thresh: float = 30.0, *,
                           confidence: float = 0.99, seed: int = 0x5EED, refine: bool = True, lo: bool = False,
                           device=None, score: str = "count"):
    """The multi-GPU adaptive loop's first round (rsac_pnp_ransac_first_round):
    pnp_ransac (Philox, adaptive) capped at its first 256-hypothesis round, run redundantly on
    every rank with no collective.  Returns (done, R, t, mask, scan, info) where scan is the Scan
    after the round and info the RansacInfo: done=True -> (R, t, mask) is pnp_ransac's result (R
    None: no model); done=False -> the scan goes on from scan.iters and (R, t) is the best model
    so far (mask None)."""
    _score_flag(score, "pnp_ransac_first_round", supported=False)
    p3 = _In(points3D, 3)
    p2 = _In(points2D, 2)
    if p3.n != p2.n:
        raise ValueError(f"points3D ({p3.n}) and points2D ({p2.n}) differ in length")
    if p3.device != p2.device:
        raise ValueError("points3D and points2D must both be host arrays or both GPU tensors")
    n = p3.n
    ctx = L.context(_device_of(p3, device))
    flags = _flags(True, refine, "philox") | (L.F_LO if lo else 0) | (L.F_DEVICE_IN if p3.device else 0)
    R, t = np.zeros(9), np.zeros(3)
    mask, mptr, mflag = _mask_buffer(p3, n)
    flags |= mflag
    scan = Scan(n_iters, n, confidence, 4)
    st = L.Stats()
    with ctx.lock:
        code = L.check(L.lib().rsac_pnp_ransac_first_round(
            ctx.handle, C.c_void_p(p3.ptr), C.c_void_p(p2.ptr), n, _K9(K).ctypes.data, int(n_iters),
            float(reproj_thresh), float(confidence), int(seed) & (2**64 - 1), flags, R.ctypes.data, t.ctypes.data,
            C.c_void_p(mptr), C.byref(scan.st), C.byref(st), _stream_of(p3)))
    info = _info(code, st)
    if code == L.MORE:
        has = scan.best >= 0
        return False, (R.reshape(3, 3) if has else None), (t if has else None), None, scan, info
    m = _finish_mask(mask, n)
    return True, (R.reshape(3, 3) if code == L.OK else None), (t if code == L.OK else None), m, scan, info


def homography_ransac(src, dst, reproj_thresh: float = 3.0, *, max_iters: int = 2000, confidence: float = 0.995,
                      seed: int = 0x5EED, sampler: str = "opencv", adaptive: bool = True, refine=True,
                      device=None, return_info: bool = False, score: str = "count"):
    """RANSAC homography src -> dst on the GPU: -> (H, mask).

    Mirrors cv2.findHomography(src, dst, cv2.RANSAC, thr) (main_v1.py:312):
    OpenCV's MWC subset sequence by default (sampler="opencv"), f32 error,
    RANSAC-phase mask, then a least-squares + LM polish of H on the inliers.
    score: "count" (default, OpenCV's rule) or "msac" (the hypothesis with the lowest truncated
    cost wins, DESIGN.md "MSAC scoring for homographies"; info.cost / info.cost_px2 carry it).
    refine: False returns the winner's minimal model, True (default) the polish on its inliers (device
    tensors: fitted on the device from the mask where it lies, the same bits); "lo" runs
    homography_local_opt from the winner's minimal model and returns that H and that mask -- the
    mask is then the optimised model's, not the RANSAC-phase one -- with info.lo_improvements the
    accepted rounds and info.n_inliers the optimised count.
    """
    refine = _hom_refine_arg(refine, "homography_ransac")
    msac = _score_flag(score, "homography_ransac")
    s = _In(src, 2)
    d = _In(dst, 2)
    if s.n != d.n:
        raise ValueError("src and dst differ in length")
    n = s.n
    ctx = L.context(_device_of(s, device))
    flags = _flags(adaptive, refine is True, sampler) | msac
    if s.device:
        flags |= L.F_DEVICE_IN
    H = np.zeros(9)
    mask, mptr, mflag = _mask_buffer(s, n)
    flags |= mflag
    st = L.Stats()
    with ctx.lock:
        code = L.check(L.lib().rsac_homography_ransac(ctx.handle, C.c_void_p(s.ptr), C.c_void_p(d.ptr), n,
                                                      int(max_iters), float(reproj_thresh), float(confidence),
                                                      int(seed) & (2**64 - 1), flags, H.ctypes.data,
                                                      C.c_void_p(mptr), C.byref(st), _stream_of(s)))
        cost = int(_last_costs(ctx, 1)[0]) if msac and return_info else -1
    m = _finish_mask(mask, n)
    out = (H.reshape(3, 3), m) if code == L.OK else (None, m)
    lo = None
    if refine == "lo" and code == L.OK:
        lo = homography_local_opt(src, dst, out[0], float(reproj_thresh) if reproj_thresh > 0 else 3.0, device=device)
        out = (lo[0], lo[1])
    if not return_info:
        return out
    info = _info(code, st)
    if msac:
        info.cost = cost
        thr = float(reproj_thresh) if reproj_thresh > 0 else 3.0  # findHomography's default
        info.cost_px2 = cost / 2.0 ** msac_shift(thr) if cost >= 0 else float("nan")
    if lo is not None:
        info.n_inliers = lo[2]
        info.lo_improvements = lo[3]
    return out + (info,)


def homography_cost(src, dst, H, thr: float):
    """(inlier count, MSAC cost) of one homography on the host: the arithmetic the GPU kernels run
    (rsac_hom_cost_host), no device needed"""
    s = np.ascontiguousarray(np.asarray(src, np.float64).reshape(-1, 2))
    d = np.ascontiguousarray(np.asarray(dst, np.float64).reshape(-1, 2))
    if s.shape[0] != d.shape[0]:
        raise ValueError("src and dst differ in length")
    H9 = np.ascontiguousarray(np.asarray(H, np.float64).reshape(9))
    cnt, cost = C.c_int32(0), C.c_int64(-1)
    L.check(L.lib().rsac_hom_cost_host(s.ctypes.data, d.ctypes.data, s.shape[0], H9.ctypes.data, float(thr),
                                       C.byref(cnt), C.byref(cost)))
    return int(cnt.value), int(cost.value)


def _lmeds_flags(n_iters, max_iters, refine, sampler):
    """n_iters=None: OpenCV's fixed count max(RANSACUpdateNumIters(confidence, 0.45, 4, max_iters), 3)
    (RSAC_F_ADAPTIVE); an integer: exactly that many hypotheses -> (flags, iteration argument)"""
    if refine not in (True, False):
        raise ValueError(f"refine must be True or False, got {refine!r}")
    if n_iters is not None and int(n_iters) < 1:
        raise ValueError("n_iters must be >= 1")
    flags = _flags(n_iters is None, refine, sampler, rvec=False)
    return flags, int(max_iters) if n_iters is None else int(n_iters)


def homography_lmeds(src, dst, *, max_iters: int = 2000, confidence: float = 0.995, n_iters=None,
                     seed: int = 0x5EED, sampler: str = "opencv", refine=True, device=None,
                     return_info: bool = False):
    """Least-median-of-squares homography src -> dst on the GPU: -> (H | None, mask).

    Mirrors cv2.findHomography(src, dst, cv2.LMEDS): no pixel threshold.  Every hypothesis (the
    subsets and minimal models of homography_ransac) is ranked by the median of its squared transfer
    errors over all points; the lowest median wins, the inlier bound follows from it (sigma =
    2.5 * 1.4826 * (1 + 5 / (n - 4)) * sqrt(median), at least 0.001), and the call succeeds when at
    least 4 points pass.  n_iters=None runs OpenCV's fixed number of hypotheses (55 at the default
    confidence and max_iters); an integer runs exactly that many.  refine: the least-squares + LM
    polish on the inliers ("lo": homography_local_opt from the winner's minimal model at thr = sigma;
    the mask is then the optimised model's, info.lo_improvements the accepted rounds).  return_info
    adds a RansacInfo with `median`, the winner's median.
    """
    refine = _hom_refine_arg(refine, "homography_lmeds")
    s = _In(src, 2)
    d = _In(dst, 2)
    if s.n != d.n:
        raise ValueError("src and dst differ in length")
    n = s.n
    ctx = L.context(_device_of(s, device))
    flags, iters = _lmeds_flags(n_iters, max_iters, refine is True, sampler)
    if s.device:
        flags |= L.F_DEVICE_IN
    H = np.zeros(9)
    mask, mptr, mflag = _mask_buffer(s, n)
    flags |= mflag
    st = L.Stats()
    med = C.c_double(-1.0)
    with ctx.lock:
        code = L.check(L.lib().rsac_homography_lmeds(ctx.handle, C.c_void_p(s.ptr), C.c_void_p(d.ptr), n, iters,
                                                     float(confidence), int(seed) & (2**64 - 1), flags,
                                                     H.ctypes.data, C.c_void_p(mptr), C.byref(med), C.byref(st),
                                                     _stream_of(s)))
    m = _finish_mask(mask, n)
    out = (H.reshape(3, 3), m) if code == L.OK else (None, m)
    lo = None
    if refine == "lo" and code == L.OK:
        lo = homography_local_opt(src, dst, out[0], lmeds_sigma(float(med.value), n, 4), device=device)
        out = (lo[0], lo[1])
    if not return_info:
        return out
    info = _info(code, st)
    info.median = float(med.value)
    if lo is not None:
        info.n_inliers = lo[2]
        info.lo_improvements = lo[3]
    return out + (info,)


def homography_lmeds_batched(src_list, dst_list, *, max_iters: int = 2000, confidence: float = 0.995, n_iters=None,
                             seed: int = 0x5EED, sampler: str = "opencv", refine: bool = True, device: int = 0):
    """P independent homography_lmeds calls in one launch sequence -> [(H | None, mask, n_inliers,
    median)] (median -1.0 without a model, 0.0 for a 4-point problem's direct model)."""
    s, off = _concat(src_list, 2)
    d, off2 = _concat(dst_list, 2)
    if not np.array_equal(off, off2):
        raise ValueError("per-problem src/dst counts differ")
    P = len(off) - 1
    if P and np.diff(off).min() < 4:
        raise ValueError("every problem needs >= 4 correspondences")
    ctx = L.context(device)
    flags, iters = _lmeds_flags(n_iters, max_iters, refine, sampler)
    H = np.zeros((P, 9))
    status = np.zeros(P, np.int32)
    ninl = np.zeros(P, np.int32)
    med = np.full(P, -1.0)
    mask = np.zeros(max(int(off[-1]), 1), np.uint8)
    with ctx.lock:
        L.check(L.lib().rsac_homography_lmeds_batched(ctx.handle, s.ctypes.data, d.ctypes.data, off.ctypes.data, P,
                                                      iters, float(confidence), int(seed) & (2**64 - 1), flags,
                                                      H.ctypes.data, status.ctypes.data, ninl.ctypes.data,
                                                      med.ctypes.data, mask.ctypes.data, None))
    out = []
    for p in range(P):
        ok = status[p] == L.OK
        out.append((H[p].reshape(3, 3) if ok else None, mask[off[p]:off[p + 1]].astype(bool), int(ninl[p]),
                    float(med[p])))
    return out


def hom_median(src, dst, H) -> float:
    """The LMedS score of one homography on the host (rsac_hom_median_host, the arithmetic the GPU
    kernel runs; no device needed): the median of the f32 squared transfer errors over all points."""
    s = np.ascontiguousarray(np.asarray(src, np.float64).reshape(-1, 2))
    d = np.ascontiguousarray(np.asarray(dst, np.float64).reshape(-1, 2))
    if s.shape[0] != d.shape[0]:
        raise ValueError("src and dst differ in length")
    H9 = np.ascontiguousarray(np.asarray(H, np.float64).reshape(9))
    med = C.c_double(0.0)
    L.check(L.lib().rsac_hom_median_host(s.ctypes.data, d.ctypes.data, s.shape[0], H9.ctypes.data, C.byref(med)))
    return float(med.value)


def lmeds_sigma(median: float, n: int, model_points: int = 4) -> float:
    """sigma of the LMedS inlier test for a best median over n points (floored at 0.001); a point is
    an inlier when its f32 squared error is <= float32(sigma * sigma)"""
    return float(L.lib().rsac_lmeds_sigma(float(median), int(n), int(model_points)))


def _fm_refine_arg(refine, what: str):
    if refine is True or refine is False or (isinstance(refine, str) and refine == "lo"):
        return refine
    raise ValueError(f"{what}: refine must be False, True or 'lo', got {refine!r}")


def _hom_refine_arg(refine, what: str):
    if refine is True or refine is False or (isinstance(refine, str) and refine == "lo"):
        return refine
    raise ValueError(f"{what}: refine must be False, True or 'lo', got {refine!r}")


def fundamental_fit(pts1, pts2, mask=None, *, device=None):
    """Least-squares fundamental matrix over the masked points (mask None = all): the normalised
    8-point fit, rank 2, unit Frobenius norm (DESIGN.md "Fundamental matrix: least-squares refit and
    local optimisation") -> F (3,3), or None without a model (fewer than 8 masked points, a
    non-finite coordinate under the mask, coincident points).

    NumPy inputs with device=None run the host twin (rsac_fundamental_fit, no GPU needed); torch
    device tensors (with a device bool / uint8 mask) or device=<index> run the kernels
    (rsac_fundamental_fit_device).  Both return the same bits.
    """
    on_device = _is_torch(pts1) and pts1.is_cuda
    if not on_device and device is None:
        a, b, _ = _fm_host_args(pts1, pts2, np.zeros(9))
        m = None if mask is None else _host_mask_arg(mask, a.shape[0])
        F = np.zeros(9)
        code = L.check(L.lib().rsac_fundamental_fit(a.ctypes.data, b.ctypes.data, a.shape[0],
                                                    m.ctypes.data if m is not None else None, F.ctypes.data))
        return F.reshape(3, 3) if code == L.OK else None
    a = _In(pts1, 2)
    b = _In(pts2, 2)
    if a.n != b.n:
        raise ValueError("pts1 and pts2 differ in length")
    if a.device != b.device:
        raise ValueError("pts1 and pts2 must both be on the host or both on the device")
    mptr, keep = _fit_mask_arg(a, mask, a.n)
    ctx = L.context(_device_of(a, device))
    F = np.zeros(9)
    with ctx.lock:
        code = L.check(L.lib().rsac_fundamental_fit_device(ctx.handle, C.c_void_p(a.ptr), C.c_void_p(b.ptr), a.n,
                                                           C.c_void_p(mptr), L.F_DEVICE_IN if a.device else 0,
                                                           F.ctypes.data, _stream_of(a)))
    return F.reshape(3, 3) if code == L.OK else None


def fundamental_local_opt(pts1, pts2, F, reproj_thresh: float = 1.5, *, max_rounds: int = 4, device=None):
    """Local optimisation of a fundamental matrix on the GPU (rsac_fundamental_local_opt) ->
    (F (3,3), mask, count, steps).

    From F: the inlier mask at reproj_thresh (fundamental_ransac's test), the least-squares fit on
    it, the fit's mask, ... -- a round is accepted only when its inlier count rises strictly, at
    most max_rounds are accepted.  Returns the last accepted model (F itself after 0 steps), its
    mask and count, and the number of accepted rounds.  The mask stays on the device for device inputs.
    """
    thr = _lo_thresh_arg(reproj_thresh, max_rounds)
    F9 = np.ascontiguousarray(np.asarray(F, np.float64).reshape(-1))
    if F9.shape[0] != 9:
        raise ValueError("F must have 9 elements")
    a = _In(pts1, 2)
    b = _In(pts2, 2)
    if a.n != b.n:
        raise ValueError("pts1 and pts2 differ in length")
    if a.n < 1:
        raise ValueError("no points")
    ctx = L.context(_device_of(a, device))
    mask, mptr, mflag = _mask_buffer(a, a.n)
    Fo = np.zeros(9)
    cnt, steps = C.c_int32(0), C.c_int32(0)
    with ctx.lock:
        L.check(L.lib().rsac_fundamental_local_opt(ctx.handle, C.c_void_p(a.ptr), C.c_void_p(b.ptr), a.n,
                                                   F9.ctypes.data, thr, int(max_rounds),
                                                   (L.F_DEVICE_IN if a.device else 0) | mflag, Fo.ctypes.data,
                                                   C.byref(cnt), C.byref(steps), C.c_void_p(mptr), _stream_of(a)))
    return Fo.reshape(3, 3), _finish_mask(mask, a.n), int(cnt.value), int(steps.value)


def _fm_minimal(minimal, what: str):
    """minimal="8pt" | "7pt" of the fundamental-matrix calls -> (flag bits, sample size)"""
    if minimal == "8pt":
        return 0, 8
    if minimal == "7pt":
        return L.F_FM_7POINT, 7
    raise ValueError(f"{what}: minimal must be '8pt' or '7pt', got {minimal!r}")


def fundamental_ransac(pts1, pts2, reproj_thresh: float = 1.5, *, max_iters: int = 100_000,
                       confidence: float = 0.99, seed: int = 0x5EED, adaptive: bool = True, device=None,
                       return_info: bool = False, exact_only: bool = False, score: str = "count", refine=False,
                       minimal: str = "8pt"):
    """Fundamental matrix RANSAC (BASELINE.json configs[3]): 8-point samples, Sampson test.

    pts1, pts2 (N,2) with x2^T F x1 = 0.  Returns (F (3,3) unit Frobenius norm or None, mask).
    minimal: "8pt" (default) or "7pt" (DESIGN.md §23): 7-point samples with up to three models each.
    max_iters and info.iters then count samples, info.best_hyp is the record index (sample
    best_hyp // 3, root best_hyp % 3), the iteration bound uses model_points = 7, and n >= 7 suffices.
    It pays at high outlier shares (fewer samples to reach the confidence) and costs about 2.4
    scored models per sample.
    score: "count" (default) or "msac" (the hypothesis with the lowest truncated squared Sampson
    cost wins, DESIGN.md "MSAC and LMedS for the fundamental matrix"; it runs the exact f64 path;
    info.cost / info.cost_px2 carry the winner's cost).
    refine: False (default) returns the winner's minimal 8-point model; True returns the
    least-squares fit on the winner's inliers (fundamental_fit on the returned mask; the mask, the
    count and info stay the RANSAC phase's, as for pnp_ransac and homography_ransac; a fit without a
    model keeps the minimal F); "lo" runs fundamental_local_opt from the winner and returns that F
    and that mask -- the mask is then the optimised model's, not the RANSAC-phase one -- with
    info.lo_improvements the accepted rounds and info.n_inliers the optimised count.
    """
    refine = _fm_refine_arg(refine, "fundamental_ransac")
    msac = _score_flag(score, "fundamental_ransac")
    mflag7, _ = _fm_minimal(minimal, "fundamental_ransac")
    a = _In(pts1, 2)
    b = _In(pts2, 2)
    if a.n != b.n:
        raise ValueError("pts1 and pts2 differ in length")
    ctx = L.context(_device_of(a, device))
    flags = _flags(adaptive, False, "philox", exact_only) | (L.F_DEVICE_IN if a.device else 0) | msac | mflag7
    if refine is True:
        flags |= L.F_REFINE
    mask, mptr, mflag = _mask_buffer(a, a.n)
    flags |= mflag
    F = np.zeros(9)
    st = L.Stats()
    with ctx.lock:
        code = L.check(L.lib().rsac_fundamental_ransac(ctx.handle, C.c_void_p(a.ptr), C.c_void_p(b.ptr), a.n,
                                                       int(max_iters), float(reproj_thresh), float(confidence),
                                                       int(seed) & (2**64 - 1), flags, F.ctypes.data,
                                                       C.c_void_p(mptr), C.byref(st), _stream_of(a)))
        cost = int(_last_costs(ctx, 1)[0]) if msac and return_info else -1
    m = _finish_mask(mask, a.n)
    out = (F.reshape(3, 3) if code == L.OK else None, m)
    lo = None
    if refine == "lo" and code == L.OK:
        lo = fundamental_local_opt(pts1, pts2, out[0], reproj_thresh, device=device)
        out = (lo[0], lo[1])
    if not return_info:
        return out
    info = _info(code, st)
    if msac:
        info.cost = cost
        info.cost_px2 = cost / 2.0 ** msac_shift(float(reproj_thresh)) if cost >= 0 else float("nan")
    if lo is not None:
        info.n_inliers = lo[2]
        info.lo_improvements = lo[3]
    return out + (info,)


def fundamental_lmeds(pts1, pts2, *, max_iters: int = 2000, confidence: float = 0.99, n_iters=None,
                      seed: int = 0x5EED, device=None, return_info: bool = False, refine=False,
                      minimal: str = "8pt"):
    """Least-median-of-squares fundamental matrix on the GPU: -> (F | None, mask).  No pixel threshold.

    minimal="7pt" (DESIGN.md §23): 7-point samples, up to three models each; the sample count is
    lmeds_num_iters(confidence, 7, max_iters), sigma divides by n - 7 (n >= 8) and the call succeeds
    with at least 7 points in the mask.  The text below describes the default, "8pt".

    Every hypothesis (the 8-point samples and models of fundamental_ransac) is ranked by the median
    of its f32 squared Sampson distances over all points; the lowest median wins, the inlier bound
    follows from it (sigma = 2.5 * 1.4826 * (1 + 5 / (n - 8)) * sqrt(median), at least 0.001; the
    mask is fundamental_ransac's test at thr = sigma), and the call succeeds when at least 8 points
    pass.  Needs n >= 9.  n_iters=None runs the fixed count lmeds_num_iters(confidence, 8, max_iters)
    (548 at the defaults); an integer runs exactly that many.  return_info adds a
    RansacInfo with `median`, the winner's median.
    refine: False (default) returns the minimal model; True replaces F by fundamental_fit on the
    returned mask (a second call on the device; a fit without a model keeps the minimal F; the mask
    stays as it is); "lo" runs fundamental_local_opt from the winner at thr = sigma and returns
    that F and that mask (the optimised model's), info.lo_improvements the accepted rounds.
    """
    refine = _fm_refine_arg(refine, "fundamental_lmeds")
    a = _In(pts1, 2)
    b = _In(pts2, 2)
    if a.n != b.n:
        raise ValueError("pts1 and pts2 differ in length")
    if n_iters is not None and int(n_iters) < 1:
        raise ValueError("n_iters must be >= 1")
    n = a.n
    mflag7, sk = _fm_minimal(minimal, "fundamental_lmeds")
    ctx = L.context(_device_of(a, device))
    flags = (L.F_ADAPTIVE if n_iters is None else 0) | (L.F_DEVICE_IN if a.device else 0) | mflag7
    iters = int(max_iters) if n_iters is None else int(n_iters)
    F = np.zeros(9)
    mask, mptr, mflag = _mask_buffer(a, n)
    flags |= mflag
    st = L.Stats()
    med = C.c_double(-1.0)
    with ctx.lock:
        code = L.check(L.lib().rsac_fundamental_lmeds(ctx.handle, C.c_void_p(a.ptr), C.c_void_p(b.ptr), n, iters,
                                                      float(confidence), int(seed) & (2**64 - 1), flags,
                                                      F.ctypes.data, C.c_void_p(mptr), C.byref(med), C.byref(st),
                                                      _stream_of(a)))
    m = _finish_mask(mask, n)
    out = (F.reshape(3, 3), m) if code == L.OK else (None, m)
    lo = None
    if code == L.OK and refine is True:
        fit = fundamental_fit(pts1, pts2, m, device=_device_of(a, device))
        if fit is not None:
            out = (fit, m)
    elif code == L.OK and refine == "lo":
        lo = fundamental_local_opt(pts1, pts2, out[0], lmeds_sigma(float(med.value), n, sk), device=device)
        out = (lo[0], lo[1])
    if not return_info:
        return out
    info = _info(code, st)
    info.median = float(med.value)
    if lo is not None:
        info.n_inliers = lo[2]
        info.lo_improvements = lo[3]
    return out + (info,)


def _fm_host_args(pts1, pts2, F):
    a = np.ascontiguousarray(np.asarray(pts1, np.float64).reshape(-1, 2))
    b = np.ascontiguousarray(np.asarray(pts2, np.float64).reshape(-1, 2))
    if a.shape[0] != b.shape[0]:
        raise ValueError("pts1 and pts2 differ in length")
    return a, b, np.ascontiguousarray(np.asarray(F, np.float64).reshape(9))


def fundamental_errors(pts1, pts2, F) -> np.ndarray:
    """The f32 squared Sampson distances of one F over all points on the host (rsac_fm_err_host, the
    arithmetic the GPU kernels run; no device needed)"""
    a, b, F9 = _fm_host_args(pts1, pts2, F)
    err = np.zeros(a.shape[0], np.float32)
    L.check(L.lib().rsac_fm_err_host(a.ctypes.data, b.ctypes.data, a.shape[0], F9.ctypes.data, err.ctypes.data))
    return err


def fundamental_cost(pts1, pts2, F, thr: float):
    """(inlier count, MSAC cost) of one F on the host (rsac_fm_cost_host), no device needed"""
    a, b, F9 = _fm_host_args(pts1, pts2, F)
    cnt, cost = C.c_int32(0), C.c_int64(-1)
    L.check(L.lib().rsac_fm_cost_host(a.ctypes.data, b.ctypes.data, a.shape[0], F9.ctypes.data, float(thr),
                                      C.byref(cnt), C.byref(cost)))
    return int(cnt.value), int(cost.value)


def fm_median(pts1, pts2, F) -> float:
    """The LMedS score of one F on the host (rsac_fm_median_host; no device needed): the median of
    the f32 squared Sampson distances over all points"""
    a, b, F9 = _fm_host_args(pts1, pts2, F)
    med = C.c_double(0.0)
    L.check(L.lib().rsac_fm_median_host(a.ctypes.data, b.ctypes.data, a.shape[0], F9.ctypes.data, C.byref(med)))
    return float(med.value)


def cubic_real_roots(c) -> np.ndarray:
    """The real roots of c[0] + c[1] x + c[2] x^2 + c[3] x^3 in ascending order, on the host
    (rsac_cubic_real_roots; no device needed): the 7-point solver's root finder, whose bits the
    kernel reproduces.  c[3] == 0 is the quadratic, c[3] == c[2] == 0 the linear case."""
    cc = np.ascontiguousarray(np.asarray(c, np.float64).reshape(4))
    roots = np.zeros(3)
    n = L.lib().rsac_cubic_real_roots(cc.ctypes.data, roots.ctypes.data)
    return roots[:n].copy()


def fundamental_minimal7(pts1, pts2) -> list:
    """The 7-point minimal solver on the host (rsac_fm_minimal7; no device needed): 7 correspondences
    -> the list of 0 .. 3 models F (3,3), unit Frobenius norm, in ascending root order -- the bits
    record 3s + r of hypotheses("fundamental", ..., minimal="7pt") holds for that sample."""
    a = np.ascontiguousarray(np.asarray(pts1, np.float64).reshape(-1, 2))
    b = np.ascontiguousarray(np.asarray(pts2, np.float64).reshape(-1, 2))
    if a.shape[0] != 7 or b.shape[0] != 7:
        raise ValueError("fundamental_minimal7 takes exactly 7 correspondences")
    F = np.zeros(27)
    n = C.c_int32(0)
    L.check(L.lib().rsac_fm_minimal7(a.ctypes.data, b.ctypes.data, F.ctypes.data, C.byref(n)))
    return [F[9 * r:9 * r + 9].reshape(3, 3).copy() for r in range(int(n.value))]


def _concat(parts, cols):
    arrs = [np.asarray(p, dtype=np.float64).reshape(-1, cols) for p in parts]
    off = np.zeros(len(arrs) + 1, np.int64)
    off[1:] = np.cumsum([a.shape[0] for a in arrs])
    return np.ascontiguousarray(np.concatenate(arrs, axis=0) if arrs else np.zeros((0, cols))), off


def _concat_host_masks(mask_list, off):
    """the concatenated uint8 masks of a batched fit on host points (one byte for no points at all)"""
    parts = [_host_mask_arg(mk, int(off[p + 1] - off[p])) for p, mk in enumerate(mask_list)]
    return np.ascontiguousarray(np.concatenate(parts)) if off[-1] else np.zeros(1, np.uint8)


class _FmBatch:
    """The concatenated points of a batched fundamental-matrix call.  Problems given as device
    tensors (every one of them) stay on the device (float64 (n, 2), RSAC_F_DEVICE_IN; the masks come
    back as device tensors); anything else is gathered into host arrays, as homography_ransac_batched
    does.  Mismatched list lengths or per-problem counts raise ValueError before any device work."""

    def __init__(self, pts1_list, pts2_list, device):
        pts1_list, pts2_list = list(pts1_list), list(pts2_list)
        if len(pts1_list) != len(pts2_list):
            raise ValueError("pts1_list and pts2_list differ in length")
        both = pts1_list + pts2_list
        self.on_device = bool(both) and all(_is_torch(x) and x.is_cuda for x in both)
        if self.on_device:
            import torch
            a = [x.reshape(-1, 2) for x in pts1_list]
            b = [x.reshape(-1, 2) for x in pts2_list]
            off = np.zeros(len(a) + 1, np.int64)
            off[1:] = np.cumsum([x.shape[0] for x in a])
            if [x.shape[0] for x in a] != [x.shape[0] for x in b]:
                raise ValueError("per-problem pts1/pts2 counts differ")
            self.tdev = a[0].device
            self.keep = (torch.cat(a).to(torch.float64).contiguous(), torch.cat(b).to(torch.float64).contiguous())
            self.ptrs = (self.keep[0].data_ptr(), self.keep[1].data_ptr())
            self.flags = L.F_DEVICE_IN
            self.device = int(self.tdev.index or 0)
        else:
            host = [x.cpu() if _is_torch(x) else x for x in both]
            a, off = _concat(host[:len(pts1_list)], 2)
            b, off2 = _concat(host[len(pts1_list):], 2)
            if not np.array_equal(off, off2):
                raise ValueError("per-problem pts1/pts2 counts differ")
            self.tdev = None
            self.keep = (a, b)
            self.ptrs = (a.ctypes.data, b.ctypes.data)
            self.flags = 0
            self.device = int(device)
        self.off = off
        self.P = len(off) - 1
        self.total = int(off[-1])
        self.counts = np.diff(off)

    def stream(self):
        if not self.on_device:
            return C.c_void_p(0)
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.tdev).cuda_stream)

    def mask_buffer(self):
        """-> (buffer, pointer, flag) for the concatenated masks, on the device when the points are"""
        if self.on_device:
            import torch
            m = torch.zeros(max(self.total, 1), dtype=torch.bool, device=self.tdev)
            return m, m.data_ptr(), L.F_DEVICE_OUT
        m = np.zeros(max(self.total, 1), np.uint8)
        return m, m.ctypes.data, 0

    def split(self, m):
        """the per-problem bool masks of a concatenated mask buffer"""
        off = self.off
        if self.on_device:
            return [m[int(off[p]):int(off[p + 1])] for p in range(self.P)]
        return [m[off[p]:off[p + 1]].astype(bool) for p in range(self.P)]

    def masks_arg(self, mask_list):
        """(pointer, keepalive) of the concatenated input masks (None: all points)"""
        if mask_list is None:
            return None, None
        mask_list = list(mask_list)
        if len(mask_list) != self.P:
            raise ValueError("mask_list and pts1_list differ in length")
        if self.on_device:
            import torch
            parts = [torch.as_tensor(mk, device=self.tdev).reshape(-1) for mk in mask_list]
            if [int(x.shape[0]) for x in parts] != [int(k) for k in self.counts]:
                raise ValueError("mask and points differ in length")
            if not self.total:
                keep = torch.zeros(1, dtype=torch.bool, device=self.tdev)
            elif len({x.dtype for x in parts}) == 1:  # one concatenation, then one comparison
                keep = torch.cat(parts)
                keep = (keep if keep.dtype == torch.bool else keep.ne(0)).contiguous()
            else:
                keep = torch.cat([x.ne(0) for x in parts]).contiguous()
            return keep.data_ptr(), keep
        keep = _concat_host_masks(mask_list, self.off)
        return keep.ctypes.data, keep


def fundamental_fit_batched(pts1_list, pts2_list, mask_list=None, *, device=0):
    """fundamental_fit of P independent problems in three launches whatever P
    (rsac_fundamental_fit_batched_device) -> [F (3,3) | None]; every F has the bits of the single
    host fit of that problem.  A problem may have fewer than 8 (masked) points: None.  Lists of
    device tensors (with device masks) are fitted in place."""
    bt = _FmBatch(pts1_list, pts2_list, device)
    if bt.P < 1:
        return []
    mptr, keep = bt.masks_arg(mask_list)
    ctx = L.context(bt.device)
    F = np.zeros((bt.P, 9))
    status = np.zeros(bt.P, np.int32)
    with ctx.lock:
        L.check(L.lib().rsac_fundamental_fit_batched_device(ctx.handle, C.c_void_p(bt.ptrs[0]), C.c_void_p(bt.ptrs[1]),
                                                            bt.off.ctypes.data, bt.P, C.c_void_p(mptr), bt.flags,
                                                            F.ctypes.data, status.ctypes.data, bt.stream()))
    del keep
    return [F[p].reshape(3, 3) if status[p] == L.OK else None for p in range(bt.P)]


def fundamental_local_opt_batched(pts1_list, pts2_list, F_list, reproj_thresh: float = 1.5, *, max_rounds: int = 4,
                                  device=0):
    """fundamental_local_opt of P independent problems side by side
    (rsac_fundamental_local_opt_batched) -> [(F (3,3) | None, mask, count, steps)].

    Every round is one batched mask, one batched fit and one host synchronisation for the problems
    whose count is still rising; each problem follows exactly the loop and acceptance rule of the
    single call.  F_list[p] None (or all zeros): no model -> (None, zero mask, 0, 0)."""
    thr = _lo_thresh_arg(reproj_thresh, max_rounds)
    bt = _FmBatch(pts1_list, pts2_list, device)
    F_list = list(F_list)
    if len(F_list) != bt.P:
        raise ValueError("F_list and pts1_list differ in length")
    Fin = _model_rows(F_list, "every F")
    if bt.P < 1:
        return []
    ctx = L.context(bt.device)
    mask, mptr, mflag = bt.mask_buffer()
    Fo = np.zeros((bt.P, 9))
    cnt = np.zeros(bt.P, np.int32)
    steps = np.zeros(bt.P, np.int32)
    with ctx.lock:
        L.check(L.lib().rsac_fundamental_local_opt_batched(ctx.handle, C.c_void_p(bt.ptrs[0]), C.c_void_p(bt.ptrs[1]),
                                                           bt.off.ctypes.data, bt.P, Fin.ctypes.data, thr,
                                                           int(max_rounds), bt.flags | mflag, Fo.ctypes.data,
                                                           cnt.ctypes.data, steps.ctypes.data, C.c_void_p(mptr),
                                                           bt.stream()))
    masks = bt.split(mask)
    return [(Fo[p].reshape(3, 3) if Fin[p].any() else None, masks[p], int(cnt[p]), int(steps[p]))
            for p in range(bt.P)]


def fundamental_ransac_batched(pts1_list, pts2_list, reproj_thresh: float = 1.5, *, max_iters: int = 2000,
                               confidence: float = 0.99, seed: int = 0x5EED, adaptive: bool = True,
                               score: str = "count", refine=False, exact_only: bool = False, device=0,
                               minimal: str = "8pt"):
    """P independent fundamental_ransac calls in one launch sequence (rsac_fundamental_ransac_batched)
    -> [(F | None, mask, n_inliers)]; under score="msac" each tuple ends with the winner's cost (-1
    without a model).  minimal="7pt": as in fundamental_ransac (max_iters counts samples, the buffers
    hold P x 3 x max_iters records, every problem needs >= 7 correspondences).

    Problem p's winner, count, mask, F and iteration bound are those of fundamental_ransac on its
    points with the same arguments (the hypotheses do not depend on the problem).  refine: False,
    True (one batched least-squares fit on the RANSAC-phase masks, which stay as they are; a fit
    without a model keeps the minimal F) or "lo" (fundamental_local_opt_batched from the winners, 4
    rounds as on the single call; mask and n_inliers are then the optimised models').
    max_iters defaults to 2000, not the single call's 100 000: the hypothesis buffers hold P x
    max_iters records.  Every problem needs >= 8 correspondences.  Lists of device tensors stay on the
    device, and so do their masks."""
    refine = _fm_refine_arg(refine, "fundamental_ransac_batched")
    msac = _score_flag(score, "fundamental_ransac_batched")
    bt = _FmBatch(pts1_list, pts2_list, device)
    if bt.P < 1:
        return []
    mflag7, sk = _fm_minimal(minimal, "fundamental_ransac_batched")
    if bt.counts.min() < sk:
        raise ValueError(f"every problem needs >= {sk} correspondences")
    ctx = L.context(bt.device)
    flags = _flags(adaptive, False, "philox", exact_only) | bt.flags | msac | mflag7
    if refine is True:
        flags |= L.F_REFINE
    mask, mptr, mflag = bt.mask_buffer()
    F = np.zeros((bt.P, 9))
    status = np.zeros(bt.P, np.int32)
    ninl = np.zeros(bt.P, np.int32)
    with ctx.lock:
        L.check(L.lib().rsac_fundamental_ransac_batched(ctx.handle, C.c_void_p(bt.ptrs[0]), C.c_void_p(bt.ptrs[1]),
                                                        bt.off.ctypes.data, bt.P, int(max_iters), float(reproj_thresh),
                                                        float(confidence), int(seed) & (2**64 - 1), flags | mflag,
                                                        F.ctypes.data, status.ctypes.data, ninl.ctypes.data,
                                                        C.c_void_p(mptr), bt.stream()))
        costs = _last_costs(ctx, bt.P) if msac else None
    Fs = [F[p].reshape(3, 3) if status[p] == L.OK else None for p in range(bt.P)]
    masks = bt.split(mask)
    counts = [int(k) for k in ninl]
    if refine == "lo":
        lo = fundamental_local_opt_batched(pts1_list, pts2_list, Fs, reproj_thresh, device=device)
        Fs, masks, counts = [r[0] for r in lo], [r[1] for r in lo], [r[2] for r in lo]
    out = []
    for p in range(bt.P):
        row = (Fs[p], masks[p], counts[p])
        out.append(row + (int(costs[p]),) if msac else row)
    return out


def fundamental_lmeds_batched(pts1_list, pts2_list, *, max_iters: int = 2000, confidence: float = 0.99, n_iters=None,
                              seed: int = 0x5EED, refine=False, device=0, minimal: str = "8pt"):
    """P independent fundamental_lmeds calls in one launch sequence (rsac_fundamental_lmeds_batched)
    -> [(F | None, mask, n_inliers, median)] (median -1.0 without a model).  minimal="7pt": as in
    fundamental_lmeds (every problem then needs >= 8 correspondences).

    The number of hypotheses is the same for every problem; each problem's sigma and inlier bound
    come from its own median and point count.  Every problem needs >= 9 correspondences.
    refine: True replaces each F by fundamental_fit_batched on the returned masks (a fit without a
    model keeps the minimal F; the masks stay); "lo" runs fundamental_local_opt from each winner at
    its own sigma -- the bounds differ per problem, so that is one call per problem -- and returns
    those F, masks and counts."""
    refine = _fm_refine_arg(refine, "fundamental_lmeds_batched")
    if n_iters is not None and int(n_iters) < 1:
        raise ValueError("n_iters must be >= 1")
    bt = _FmBatch(pts1_list, pts2_list, device)
    if bt.P < 1:
        return []
    mflag7, sk = _fm_minimal(minimal, "fundamental_lmeds_batched")
    if bt.counts.min() < sk + 1:
        raise ValueError(f"every problem needs >= {sk + 1} correspondences")
    ctx = L.context(bt.device)
    flags = (L.F_ADAPTIVE if n_iters is None else 0) | bt.flags | mflag7
    iters = int(max_iters) if n_iters is None else int(n_iters)
    mask, mptr, mflag = bt.mask_buffer()
    F = np.zeros((bt.P, 9))
    status = np.zeros(bt.P, np.int32)
    ninl = np.zeros(bt.P, np.int32)
    med = np.full(bt.P, -1.0)
    with ctx.lock:
        L.check(L.lib().rsac_fundamental_lmeds_batched(ctx.handle, C.c_void_p(bt.ptrs[0]), C.c_void_p(bt.ptrs[1]),
                                                       bt.off.ctypes.data, bt.P, iters, float(confidence),
                                                       int(seed) & (2**64 - 1), flags | mflag, F.ctypes.data,
                                                       status.ctypes.data, ninl.ctypes.data, med.ctypes.data,
                                                       C.c_void_p(mptr), bt.stream()))
    Fs = [F[p].reshape(3, 3) if status[p] == L.OK else None for p in range(bt.P)]
    masks = bt.split(mask)
    counts = [int(k) for k in ninl]
    if refine is True:
        fits = fundamental_fit_batched(pts1_list, pts2_list, masks, device=device)
        Fs = [fit if (F0 is not None and fit is not None) else F0 for F0, fit in zip(Fs, fits)]
    elif refine == "lo":
        pts1_list, pts2_list = list(pts1_list), list(pts2_list)
        for p in range(bt.P):
            if Fs[p] is not None:
                sigma = lmeds_sigma(float(med[p]), int(bt.counts[p]), sk)
                Fs[p], masks[p], counts[p], _ = fundamental_local_opt(pts1_list[p], pts2_list[p], Fs[p], sigma,
                                                                      device=bt.device)
    return [(Fs[p], masks[p], counts[p], float(med[p])) for p in range(bt.P)]


def pnp_ransac_batched(points2D_list, points3D_list, K_list, n_iters: int = 5000, reproj_thresh: float = 30.0, *,
                       confidence: float = 0.99, seed: int = 0x5EED, sampler: str = "philox", adaptive: bool = True,
                       refine: bool = True, device: int = 0, minimal: str = "p3p", rvec=None, dist=None,
                       score: str = "count"):
    """P independent PnP problems in one call (K sweep of testpro-K.py:58-75, C3 of BASELINE.json).

    Returns a list of (R, t, mask, n_inliers) per problem (R, t None on failure); under
    score="msac" each tuple ends with the winner's cost (int, -1 without a model).
    """
    msac = _score_flag(score, "pnp_ransac_batched", dist=dist)
    _no_dist(dist, "pnp_ransac_batched")
    p3, off = _concat(points3D_list, 3)
    p2, off2 = _concat(points2D_list, 2)
    if not np.array_equal(off, off2):
        raise ValueError("per-problem 3D/2D point counts differ")
    P = len(off) - 1
    Ks = np.ascontiguousarray(np.stack([np.asarray(k, np.float64).reshape(9) for k in K_list]))
    if Ks.shape[0] != P:
        raise ValueError("one K per problem required")
    if P and np.diff(off).min() < 4:
        raise ValueError("every problem needs >= 4 correspondences")
    ctx = L.context(device)
    flags = _flags(adaptive, refine, sampler, minimal=minimal, rvec=rvec) | msac
    R = np.zeros((P, 9))
    t = np.zeros((P, 3))
    status = np.zeros(P, np.int32)
    ninl = np.zeros(P, np.int32)
    mask = np.zeros(max(int(off[-1]), 1), np.uint8)
    with ctx.lock:
        L.check(L.lib().rsac_pnp_ransac_batched(ctx.handle, p3.ctypes.data, p2.ctypes.data, off.ctypes.data, P,
                                                Ks.ctypes.data, int(n_iters), float(reproj_thresh), float(confidence),
                                                int(seed) & (2**64 - 1), flags, R.ctypes.data, t.ctypes.data,
                                                status.ctypes.data, ninl.ctypes.data, mask.ctypes.data, None))
        costs = _last_costs(ctx, P) if msac else None
    out = []
    for p in range(P):
        m = mask[off[p]:off[p + 1]].astype(bool)
        ok = status[p] == L.OK
        row = (R[p].reshape(3, 3) if ok else None, t[p] if ok else None, m, int(ninl[p]))
        out.append(row + (int(costs[p]),) if msac else row)
    return out


def _pnp_lmeds_flags(what, n_iters, max_iters, confidence, refine, sampler, minimal, rvec):
    """The argument checks of the LMedS PnP calls (before any device work) -> (flags, iteration
    argument).  n_iters=None: the fixed count lmeds_num_iters(confidence, max_iters, model_points)
    (RSAC_F_ADAPTIVE); an integer: exactly that many hypotheses."""
    if not 0.0 < float(confidence) < 1.0:
        raise ValueError(f"{what}: confidence must lie in (0, 1), got {confidence!r}")
    if n_iters is None and int(max_iters) < 1:
        raise ValueError(f"{what}: max_iters must be >= 1")
    if n_iters is not None and int(n_iters) < 1:
        raise ValueError(f"{what}: n_iters must be >= 1")
    flags = _flags(n_iters is None, refine, sampler, minimal=minimal, rvec=rvec)
    return flags, int(max_iters) if n_iters is None else int(n_iters)


def pnp_lmeds(points2D, points3D, K, *, max_iters: int = 2000, confidence: float = 0.99, n_iters=None,
              seed: int = 0x5EED, sampler: str = "philox", minimal: str = "p3p", rvec=None, refine=True,
              device=None, return_info: bool = False):
    """Least-median-of-squares PnP on the GPU: -> (R | None, t | None, mask).  No pixel threshold.

    Every hypothesis (the samples and minimal models of pnp_ransac under the same sampler, minimal
    and rvec) is ranked by the median of its f32 squared reprojection errors over all points; the
    lowest median wins, the inlier bound follows from it (sigma = 2.5 * 1.4826 * (1 + 5 / (n -
    model_points)) * sqrt(median), at least 0.001; a point is an inlier when its squared error is <=
    float32(sigma^2)), and the call succeeds when at least model_points points pass (4 for "p3p", 5
    for "epnp5").  More than half of the points must be inliers for the median to be an inlier's
    error.  n_iters=None runs the fixed count lmeds_num_iters(confidence, max_iters, model_points)
    (48 for P3P, 89 for EPnP-5 at the defaults); an integer runs exactly that many hypotheses.
    refine: as in pnp_ransac (True / "lm", False, "epnp", "epnp+lm"), the final solve on the LMedS
    mask.  sampler="opencv" turns the rvec round trip on by default.  GPU tensors in: the mask stays
    on the GPU.  return_info adds a RansacInfo whose `median` is the winner's median in px^2 (-1.0
    without a model, 0.0 for the direct model of exactly model_points points).
    Lens distortion is not a parameter: undistort first, rsac.undistort_points(..., ideal=True).
    """
    flags, iters = _pnp_lmeds_flags("pnp_lmeds", n_iters, max_iters, confidence, refine, sampler, minimal, rvec)
    p3 = _In(points3D, 3)
    p2 = _In(points2D, 2)
    if p3.n != p2.n:
        raise ValueError(f"points3D ({p3.n}) and points2D ({p2.n}) differ in length")
    if p3.device != p2.device:
        raise ValueError("points3D and points2D must both be host arrays or both GPU tensors")
    n = p3.n
    K9 = _K9(K)
    ctx = L.context(_device_of(p3, device))
    if p3.device:
        flags |= L.F_DEVICE_IN
    R, t = np.zeros(9), np.zeros(3)
    mask, mptr, mflag = _mask_buffer(p3, n)
    flags |= mflag
    st = L.Stats()
    med = C.c_double(-1.0)
    with ctx.lock:
        code = L.check(L.lib().rsac_pnp_lmeds(ctx.handle, C.c_void_p(p3.ptr), C.c_void_p(p2.ptr), n, K9.ctypes.data,
                                              iters, float(confidence), int(seed) & (2**64 - 1), flags, R.ctypes.data,
                                              t.ctypes.data, C.c_void_p(mptr), C.byref(med), C.byref(st),
                                              _stream_of(p3)))
    m = _finish_mask(mask, n)
    out = (R.reshape(3, 3), t, m) if code == L.OK else (None, None, m)
    if not return_info:
        return out
    info = _info(code, st)
    info.median = float(med.value)
    return out + (info,)


def pnp_lmeds_batched(points2D_list, points3D_list, K_list, *, max_iters: int = 2000, confidence: float = 0.99,
                      n_iters=None, seed: int = 0x5EED, sampler: str = "philox", minimal: str = "p3p", rvec=None,
                      refine=True, device: int = 0):
    """P independent pnp_lmeds calls in one launch sequence -> [(R | None, t | None, mask, n_inliers,
    median)].  A K sweep (testpro-K.py:58-75) passes the same points with one K per problem: the
    winners' medians are comparable across the intrinsics, which inlier counts under one pixel
    bound are not.  Undistort first (rsac.undistort_points(..., ideal=True)): no dist here."""
    flags, iters = _pnp_lmeds_flags("pnp_lmeds_batched", n_iters, max_iters, confidence, refine, sampler, minimal,
                                    rvec)
    p3, off = _concat(points3D_list, 3)
    p2, off2 = _concat(points2D_list, 2)
    if not np.array_equal(off, off2):
        raise ValueError("per-problem 3D/2D point counts differ")
    P = len(off) - 1
    if P < 1:
        raise ValueError("pnp_lmeds_batched: at least one problem required")
    Ks = np.ascontiguousarray(np.stack([np.asarray(k, np.float64).reshape(9) for k in K_list]))
    if Ks.shape[0] != P:
        raise ValueError("one K per problem required")
    if np.diff(off).min() < 4:
        raise ValueError("every problem needs >= 4 correspondences")
    ctx = L.context(device)
    R = np.zeros((P, 9))
    t = np.zeros((P, 3))
    status = np.zeros(P, np.int32)
    ninl = np.zeros(P, np.int32)
    med = np.full(P, -1.0)
    mask = np.zeros(max(int(off[-1]), 1), np.uint8)
    with ctx.lock:
        L.check(L.lib().rsac_pnp_lmeds_batched(ctx.handle, p3.ctypes.data, p2.ctypes.data, off.ctypes.data, P,
                                               Ks.ctypes.data, iters, float(confidence), int(seed) & (2**64 - 1),
                                               flags, R.ctypes.data, t.ctypes.data, status.ctypes.data,
                                               ninl.ctypes.data, med.ctypes.data, mask.ctypes.data, None))
    out = []
    for p in range(P):
        ok = status[p] == L.OK
        out.append((R[p].reshape(3, 3) if ok else None, t[p] if ok else None, mask[off[p]:off[p + 1]].astype(bool),
                    int(ninl[p]), float(med[p])))
    return out


def pnp_medians(points2D, points3D, K, hyp_begin: int = 0, n_hyps: int = 1024, *, seed: int = 0x5EED, subsets=None,
                minimal: str = "p3p", rvec=None, device=None):
    """The per-hypothesis probe of pnp_lmeds (rsac_pnp_medians) -> (status, medians, models): int8
    status, the f64 LMedS medians (-1.0 without a model) and the (n_hyps, 16) model records of
    hypotheses [hyp_begin, hyp_begin + n_hyps) of the Philox sampler, or of an (n_hyps, 4) int32
    subset table ((n_hyps, 5) for minimal="epnp5").  rvec: as in hypotheses (default: on exactly
    when subsets are given)."""
    if int(n_hyps) < 1:
        raise ValueError("pnp_medians: n_hyps must be >= 1")
    if minimal not in ("p3p", "epnp5"):
        raise ValueError(f"minimal must be 'p3p' or 'epnp5', got {minimal!r}")
    k = 5 if minimal == "epnp5" else 4
    if rvec is None:
        rvec = subsets is not None
    sub = None if subsets is None else np.ascontiguousarray(np.asarray(subsets, np.int32).reshape(n_hyps, k))
    A = _In(points3D, 3)
    B = _In(points2D, 2)
    if A.n != B.n:
        raise ValueError(f"points3D ({A.n}) and points2D ({B.n}) differ in length")
    if A.device != B.device:
        raise ValueError("points3D and points2D must both be host arrays or both GPU tensors")
    K9 = _K9(K)
    ctx = L.context(_device_of(A, device))
    flags = (L.F_DEVICE_IN if A.device else 0) | (L.F_RVEC_ROUNDTRIP if rvec else 0)
    flags |= L.F_MINIMAL_EPNP5 if k == 5 else 0
    status = np.zeros(n_hyps, np.int8)
    med = np.zeros(n_hyps, np.float64)
    models = np.zeros((n_hyps, 16))
    with ctx.lock:
        L.check(L.lib().rsac_pnp_medians(ctx.handle, C.c_void_p(A.ptr), C.c_void_p(B.ptr), A.n, K9.ctypes.data,
                                         int(hyp_begin), int(n_hyps), int(seed) & (2**64 - 1), flags,
                                         None if sub is None else sub.ctypes.data, med.ctypes.data,
                                         status.ctypes.data, models.ctypes.data, _stream_of(A)))
    return status, med, models


def pnp_median(points2D, points3D, K, model12) -> float:
    """The LMedS score of one pose (R 9 row-major, then t) on the host (rsac_pnp_median_host, the
    arithmetic the GPU kernels run; no device needed): the median of the f32 squared reprojection
    errors over all points."""
    P3 = np.ascontiguousarray(np.asarray(points3D, np.float64).reshape(-1, 3))
    P2 = np.ascontiguousarray(np.asarray(points2D, np.float64).reshape(-1, 2))
    if P3.shape[0] != P2.shape[0]:
        raise ValueError("points3D and points2D differ in length")
    m12 = np.ascontiguousarray(np.asarray(model12, np.float64).reshape(-1)[:12])
    if m12.size != 12:
        raise ValueError("model12: 12 values (R row-major, then t) expected")
    med = C.c_double(0.0)
    L.check(L.lib().rsac_pnp_median_host(P3.ctypes.data, P2.ctypes.data, P3.shape[0], _K9(K).ctypes.data,
                                         m12.ctypes.data, C.byref(med)))
    return float(med.value)


def pnp_ransac_batched_flat(points2D, points3D, offsets, Ks, n_iters: int = 5000, reproj_thresh: float = 30.0, *,
                            confidence: float = 0.99, seed: int = 0x5EED, sampler: str = "philox",
                            adaptive: bool = True, refine: bool = True, device=None, minimal: str = "p3p",
                            dist=None, score: str = "count", exact_only: bool = False):
    """Batched PnP over problems already concatenated: points2D (N,2), points3D (N,3) f64 (numpy,
    or torch cuda tensors that stay on the device), offsets (P+1) int64, Ks (P,3,3).

    Returns (R (P,3,3), t (P,3), ok (P,) bool, n_inliers (P,), mask (N,) bool -- on the device
    for device inputs).  Same results as pnp_ransac_batched on the split lists.  Under
    score="msac" a sixth element follows: the winners' costs (P,) int64.  exact_only: the all-f64
    scoring kernel without the f32 pre-filter (A/B runs; implied by score="msac").
    """
    msac = _score_flag(score, "pnp_ransac_batched_flat", dist=dist)
    _no_dist(dist, "pnp_ransac_batched_flat")
    p3 = _In(points3D, 3)
    p2 = _In(points2D, 2)
    off = np.ascontiguousarray(np.asarray(offsets, np.int64).reshape(-1))
    P = off.size - 1
    if P < 1 or off[0] != 0 or off[-1] != p3.n or p2.n != p3.n:
        raise ValueError("offsets must run from 0 to the number of points")
    if np.diff(off).min() < 4:
        raise ValueError("every problem needs >= 4 correspondences")
    Kf = np.ascontiguousarray(np.asarray(Ks, np.float64).reshape(P, 9))
    ctx = L.context(_device_of(p3, device))
    flags = _flags(adaptive, refine, sampler, exact_only, minimal=minimal) | (L.F_DEVICE_IN if p3.device else 0) | msac
    mask, mptr, mflag = _mask_buffer(p3, p3.n)
    flags |= mflag
    R = np.zeros((P, 9))
    t = np.zeros((P, 3))
    status = np.zeros(P, np.int32)
    ninl = np.zeros(P, np.int32)
    with ctx.lock:
        L.check(L.lib().rsac_pnp_ransac_batched(ctx.handle, C.c_void_p(p3.ptr), C.c_void_p(p2.ptr), off.ctypes.data, P,
                                                Kf.ctypes.data, int(n_iters), float(reproj_thresh), float(confidence),
                                                int(seed) & (2**64 - 1), flags, R.ctypes.data, t.ctypes.data,
                                                status.ctypes.data, ninl.ctypes.data, C.c_void_p(mptr),
                                                _stream_of(p3)))
        costs = _last_costs(ctx, P) if msac else None
    out = (R.reshape(P, 3, 3), t, status == L.OK, ninl, _finish_mask(mask, p3.n))
    return out + (costs,) if msac else out


def pnp_ransac_batched_rows(points2D, points3D, offsets, Ks, n_iters: int = 5000, reproj_thresh: float = 30.0, *,
                            confidence: float = 0.99, seed: int = 0x5EED, sampler: str = "philox",
                            adaptive: bool = True, refine: bool = True, device=None, minimal: str = "p3p",
                            dist=None, score: str = "count"):
    """pnp_ransac_batched_flat with the results as one (P, 14) float64 tensor of rows (ok, n_inliers,
    R 9, t 3) on the device, written there by the library (rsac_pnp_ransac_batched_rows): the
    multi-GPU problem shards all-gather them with no host arrays in between.  Inputs as
    pnp_ransac_batched_flat (device tensors stay on the device) -> (rows, mask)."""
    _score_flag(score, "pnp_ransac_batched_rows", supported=False)
    _no_dist(dist, "pnp_ransac_batched_rows")
    import torch
    p3 = _In(points3D, 3)
    p2 = _In(points2D, 2)
    off = np.ascontiguousarray(np.asarray(offsets, np.int64).reshape(-1))
    P = off.size - 1
    if P < 1 or off[0] != 0 or off[-1] != p3.n or p2.n != p3.n:
        raise ValueError("offsets must run from 0 to the number of points")
    if np.diff(off).min() < 4:
        raise ValueError("every problem needs >= 4 correspondences")
    Kf = np.ascontiguousarray(np.asarray(Ks, np.float64).reshape(P, 9))
    dev = _device_of(p3, device)
    ctx = L.context(dev)
    flags = _flags(adaptive, refine, sampler, minimal=minimal) | (L.F_DEVICE_IN if p3.device else 0)
    mask, mptr, mflag = _mask_buffer(p3, p3.n)
    flags |= mflag
    rows = torch.empty((P, 14), dtype=torch.float64, device=torch.device("cuda", dev))
    stream = _stream_of(p3) if p3.device else C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream)
    with ctx.lock:
        L.check(L.lib().rsac_pnp_ransac_batched_rows(ctx.handle, C.c_void_p(p3.ptr), C.c_void_p(p2.ptr),
                                                     off.ctypes.data, P, Kf.ctypes.data, int(n_iters),
                                                     float(reproj_thresh), float(confidence), int(seed) & (2**64 - 1),
                                                     flags, C.c_void_p(rows.data_ptr()), C.c_void_p(mptr), stream))
    return rows, _finish_mask(mask, p3.n)


def homography_ransac_batched(src_list, dst_list, reproj_thresh: float = 3.0, *, max_iters: int = 2000,
                              confidence: float = 0.995, seed: int = 0x5EED, sampler: str = "opencv",
                              adaptive: bool = True, refine: bool = True, device: int = 0, score: str = "count"):
    """P independent findHomography calls in one launch sequence (main_v1.py:274-284)
    -> [(H | None, mask, n_inliers)]; under score="msac" each tuple ends with the winner's cost (int,
    -1 without a model or for a 4-point problem's direct model)."""
    msac = _score_flag(score, "homography_ransac_batched")
    s, off = _concat(src_list, 2)
    d, off2 = _concat(dst_list, 2)
    if not np.array_equal(off, off2):
        raise ValueError("per-problem src/dst counts differ")
    P = len(off) - 1
    if P and np.diff(off).min() < 4:
        raise ValueError("every problem needs >= 4 correspondences")
    ctx = L.context(device)
    flags = _flags(adaptive, refine, sampler) | msac
    H = np.zeros((P, 9))
    status = np.zeros(P, np.int32)
    ninl = np.zeros(P, np.int32)
    mask = np.zeros(max(int(off[-1]), 1), np.uint8)
    with ctx.lock:
        L.check(L.lib().rsac_homography_ransac_batched(ctx.handle, s.ctypes.data, d.ctypes.data, off.ctypes.data, P,
                                                       int(max_iters), float(reproj_thresh), float(confidence),
                                                       int(seed) & (2**64 - 1), flags, H.ctypes.data,
                                                       status.ctypes.data, ninl.ctypes.data, mask.ctypes.data, None))
        costs = _last_costs(ctx, P) if msac else None
    out = []
    for p in range(P):
        ok = status[p] == L.OK
        row = (H[p].reshape(3, 3) if ok else None, mask[off[p]:off[p + 1]].astype(bool), int(ninl[p]))
        out.append(row + (int(costs[p]),) if msac else row)
    return out


def homography_costs(src, dst, hyp_begin: int = 0, n_hyps: int = 1024, reproj_thresh: float = 3.0, *,
                     seed: int = 0x5EED, subsets=None, device=None):
    """Raw per-hypothesis (status, counts, models, costs) of the homography MSAC path for one problem
    (rsac_homography_hypotheses_msac): hypotheses("homography", ...) plus the int64 MSAC costs (-1
    without a model).  subsets: optional (n_hyps, 4) int32 index table replacing the Philox draw."""
    A = _In(src, 2)
    B = _In(dst, 2)
    if A.n != B.n:
        raise ValueError("src and dst differ in length")
    n_hyps = int(n_hyps)
    sub = None if subsets is None else np.ascontiguousarray(np.asarray(subsets, np.int32).reshape(n_hyps, 4))
    ctx = L.context(_device_of(A, device))
    counts = np.zeros(n_hyps, np.int32)
    status = np.zeros(n_hyps, np.int8)
    models = np.zeros((n_hyps, 16))
    cost = np.zeros(n_hyps, np.int64)
    with ctx.lock:
        L.check(L.lib().rsac_homography_hypotheses_msac(
            ctx.handle, C.c_void_p(A.ptr), C.c_void_p(B.ptr), A.n, int(hyp_begin), n_hyps, float(reproj_thresh),
            int(seed) & (2**64 - 1), L.F_DEVICE_IN if A.device else 0, None if sub is None else sub.ctypes.data,
            counts.ctypes.data, status.ctypes.data, models.ctypes.data, cost.ctypes.data, _stream_of(A)))
    return status, counts, models, cost


def fundamental_costs(pts1, pts2, hyp_begin: int = 0, n_hyps: int = 1024, reproj_thresh: float = 1.5, *,
                      seed: int = 0x5EED, device=None, minimal: str = "8pt"):
    """Raw per-hypothesis (status, counts, models, costs) of the fundamental-matrix MSAC path for one
    problem (rsac_fundamental_hypotheses_msac): hypotheses("fundamental", ..., exact_only=True) plus
    the int64 MSAC costs (-1 without a model).  minimal="7pt": n_hyps samples, 3 * n_hyps rows."""
    A = _In(pts1, 2)
    B = _In(pts2, 2)
    if A.n != B.n:
        raise ValueError("pts1 and pts2 differ in length")
    n_hyps = int(n_hyps)
    mflag7, sk = _fm_minimal(minimal, "fundamental_costs")
    rows = 3 * n_hyps if sk == 7 else n_hyps
    ctx = L.context(_device_of(A, device))
    counts = np.zeros(rows, np.int32)
    status = np.zeros(rows, np.int8)
    models = np.zeros((rows, 16))
    cost = np.zeros(rows, np.int64)
    with ctx.lock:
        L.check(L.lib().rsac_fundamental_hypotheses_msac(
            ctx.handle, C.c_void_p(A.ptr), C.c_void_p(B.ptr), A.n, int(hyp_begin), n_hyps, float(reproj_thresh),
            int(seed) & (2**64 - 1), (L.F_DEVICE_IN if A.device else 0) | mflag7, counts.ctypes.data, status.ctypes.data,
            models.ctypes.data, cost.ctypes.data, _stream_of(A)))
    return status, counts, models, cost


def score_poses(points2D, points3D, K, poses, reproj_thresh: float = 30.0, device=None, exact_only: bool = False,
                *, dist=None, costs: bool = False):
    """Inlier counts of given poses ((H, 3, 4) [R | t] or (H, 12)) -- the minimal scoring slice.
    dist: lens distortion coefficients (4, 5 or 8): the raw pixels against the distorted projection.
    costs=True: -> (counts, costs), the int64 MSAC costs beside the counts of the all-f64 test."""
    p3 = _In(points3D, 3)
    p2 = _In(points2D, 2)
    poses = np.asarray(poses, np.float64)
    if poses.ndim == 3:
        poses = np.concatenate([poses[:, :, :3].reshape(-1, 9), poses[:, :, 3]], axis=1)
    poses = np.ascontiguousarray(poses.reshape(-1, 12))
    ctx = L.context(_device_of(p3, device))
    flags = (L.F_DEVICE_IN if p3.device else 0) | (L.F_EXACT_ONLY if exact_only else 0)
    counts = np.zeros(poses.shape[0], np.int32)
    K9 = _K9(K)
    d, nd = _dist_arg(dist)
    if costs and d is not None:
        raise NotImplementedError("score_poses: costs=True with dist (lens distortion) is not built")
    if costs:
        cost = np.zeros(poses.shape[0], np.int64)
        with ctx.lock:
            L.check(L.lib().rsac_score_poses_msac(ctx.handle, C.c_void_p(p3.ptr), C.c_void_p(p2.ptr), p3.n,
                                                  K9.ctypes.data, poses.ctypes.data, poses.shape[0],
                                                  float(reproj_thresh), flags, counts.ctypes.data, cost.ctypes.data,
                                                  _stream_of(p3)))
        return counts, cost
    with ctx.lock:
        if d is not None:
            L.check(L.lib().rsac_score_poses_dist(ctx.handle, C.c_void_p(p3.ptr), C.c_void_p(p2.ptr), p3.n,
                                                  K9.ctypes.data, d.ctypes.data, nd, poses.ctypes.data,
                                                  poses.shape[0], float(reproj_thresh), flags, counts.ctypes.data,
                                                  _stream_of(p3)))
        else:
            L.check(L.lib().rsac_score_poses(ctx.handle, C.c_void_p(p3.ptr), C.c_void_p(p2.ptr), p3.n,
                                             K9.ctypes.data, poses.ctypes.data, poses.shape[0], float(reproj_thresh),
                                             flags, counts.ctypes.data, _stream_of(p3)))
    return counts


def _seen_inputs(p3, p2, points3D, points2D):
    """What evaluate_range's set-up reuse remembers of a call's inputs: the caller's two device
    tensors and their _version counters, or None where reuse is impossible -- host inputs, inputs
    the wrapper had to copy or convert (the copy is another tensor at every call), and inference
    tensors, which track no version."""
    if not (p3.device and p2.device and p3.keep is points3D and p2.keep is points2D):
        return None
    if p3.keep.is_inference() or p2.keep.is_inference():
        return None
    return (p3.keep, p2.keep, p3.keep._version, p2.keep._version)


def _unchanged_flag(ctx, seen) -> int:
    """F_POINTS_UNCHANGED when `seen` is what the context saw at its last call; the context then
    remembers `seen` once the call has returned (the caller holds ctx.lock).  Until then, and after a
    call that cannot be reused, it holds no tensor."""
    last, ctx.last_in = ctx.last_in, None
    if (seen is not None and last is not None and last[0] is seen[0] and last[1] is seen[1]
            and last[2] == seen[2] and last[3] == seen[3]):
        return L.F_POINTS_UNCHANGED
    return 0


def evaluate_range(points2D, points3D, K, hyp_begin: int, n_hyps: int, reproj_thresh: float = 30.0, *,
                   seed: int = 0x5EED, device=None, return_info: bool = False, exact_only: bool = False,
                   with_mask: bool = False, device_result: bool = False, context=None, reuse_setup: bool = True):
    """Evaluate Philox hypotheses [hyp_begin, hyp_begin + n_hyps) of one problem.

    Returns (key, model12[, mask][, info]) where key = (count << 32) | (0xFFFFFFFF - best_index)
    (or -1) and mask is the best hypothesis' RANSAC-phase mask (with_mask=True; on the GPU for
    GPU inputs).  The sharded driver (rsac.parallel) all-reduces the key with MAX.

    device_result=True (GPU tensor inputs): nothing waits for the GPU; key is a 1-element int64
    tensor (raw packed key, 0 = no model) and model12 a float64 tensor, both on the device.
    context: an rsac Context of its own (default: the device's shared one) -- calls on different
    contexts and torch streams may run concurrently (each context has its own device scratch).

    reuse_setup (GPU tensor inputs): successive calls on one context with the same two tensor
    objects, K, threshold and stream do not repeat the per-problem set-up (the f32 conversion, the
    scorer's point operands, the frame) when neither tensor's ``_version`` counter has moved since
    the context's last call (F_POINTS_UNCHANGED of include/rsac.h); every in-place torch operation
    moves it, and the context keeps a reference to both tensors until its next call.  Inputs the
    wrapper has to copy (another dtype or layout) and inference-mode tensors (no version counter)
    are never reused, and the context then holds no reference.  Writes torch does not see -- a
    foreign kernel on the raw pointer, a DLPack consumer -- leave ``_version`` alone: after such a
    write pass reuse_setup=False once (or always).  The results are the same bits either way.
    """
    p3 = _In(points3D, 3)
    p2 = _In(points2D, 2)
    if device_result and not p3.device:
        raise ValueError("device_result needs GPU tensor inputs")
    ctx = context if context is not None else L.context(_device_of(p3, device))
    flags = (L.F_DEVICE_IN if p3.device else 0) | (L.F_EXACT_ONLY if exact_only else 0)
    seen = _seen_inputs(p3, p2, points3D, points2D) if reuse_setup else None
    K9 = _K9(K)
    st = L.Stats()
    mask = mptr = None
    if with_mask:
        mask, mptr, mflag = _mask_buffer(p3, p3.n)
        flags |= mflag
    if device_result:
        import torch
        dev = p3.keep.device
        key_t = torch.empty(1, dtype=torch.int64, device=dev)  # written by the call (no fill launch)
        model_t = torch.empty(12, dtype=torch.float64, device=dev)
        with ctx.lock:
            flags |= _unchanged_flag(ctx, seen)
            L.check(L.lib().rsac_pnp_evaluate_range(ctx.handle, C.c_void_p(p3.ptr), C.c_void_p(p2.ptr), p3.n,
                                                    K9.ctypes.data, int(hyp_begin), int(n_hyps),
                                                    float(reproj_thresh), int(seed) & (2**64 - 1),
                                                    flags | L.F_ASYNC,
                                                    C.cast(key_t.data_ptr(), C.POINTER(C.c_int64)),
                                                    C.c_void_p(model_t.data_ptr()),
                                                    C.c_void_p(mptr) if with_mask else None, C.byref(st),
                                                    _stream_of(p3)))
            ctx.last_in = seen
        out = (key_t, model_t)
        return out + (_finish_mask(mask, p3.n),) if with_mask else out
    key = C.c_int64(-1)
    model = np.zeros(12)
    with ctx.lock:
        flags |= _unchanged_flag(ctx, seen)
        code = L.check(L.lib().rsac_pnp_evaluate_range(ctx.handle, C.c_void_p(p3.ptr), C.c_void_p(p2.ptr), p3.n,
                                                       K9.ctypes.data, int(hyp_begin), int(n_hyps),
                                                       float(reproj_thresh), int(seed) & (2**64 - 1), flags,
                                                       C.byref(key), model.ctypes.data,
                                                       C.c_void_p(mptr) if with_mask else None, C.byref(st),
                                                       _stream_of(p3)))
        ctx.last_in = seen
    out = (int(key.value), model)
    if with_mask:
        out = out + (_finish_mask(mask, p3.n),)
    if return_info:
        out = out + (_info(code, st),)
    return out


def hypothesis_rows(points2D, points3D, K, hyp_begin: int, n_hyps: int, reproj_thresh: float, rows, *,
                    seed: int = 0x5EED):
    """{status, count} int32 rows of Philox hypotheses [hyp_begin, hyp_begin + n_hyps) written into
    the device tensor ``rows`` (at least (n_hyps, 2) int32, contiguous) on the inputs' stream, without
    waiting -- the multi-GPU round's exchange format (rsac_pnp_hypothesis_rows)."""
    import torch
    p3 = _In(points3D, 3)
    p2 = _In(points2D, 2)
    if not (p3.device and rows.is_cuda and rows.dtype == torch.int32 and rows.is_contiguous()
            and rows.shape[0] >= n_hyps and rows.shape[-1] == 2):
        raise ValueError("hypothesis_rows needs GPU tensor inputs and an (n, 2) int32 contiguous device tensor")
    ctx = L.context(_device_of(p3, None))
    with ctx.lock:
        L.check(L.lib().rsac_pnp_hypothesis_rows(ctx.handle, C.c_void_p(p3.ptr), C.c_void_p(p2.ptr), p3.n,
                                                 _K9(K).ctypes.data, int(hyp_begin), int(n_hyps),
                                                 float(reproj_thresh), int(seed) & (2**64 - 1),
                                                 L.F_DEVICE_IN | L.F_DEVICE_OUT, C.c_void_p(rows.data_ptr()),
                                                 _stream_of(p3)))
    return rows


def winner(points2D, points3D, K, key, reproj_thresh: float = 30.0, *, seed: int = 0x5EED, with_mask: bool = True,
           context=None):
    """Re-derive the hypothesis named by a device packed key (e.g. after an all-reduce) on this
    GPU: (model12 tensor, mask tensor) without a host round trip (rsac_pnp_winner).  context: as
    evaluate_range."""
    import torch
    p3 = _In(points3D, 3)
    p2 = _In(points2D, 2)
    if not p3.device:
        raise ValueError("winner() needs GPU tensor inputs")
    ctx = context if context is not None else L.context(_device_of(p3, None))
    dev = p3.keep.device
    model_t = torch.zeros(12, dtype=torch.float64, device=dev)
    mask_t = torch.empty(max(p3.n, 1), dtype=torch.uint8, device=dev) if with_mask else None
    K9 = _K9(K)
    with ctx.lock:
        L.check(L.lib().rsac_pnp_winner(ctx.handle, C.c_void_p(p3.ptr), C.c_void_p(p2.ptr), p3.n, K9.ctypes.data,
                                        float(reproj_thresh), int(seed) & (2**64 - 1), C.c_void_p(key.data_ptr()),
                                        C.c_void_p(model_t.data_ptr()),
                                        C.c_void_p(mask_t.data_ptr()) if with_mask else None, _stream_of(p3)))
    return model_t, (_finish_mask(mask_t, p3.n) if with_mask else None)


def hypotheses(model: str, a, b, K=None, hyp_begin: int = 0, n_hyps: int = 1024, reproj_thresh: float = 30.0, *,
               seed: int = 0x5EED, subsets=None, device=None, exact_only: bool = False, minimal: str = "p3p",
               rvec=None, dist=None, costs: bool = False, medians: bool = False, K2=None):
    """Raw per-hypothesis (status, counts, models) of the GPU hot path for one problem.

    model "essential" (DESIGN.md §24): a = pts1, b = pts2 (N,2) pixels (or float32 (2,N) device
    tensors), K required, K2 optional: hyp_begin and n_hyps count five-point samples and every
    output has 10 * n_hyps rows, rows 10 s .. 10 s + 9 the models F = K2^-T E K^-1 of sample s in
    ascending root order (status 0 past its model count); costs=True appends the int64 MSAC costs
    and runs the exact path.  No subsets, medians, minimal or dist.

    medians=True (models "homography" and "fundamental"): -> (status, medians, models), the f64 LMedS
    medians (-1.0 without a model) in place of the counts (rsac_homography_medians /
    rsac_fundamental_medians; reproj_thresh is not used).

    costs=True (model "pnp", no dist): -> (status, counts, models, costs), the int64 MSAC costs
    (-1 without a model) beside the counts of the all-f64 test (rsac_pnp_hypotheses_msac).

    model "pnp": a = points3D (N,3), b = points2D (N,2), K required.
    model "homography": a = src (N,2), b = dst (N,2).
    model "fundamental": a = pts1 (N,2), b = pts2 (N,2); minimal="7pt"  runs the 7-point
    solver: hyp_begin and n_hyps then count samples and every output has 3 * n_hyps rows, rows 3s,
    3s + 1, 3s + 2 the models of sample s in ascending root order (status 0 past its model count).
    subsets: optional (n_hyps, 4) int32 index table replacing the Philox draw ((n_hyps, 5) for
    minimal="epnp5", PnP's 5-point EPnP kernel).  rvec: PnP models through Rodrigues(Rodrigues(R));
    the default (None) is on exactly when subsets are given, as pnp_ransac(sampler="opencv") scores
    OpenCV's MWC subsets, so the probe returns the rotations that run scores.
    dist (model "pnp" only): lens distortion coefficients (4, 5 or 8): the models are solved on the
    undistorted (ideal) pixels, the counts are those of the distorted test on the raw pixels.
    """
    if model == "essential":
        if subsets is not None or medians or dist is not None or minimal != "p3p":
            raise NotImplementedError("hypotheses('essential', ...): no subsets, medians, dist or minimal")
        return _essential_hypotheses(a, b, K, K2, hyp_begin, n_hyps, reproj_thresh, seed, device, exact_only, costs)
    if rvec is None:
        rvec = subsets is not None
    pnp = model == "pnp"
    if model not in ("pnp", "homography", "fundamental"):
        raise ValueError(f"unknown model {model!r}")
    d, nd = _dist_arg(dist)
    if d is not None and not pnp:
        raise NotImplementedError(f"hypotheses: dist with model {model!r} (lens distortion is built for PnP only)")
    if costs and (not pnp or d is not None):
        raise NotImplementedError("hypotheses: costs=True is built for model 'pnp' without dist "
                                  "(homography_costs and fundamental_costs return the other models' costs)")
    if medians and pnp:
        raise NotImplementedError("hypotheses: medians=True is built for models 'homography' and 'fundamental'")
    if medians and model == "fundamental" and subsets is not None:
        raise ValueError("hypotheses: the fundamental-matrix sampler is Philox only (no subsets)")
    A = _In(a, 3 if pnp else 2)
    B = _In(b, 2)
    ctx = L.context(_device_of(A, device))
    flags = (L.F_DEVICE_IN if A.device else 0) | (L.F_EXACT_ONLY if exact_only else 0)
    flags |= L.F_RVEC_ROUNDTRIP if (rvec and pnp) else 0
    k = 4
    rows = int(n_hyps)  # output rows: 3 per sample under minimal="7pt"
    if minimal in ("8pt", "7pt"):
        if model != "fundamental":
            raise ValueError(f"minimal={minimal!r} is a fundamental-matrix solver")
        if minimal == "7pt":
            flags |= L.F_FM_7POINT
            rows = 3 * int(n_hyps)
    elif minimal == "epnp5":
        if not pnp:
            raise ValueError("minimal='epnp5' is a PnP kernel")
        flags |= L.F_MINIMAL_EPNP5
        k = 5
    elif minimal != "p3p":
        raise ValueError(f"minimal must be 'p3p' or 'epnp5' (model 'fundamental': '8pt' or '7pt'), got {minimal!r}")
    counts = np.zeros(rows, np.int32)
    status = np.zeros(rows, np.int8)
    models = np.zeros((rows, 16))
    sub = None if subsets is None else np.ascontiguousarray(np.asarray(subsets, np.int32).reshape(n_hyps, k))
    if medians:
        if exact_only:
            raise ValueError("hypotheses: exact_only does not apply to medians=True")
        med = np.zeros(rows, np.float64)
        if model == "fundamental":
            with ctx.lock:
                L.check(L.lib().rsac_fundamental_medians(ctx.handle, C.c_void_p(A.ptr), C.c_void_p(B.ptr), A.n,
                                                         int(hyp_begin), int(n_hyps), int(seed) & (2**64 - 1), flags,
                                                         med.ctypes.data, status.ctypes.data, models.ctypes.data,
                                                         _stream_of(A)))
            return status, med, models
        with ctx.lock:
            L.check(L.lib().rsac_homography_medians(ctx.handle, C.c_void_p(A.ptr), C.c_void_p(B.ptr), A.n,
                                                    int(hyp_begin), int(n_hyps), int(seed) & (2**64 - 1), flags,
                                                    None if sub is None else sub.ctypes.data, med.ctypes.data,
                                                    status.ctypes.data, models.ctypes.data, _stream_of(A)))
        return status, med, models
    if costs:
        cost = np.zeros(n_hyps, np.int64)
        K9 = _K9(K)
        with ctx.lock:
            L.check(L.lib().rsac_pnp_hypotheses_msac(ctx.handle, C.c_void_p(A.ptr), C.c_void_p(B.ptr), A.n,
                                                     K9.ctypes.data, int(hyp_begin), int(n_hyps), float(reproj_thresh),
                                                     int(seed) & (2**64 - 1), flags,
                                                     None if sub is None else sub.ctypes.data, counts.ctypes.data,
                                                     status.ctypes.data, models.ctypes.data, cost.ctypes.data,
                                                     _stream_of(A)))
        return status, counts, models, cost
    with ctx.lock:
        if pnp and d is not None:
            K9 = _K9(K)
            L.check(L.lib().rsac_pnp_hypotheses_dist(ctx.handle, C.c_void_p(A.ptr), C.c_void_p(B.ptr), A.n,
                                                     K9.ctypes.data, d.ctypes.data, nd, int(hyp_begin), int(n_hyps),
                                                     float(reproj_thresh), int(seed) & (2**64 - 1), flags,
                                                     None if sub is None else sub.ctypes.data, counts.ctypes.data,
                                                     status.ctypes.data, models.ctypes.data, _stream_of(A)))
        elif pnp:
            K9 = _K9(K)
            L.check(L.lib().rsac_pnp_hypotheses(ctx.handle, C.c_void_p(A.ptr), C.c_void_p(B.ptr), A.n, K9.ctypes.data,
                                                int(hyp_begin), int(n_hyps), float(reproj_thresh),
                                                int(seed) & (2**64 - 1), flags,
                                                None if sub is None else sub.ctypes.data, counts.ctypes.data,
                                                status.ctypes.data, models.ctypes.data, _stream_of(A)))
        elif model == "fundamental":
            L.check(L.lib().rsac_fundamental_hypotheses(ctx.handle, C.c_void_p(A.ptr), C.c_void_p(B.ptr), A.n,
                                                        int(hyp_begin), int(n_hyps), float(reproj_thresh),
                                                        int(seed) & (2**64 - 1), flags, counts.ctypes.data,
                                                        status.ctypes.data, models.ctypes.data, _stream_of(A)))
        else:
            L.check(L.lib().rsac_homography_hypotheses(ctx.handle, C.c_void_p(A.ptr), C.c_void_p(B.ptr), A.n,
                                                       int(hyp_begin), int(n_hyps), float(reproj_thresh),
                                                       int(seed) & (2**64 - 1), flags,
                                                       None if sub is None else sub.ctypes.data, counts.ctypes.data,
                                                       status.ctypes.data, models.ctypes.data, _stream_of(A)))
    return status, counts, models


def pose_mask(points2D, points3D, K, model12, reproj_thresh: float = 30.0, device=None, *, dist=None):
    """RANSAC-test mask (and count) of one pose model (R 9 row-major, t 3).
    dist: lens distortion coefficients (4, 5 or 8): the raw pixels against the distorted projection."""
    p3 = _In(points3D, 3)
    p2 = _In(points2D, 2)
    ctx = L.context(_device_of(p3, device))
    flags = L.F_DEVICE_IN if p3.device else 0
    mask, mptr, mflag = _mask_buffer(p3, p3.n)
    flags |= mflag
    cnt = C.c_int32(0)
    K9 = _K9(K)
    m12 = np.ascontiguousarray(np.asarray(model12, np.float64).reshape(12))
    d, nd = _dist_arg(dist)
    with ctx.lock:
        if d is not None:
            L.check(L.lib().rsac_pnp_mask_dist(ctx.handle, C.c_void_p(p3.ptr), C.c_void_p(p2.ptr), p3.n,
                                               K9.ctypes.data, d.ctypes.data, nd, m12.ctypes.data,
                                               float(reproj_thresh), flags, C.c_void_p(mptr), C.byref(cnt),
                                               _stream_of(p3)))
        else:
            L.check(L.lib().rsac_pnp_mask(ctx.handle, C.c_void_p(p3.ptr), C.c_void_p(p2.ptr), p3.n, K9.ctypes.data,
                                          m12.ctypes.data, float(reproj_thresh), flags, C.c_void_p(mptr),
                                          C.byref(cnt), _stream_of(p3)))
    return _finish_mask(mask, p3.n), int(cnt.value)


def _ideal_pixels(P2, K, dist):
    """raw pixels -> the ideal (undistorted) pixels the solvers run on, as float64 holding the f32
    values (host); P2 itself without distortion"""
    d, _ = _dist_arg(dist)
    if d is None:
        return P2
    return np.ascontiguousarray(undistort_points(P2, K, d, ideal=True).astype(np.float64))


def refine_pose(points2D, points3D, K, R, t, mask=None, max_iter: int = 20, *, dist=None):
    """LM refinement of (R, t) on host arrays (cv2.solvePnPRefineLM, main_v1.py:508) -> (R, t).
    dist: lens distortion coefficients: the points are undistorted first and the refit minimises
    the error on the ideal pixels (not the distorted residual OpenCV's LM uses)."""
    P3 = np.ascontiguousarray(np.asarray(points3D, np.float64).reshape(-1, 3))
    P2 = np.ascontiguousarray(np.asarray(points2D, np.float64).reshape(-1, 2))
    P2 = _ideal_pixels(P2, K, dist)
    Rr = np.ascontiguousarray(np.asarray(R, np.float64).reshape(9)).copy()
    tr = np.ascontiguousarray(np.asarray(t, np.float64).reshape(3)).copy()
    m = None if mask is None else np.ascontiguousarray(np.asarray(mask, np.uint8).reshape(-1))
    K9 = _K9(K)
    L.check(L.lib().rsac_pnp_refine(P3.ctypes.data, P2.ctypes.data, P3.shape[0], K9.ctypes.data,
                                    None if m is None else m.ctypes.data, Rr.ctypes.data, tr.ctypes.data,
                                    int(max_iter)))
    return Rr.reshape(3, 3), tr


def refine_pose_device(points2D, points3D, K, R, t, mask=None, device=None, *, dist=None):
    """cv2.solvePnPRefineLM (main_v1.py:508, testpro-K.py:122) on the GPU: LM from (R, t) over the
    (masked) correspondences -> (R, t).  Host arrays; the same bits as refine_pose (host).
    dist: as refine_pose (undistort first, refine on the ideal pixels)."""
    P3 = np.ascontiguousarray(np.asarray(points3D, np.float64).reshape(-1, 3))
    P2 = np.ascontiguousarray(np.asarray(points2D, np.float64).reshape(-1, 2))
    P2 = _ideal_pixels(P2, K, dist)
    if P3.shape[0] != P2.shape[0]:
        raise ValueError("points3D and points2D differ in length")
    Rr = np.ascontiguousarray(np.asarray(R, np.float64).reshape(9)).copy()
    tr = np.ascontiguousarray(np.asarray(t, np.float64).reshape(3)).copy()
    m = None if mask is None else np.ascontiguousarray(np.asarray(mask, np.uint8).reshape(-1))
    ctx = L.context(0 if device is None else int(device))
    with ctx.lock:
        L.check(L.lib().rsac_pnp_refine_lm(ctx.handle, P3.ctypes.data, P2.ctypes.data, P3.shape[0], _K9(K).ctypes.data,
                                           None if m is None else m.ctypes.data, Rr.ctypes.data, tr.ctypes.data, None))
    return Rr.reshape(3, 3), tr


def reprojection_errors(points3D, points2D, K, R, t, *, device=None, return_projection: bool = False, dist=None):
    """compute_reprojection_error (testpro-K.py:32-36) on the GPU: ||pixel - projectPoints(X)||_2
    per point, f64 throughout; dist: lens distortion coefficients (4, 5 or 8) of projectPoints.
    R (3,3) or a Rodrigues vector (3,), t (3,).
    GPU tensor inputs keep the outputs on the device.  -> errors (N,) [, projections (N, 2)]."""
    p3 = _In(points3D, 3)
    p2 = _In(points2D, 2)
    if p3.n != p2.n:
        raise ValueError("points3D and points2D differ in length")
    if p3.device != p2.device:
        raise ValueError("points3D and points2D must both be host arrays or both GPU tensors")
    r = np.asarray(R, np.float64)
    R9 = np.ascontiguousarray(rodrigues(r).reshape(9) if r.size == 3 else r.reshape(9))
    t3 = np.ascontiguousarray(np.asarray(t, np.float64).reshape(3))
    n = p3.n
    ctx = L.context(_device_of(p3, device))
    if p3.device:
        import torch
        err = torch.empty(max(n, 1), dtype=torch.float64, device=p3.keep.device)
        proj = torch.empty((max(n, 1), 2), dtype=torch.float64, device=p3.keep.device) if return_projection else None
        eptr, pptr = err.data_ptr(), (proj.data_ptr() if proj is not None else None)
        flags = L.F_DEVICE_IN
    else:
        err = np.zeros(max(n, 1))
        proj = np.zeros((max(n, 1), 2)) if return_projection else None
        eptr, pptr = err.ctypes.data, (proj.ctypes.data if proj is not None else None)
        flags = 0
    d, nd = _dist_arg(dist)
    with ctx.lock:
        if d is not None:
            L.check(L.lib().rsac_pnp_reprojection_errors_dist(ctx.handle, C.c_void_p(p3.ptr), C.c_void_p(p2.ptr), n,
                                                              _K9(K).ctypes.data, d.ctypes.data, nd, R9.ctypes.data,
                                                              t3.ctypes.data, flags,
                                                              C.c_void_p(pptr) if pptr else None, C.c_void_p(eptr),
                                                              _stream_of(p3)))
        else:
            L.check(L.lib().rsac_pnp_reprojection_errors(ctx.handle, C.c_void_p(p3.ptr), C.c_void_p(p2.ptr), n,
                                                         _K9(K).ctypes.data, R9.ctypes.data, t3.ctypes.data, flags,
                                                         C.c_void_p(pptr) if pptr else None, C.c_void_p(eptr),
                                                         _stream_of(p3)))
    return (err[:n], proj[:n]) if return_projection else err[:n]


def compute_reprojection_error(pos3d, pixels, K, dist_coeffs, rvec, tvec, *, dist=None):
    """The reference's helper (testpro-K.py:32-36) with its signature: projectPoints through the
    Rodrigues vector rvec (with the lens distortion dist_coeffs, 4 / 5 / 8 coefficients; dist= is
    the same argument by keyword), then the per-point L2 norm -- on the GPU (reprojection_errors)."""
    rv = np.asarray(rvec, np.float64).reshape(-1)
    R = rodrigues(rv) if rv.size == 3 else rv.reshape(3, 3)
    e = reprojection_errors(pos3d, pixels, K, R, tvec, dist=dist_coeffs if dist is None else dist)
    return e


def undistort_points(points2D, K, dist, *, device=None, ideal: bool = False):
    """cv2.undistortPoints' iteration (five rounds) on the f32-rounded pixels: (N, 2) raw pixels ->
    (N, 2) float64 normalised points, or with ideal=True the float32 ideal pixels (x fx + cx,
    y fy + cy) the solvers run on.  Host arrays run on the host (no GPU needed) unless device is
    given; a GPU tensor (float64) runs the kernel in place and returns a tensor.  The host and the
    kernel give the same bits."""
    p2 = _In(points2D, 2)
    d, nd = _dist_arg(dist)
    K9 = _K9(K)
    n = p2.n
    dptr = None if d is None else d.ctypes.data
    if p2.device:
        import torch
        out = torch.empty((max(n, 1), 2), dtype=torch.float32 if ideal else torch.float64, device=p2.keep.device)
        ctx = L.context(_device_of(p2, device))
        with ctx.lock:
            L.check(L.lib().rsac_undistort_points_device(ctx.handle, C.c_void_p(p2.ptr), n, K9.ctypes.data, dptr, nd,
                                                         L.F_DEVICE_IN, None if ideal else C.c_void_p(out.data_ptr()),
                                                         C.c_void_p(out.data_ptr()) if ideal else None,
                                                         _stream_of(p2)))
        return out[:n]
    out = np.zeros((max(n, 1), 2), np.float32 if ideal else np.float64)
    norm_ptr, ideal_ptr = (None, out.ctypes.data) if ideal else (out.ctypes.data, None)
    if device is None:
        L.check(L.lib().rsac_undistort_points(C.c_void_p(p2.ptr), n, K9.ctypes.data, dptr, nd, norm_ptr, ideal_ptr))
    else:
        ctx = L.context(int(device))
        with ctx.lock:
            L.check(L.lib().rsac_undistort_points_device(ctx.handle, C.c_void_p(p2.ptr), n, K9.ctypes.data, dptr, nd,
                                                         0, norm_ptr, ideal_ptr, None))
    return out[:n]


def project_points(points3D, K, dist, R, t):
    """cv2.projectPoints on the host (no GPU needed), f64: (N, 3) -> (N, 2) pixels through the
    lens distortion dist (4, 5 or 8 coefficients; None / zeros: the pinhole projection).
    R (3,3) or a Rodrigues vector (3,), t (3,)."""
    P3 = np.ascontiguousarray(np.asarray(points3D, np.float64).reshape(-1, 3))
    d, nd = _dist_arg(dist)
    r = np.asarray(R, np.float64)
    R9 = np.ascontiguousarray(rodrigues(r).reshape(9) if r.size == 3 else r.reshape(9))
    t3 = np.ascontiguousarray(np.asarray(t, np.float64).reshape(3))
    out = np.zeros((max(P3.shape[0], 1), 2))
    L.check(L.lib().rsac_project_points_dist(P3.ctypes.data, P3.shape[0], _K9(K).ctypes.data,
                                             None if d is None else d.ctypes.data, nd, R9.ctypes.data,
                                             t3.ctypes.data, out.ctypes.data))
    return out[:P3.shape[0]]


@dataclass
class OrientationResult:
    """Outputs of estimate_camera_orientation (testpro-K.py:39-162), one row per intrinsic."""
    rvec: np.ndarray | None          # (3, 1) solvePnPRefineLM's rotation vector (None: every K failed)
    tvec: np.ndarray | None          # (3, 1)
    best: int                        # index of the chosen K (-1: none)
    K: np.ndarray                    # (P, 3, 3) the candidates, loop order (focal outer, sensor inner)
    mean_error: np.ndarray           # (P,) mean inlier reprojection error (NaN: failed the gate)
    ok: np.ndarray                   # (P,) passed "success and >= 6 inliers" (testpro-K.py:77)
    n_inliers: np.ndarray            # (P,)
    rvec_initial: np.ndarray         # (P, 3) solvePnPRansac's rotation vectors
    tvec_initial: np.ndarray         # (P, 3)
    masks: np.ndarray                # (P, N) RANSAC-phase inlier masks
    focal_sensor: list               # (focal length, (sensor w, sensor h)) of every K
    ranking: list                    # (distance to the known origin, mean error, K index, camera origin), sorted

    @property
    def best_K(self):
        return self.K[self.best] if self.best >= 0 else None


def intrinsics_grid(focal_lengths, sensor_sizes, image_size):
    """The candidate intrinsics of testpro-K.py:58-70, in its loop order."""
    Ks, fs = [], []
    for focal_length in focal_lengths:
        for (sensor_width, sensor_height) in sensor_sizes:
            fx = focal_length / (sensor_width / image_size[0])
            fy = focal_length / (sensor_height / image_size[1])
            Ks.append(np.array([[fx, 0, image_size[0] / 2], [0, fy, image_size[1] / 2], [0, 0, 1]], np.float64))
            fs.append((focal_length, (sensor_width, sensor_height)))
    return np.stack(Ks), fs


def estimate_camera_orientation(pos3d, pixels, focal_lengths, sensor_sizes, image_size, known_camera_origin=None, *,
                                n_iters: int = 5000, reproj_thresh: float = 30.0, confidence: float = 0.99,
                                seed: int = 0x5EED, sampler: str = "opencv", minimal: str = "epnp5", refine="lm",
                                min_inliers: int = 6, device: int = 0, return_info: bool = False, rvec=None,
                                dist=None, score: str = "count"):
    """estimate_camera_orientation of testpro-K.py:39-125 as one GPU call sequence
    (rsac_pnp_orientation_sweep): solvePnPRansac under every candidate K (one batched launch), the
    mean inlier reprojection error of each on the device, the first K with the smallest, then
    solvePnPRefineLM of its pose on its inliers.  Returns (rvec, tvec) like the reference
    ((None, None) when every K failed), or the OrientationResult with return_info=True.

    The defaults are what testpro-K.py:72-75 executes: cv2.solvePnPRansac with no `flags`, i.e.
    SOLVEPNP_ITERATIVE -- EPnP on 5-point samples drawn from OpenCV's MWC stream
    (minimal="epnp5", sampler="opencv"), then the LM final solve on the inliers (refine="lm").
    minimal="p3p" / sampler="philox" run this project's benchmark kernel instead."""
    _score_flag(score, "estimate_camera_orientation", supported=False)
    _no_dist(dist, "estimate_camera_orientation")
    if int(min_inliers) < 3:
        raise ValueError("min_inliers must be >= 3 (solvePnPRefineLM needs 3 inliers)")
    P3 = np.ascontiguousarray(np.asarray(pos3d, np.float64).reshape(-1, 3))
    P2 = np.ascontiguousarray(np.asarray(pixels, np.float64).reshape(-1, 2))
    if P3.shape[0] != P2.shape[0]:
        raise ValueError("pos3d and pixels differ in length")
    Ks, fs = intrinsics_grid(focal_lengths, sensor_sizes, image_size)
    P, n = Ks.shape[0], P3.shape[0]
    K9 = np.ascontiguousarray(Ks.reshape(P, 9))
    best = C.c_int32(-1)
    mean = np.zeros(P)
    models = np.zeros((P, 12))
    status = np.zeros(P, np.int32)
    ninl = np.zeros(P, np.int32)
    masks = np.zeros((P, max(n, 1)), np.uint8)
    R, t = np.zeros(9), np.zeros(3)
    ctx = L.context(device)
    with ctx.lock:
        code = L.check(L.lib().rsac_pnp_orientation_sweep(
            ctx.handle, P3.ctypes.data, P2.ctypes.data, n, K9.ctypes.data, P, int(n_iters), float(reproj_thresh),
            float(confidence), int(seed) & (2**64 - 1), _flags(True, refine, sampler, minimal=minimal, rvec=rvec), int(min_inliers),
            C.byref(best), mean.ctypes.data, models.ctypes.data, status.ctypes.data, ninl.ctypes.data,
            masks.ctypes.data, R.ctypes.data, t.ctypes.data, None))
    ok = status == L.OK
    b = int(best.value)
    rvec = rodrigues(R.reshape(3, 3)).reshape(3, 1) if code == L.OK else None
    tvec = t.reshape(3, 1).copy() if code == L.OK else None
    if not return_info:
        return rvec, tvec
    rv0 = np.stack([rodrigues(models[k, :9].reshape(3, 3)).reshape(3) for k in range(P)])
    ranking = []
    if known_camera_origin is not None:
        o = np.asarray(known_camera_origin, np.float64).reshape(3)
        for k in np.flatnonzero(ok):
            Rk = rodrigues(rv0[k])
            origin = -Rk.T @ models[k, 9:12]
            ranking.append((float(np.linalg.norm(origin - o)), float(mean[k]), int(k), origin))
        ranking.sort(key=lambda x: x[0])  # testpro-K.py:103 (stable, as Python's sort)
    return OrientationResult(rvec=rvec, tvec=tvec, best=b, K=Ks, mean_error=mean, ok=ok, n_inliers=ninl,
                             rvec_initial=rv0, tvec_initial=models[:, 9:12].copy(), masks=masks[:, :n].astype(bool),
                             focal_sensor=fs, ranking=ranking)


def epnp_pose(points2D, points3D, K, mask=None):
    """EPnP on all (or the masked) points, cv2.solvePnP(..., flags=SOLVEPNP_EPNP) -> (R, t) or
    (None, None) for < 4 points / a planar cloud.  Host arrays; the same numbers as the device pass
    of pnp_ransac(refine="epnp")."""
    P3 = np.ascontiguousarray(np.asarray(points3D, np.float64).reshape(-1, 3))
    P2 = np.ascontiguousarray(np.asarray(points2D, np.float64).reshape(-1, 2))
    m = None if mask is None else np.ascontiguousarray(np.asarray(mask, np.uint8).reshape(-1))
    R, t = np.zeros(9), np.zeros(3)
    code = L.check(L.lib().rsac_pnp_epnp(P3.ctypes.data, P2.ctypes.data, P3.shape[0], _K9(K).ctypes.data,
                                         None if m is None else m.ctypes.data, R.ctypes.data, t.ctypes.data))
    return (R.reshape(3, 3), t) if code == L.OK else (None, None)


def epnp_minimal(points2D, points3D, K):
    """solvePnPRansac's default minimal solver on one 5-point sample, on the host: solvePnP(...,
    SOLVEPNP_EPNP) in OpenCV's operation sequence (rsac_cvepnp.h, the source the k_cvepnp5_*
    kernels run) -> (R, t).  Inputs are rounded to f32 like solvePnPRansac's CV_32F copies."""
    P3 = np.ascontiguousarray(np.asarray(points3D, np.float64).reshape(5, 3))
    P2 = np.ascontiguousarray(np.asarray(points2D, np.float64).reshape(5, 2))
    R, t = np.zeros(9), np.zeros(3)
    L.check(L.lib().rsac_pnp_epnp_minimal(P3.ctypes.data, P2.ctypes.data, _K9(K).ctypes.data, R.ctypes.data,
                                          t.ctypes.data))
    return R.reshape(3, 3), t


def _host_mask_arg(mask, n):
    m = np.ascontiguousarray(np.asarray(mask.cpu() if _is_torch(mask) else mask).reshape(-1) != 0, np.uint8)
    if m.shape[0] != n:
        raise ValueError("mask and points differ in length")
    return m


def _fit_mask_arg(inp, mask, n):
    """(pointer, keepalive) of a fit call's mask: on the device when the points are"""
    if mask is None:
        return None, None
    if inp.device:
        import torch
        keep = torch.as_tensor(mask, device=inp.keep.device).reshape(-1).ne(0).contiguous()
        if keep.shape[0] != n:
            raise ValueError("mask and points differ in length")
        return keep.data_ptr(), keep
    keep = _host_mask_arg(mask, n)
    return keep.ctypes.data, keep


def homography_fit(src, dst, mask=None, *, device=None):
    """Least-squares normalised DLT + LM on all (or masked) points -> H (findHomography method 0),
    or None without a model (fewer than 4 masked points, a zero deviation sum).

    NumPy inputs with device=None run the host twin (rsac_homography_fit, no GPU needed); torch
    device tensors ((n, 2), or float32 SoA of shape (2, n), with a device bool / uint8 mask) or
    device=<index> run the kernel (rsac_homography_fit_device).  Both return the same bits.
    """
    on_device = _is_torch(src) and src.is_cuda
    if not on_device and device is None:
        s = np.ascontiguousarray(np.asarray(src, np.float64).reshape(-1, 2))
        d = np.ascontiguousarray(np.asarray(dst, np.float64).reshape(-1, 2))
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask, np.uint8).reshape(-1))
        H = np.zeros(9)
        code = L.check(L.lib().rsac_homography_fit(s.ctypes.data, d.ctypes.data, s.shape[0],
                                                   None if m is None else m.ctypes.data, H.ctypes.data))
        return H.reshape(3, 3) if code == L.OK else None
    a = _hom_in(src)
    b = _hom_in(dst)
    if a.n != b.n:
        raise ValueError("src and dst differ in length")
    if a.device != b.device or _in_flags(a) != _in_flags(b):
        raise ValueError("src and dst must share one residence and layout")
    mptr, keep = _fit_mask_arg(a, mask, a.n)
    ctx = L.context(_device_of(a, device))
    H = np.zeros(9)
    with ctx.lock:
        code = L.check(L.lib().rsac_homography_fit_device(ctx.handle, C.c_void_p(a.ptr), C.c_void_p(b.ptr), a.n,
                                                          C.c_void_p(mptr), _in_flags(a), H.ctypes.data,
                                                          _stream_of(a)))
    del keep
    return H.reshape(3, 3) if code == L.OK else None


def homography_fit_batched(src_list, dst_list, mask_list=None, *, device=0):
    """homography_fit of P independent problems in one launch, one wave each
    (rsac_homography_fit_batched_device) -> [H (3,3) | None]; every H equals the single host fit."""
    s, off = _concat(src_list, 2)
    d, off2 = _concat(dst_list, 2)
    if not np.array_equal(off, off2):
        raise ValueError("per-problem src/dst counts differ")
    P = len(off) - 1
    if P < 1:
        return []
    m = None
    if mask_list is not None:
        if len(mask_list) != P:
            raise ValueError("mask_list and src_list differ in length")
        m = _concat_host_masks(mask_list, off)
    ctx = L.context(int(device))
    H = np.zeros((P, 9))
    status = np.zeros(P, np.int32)
    with ctx.lock:
        L.check(L.lib().rsac_homography_fit_batched_device(ctx.handle, s.ctypes.data, d.ctypes.data, off.ctypes.data, P,
                                                           None if m is None else m.ctypes.data, 0, H.ctypes.data,
                                                           status.ctypes.data, None))
    return [H[p].reshape(3, 3) if status[p] == L.OK else None for p in range(P)]


def homography_local_opt(src, dst, H, reproj_thresh: float = 3.0, *, max_rounds: int = 4, device=None):
    """Local optimisation of a homography on the GPU (rsac_homography_local_opt) ->
    (H (3,3), mask, count, steps).

    From H: the inlier mask at reproj_thresh (homography_ransac's test), homography_fit on it, the
    fit's mask, ... -- a round is accepted only when its inlier count rises strictly, at most
    max_rounds are accepted.  Returns the last accepted model (H itself after 0 steps), its mask
    and count, and the number of accepted rounds.  The mask stays on the device for device inputs.
    """
    thr = _lo_thresh_arg(reproj_thresh, max_rounds)
    H9 = np.ascontiguousarray(np.asarray(H, np.float64).reshape(-1))
    if H9.shape[0] != 9:
        raise ValueError("H must have 9 elements")
    a = _hom_in(src)
    b = _hom_in(dst)
    if a.n != b.n:
        raise ValueError("src and dst differ in length")
    if a.device != b.device or _in_flags(a) != _in_flags(b):
        raise ValueError("src and dst must share one residence and layout")
    if a.n < 1:
        raise ValueError("no points")
    ctx = L.context(_device_of(a, device))
    mask, mptr, mflag = _mask_buffer(a, a.n)
    Ho = np.zeros(9)
    cnt, steps = C.c_int32(0), C.c_int32(0)
    with ctx.lock:
        L.check(L.lib().rsac_homography_local_opt(ctx.handle, C.c_void_p(a.ptr), C.c_void_p(b.ptr), a.n,
                                                  H9.ctypes.data, thr, int(max_rounds), _in_flags(a) | mflag,
                                                  Ho.ctypes.data, C.byref(cnt), C.byref(steps), C.c_void_p(mptr),
                                                  _stream_of(a)))
    return Ho.reshape(3, 3), _finish_mask(mask, a.n), int(cnt.value), int(steps.value)


def rodrigues(src):
    """cv2.Rodrigues (main_v1.py:895): (3,) vector <-> (3, 3) matrix."""
    a = np.ascontiguousarray(np.asarray(src, np.float64))
    if a.size == 3:
        R = np.zeros(9)
        L.lib().rsac_rodrigues_v2m(a.reshape(3).ctypes.data, R.ctypes.data)
        return R.reshape(3, 3)
    if a.size == 9:
        r = np.zeros(3)
        L.lib().rsac_rodrigues_m2v(a.reshape(9).ctypes.data, r.ctypes.data)
        return r.reshape(3, 1)
    raise ValueError("Rodrigues expects a 3-vector or a 3x3 matrix")


def update_num_iters(p: float, ep: float, model_points: int, max_iters: int) -> int:
    """RANSACUpdateNumIters of OpenCV, as the driver applies it after every new best model."""
    return int(L.lib().rsac_update_num_iters(float(p), float(ep), int(model_points), int(max_iters)))


@dataclass
class LocationResult:
    """Outputs of rsac.location_search, one row per candidate camera location."""
    err: np.ndarray  # (L, 2) f64: err1, err2 (num_matches of main_v1.py:273; (0, 0) = no model)
    H: np.ndarray  # (L, 3, 3) findHomography's H (main_v1.py:312; M = inv(H) at :314)
    ok: np.ndarray  # (L,) bool
    n_inliers: np.ndarray  # (L,) int32
    mask: np.ndarray  # (L, n_good) bool, RANSAC-phase
    n_good: int  # features noted on the image
    cost: np.ndarray | None = None  # score="msac": (L,) int64 winners' costs (-1: none); None otherwise

    @property
    def best(self) -> int:
        """argmin of err2 with 0 -> 1e6, as main_v1.py:863-866 picks the camera location."""
        e2 = self.err[:, 1].copy()
        e2[e2 == 0] = 1000000
        return int(np.argmin(e2))


def location_search(pos3d, pixels, locations, ransacbound: float = 75.0, *, max_iters: int = 2000,
                    confidence: float = 0.995, sampler: str = "opencv", adaptive: bool = True, refine: bool = True,
                    device: int = 0, score: str = "count") -> LocationResult:
    """The camera-location search of find_homographies (main_v1.py:254-297) in one call.

    pos3d (N,3) feature positions, pixels (N,2) (rows (0,0) = not noted on the image,
    main_v1.py:304), locations (L,3) candidate camera positions.  For every location the
    homography RANSAC of find_homography (main_v1.py:300-312) and its err1/err2 score
    (main_v1.py:332-348, 419) run on the GPU.  score="msac": every location's RANSAC picks the
    hypothesis with the lowest truncated cost (DESIGN.md "MSAC scoring for homographies") and
    result.cost holds the winners' costs.
    """
    msac = _score_flag(score, "location_search")
    P3 = np.ascontiguousarray(np.asarray(pos3d, np.float64).reshape(-1, 3))
    P2 = np.ascontiguousarray(np.asarray(pixels, np.float64).reshape(-1, 2))
    LC = np.ascontiguousarray(np.asarray(locations, np.float64).reshape(-1, 3))
    if P3.shape[0] != P2.shape[0]:
        raise ValueError("pos3d and pixels differ in length")
    L_, n = LC.shape[0], P3.shape[0]
    n_good_max = int(np.count_nonzero((P2[:, 0] != 0) | (P2[:, 1] != 0)))
    err = np.zeros((L_, 2))
    H = np.zeros((L_, 9))
    st = np.zeros(L_, np.int32)
    ninl = np.zeros(L_, np.int32)
    mask = np.zeros(max(L_ * n_good_max, 1), np.uint8)
    ng = C.c_int32(0)
    ctx = L.context(device)
    with ctx.lock:
        L.check(L.lib().rsac_location_search(ctx.handle, P3.ctypes.data, P2.ctypes.data, n, LC.ctypes.data, L_,
                                             float(ransacbound), int(max_iters), float(confidence),
                                             _flags(adaptive, refine, sampler) | msac, H.ctypes.data, err.ctypes.data,
                                             st.ctypes.data, ninl.ctypes.data, mask.ctypes.data, C.byref(ng), None))
        cost = _last_costs(ctx, L_) if msac else None
    g = int(ng.value)
    return LocationResult(err=err, H=H.reshape(L_, 3, 3), ok=st == L.OK, n_inliers=ninl,
                          mask=mask[:L_ * g].reshape(L_, g).astype(bool), n_good=g, cost=cost)


def local_opt(points2D, points3D, K, model12, reproj_thresh: float = 30.0, device=None):
    """One LO-RANSAC local optimisation of a pose -> (model12, inlier count, steps)."""
    p3 = _In(points3D, 3)
    p2 = _In(points2D, 2)
    ctx = L.context(_device_of(p3, device))
    m_in = np.ascontiguousarray(np.asarray(model12, np.float64).reshape(12))
    m_out = np.zeros(12)
    cnt = C.c_int32(0)
    steps = C.c_int32(0)
    K9 = _K9(K)
    with ctx.lock:
        L.check(L.lib().rsac_pnp_local_opt(ctx.handle, C.c_void_p(p3.ptr), C.c_void_p(p2.ptr), p3.n, K9.ctypes.data,
                                           m_in.ctypes.data, float(reproj_thresh),
                                           L.F_DEVICE_IN if p3.device else 0, m_out.ctypes.data, C.byref(cnt),
                                           C.byref(steps), _stream_of(p3)))
    return m_out, int(cnt.value), int(steps.value)


def lmeds_num_iters(confidence: float = 0.995, max_iters: int = 2000, model_points: int = 4) -> int:
    """OpenCV's fixed LMedS hypothesis count: max(RANSACUpdateNumIters(confidence, 0.45, 4, max_iters), 3)"""
    return int(L.lib().rsac_lmeds_num_iters(float(confidence), int(model_points), int(max_iters)))


class LmedsScan:
    """The LMedS scan (rsac_scan_lmeds of include/rsac.h) over (status, median) rows in hypothesis
    order, fed in one piece or in chunks: `best` (-1: none), `best_median`, `iter`, `done`."""

    def __init__(self, n_iters: int):
        self.st = L.ScanLmedsState()
        L.lib().rsac_scan_lmeds_init(C.byref(self.st), int(n_iters))

    def step(self, status, medians):
        st = np.ascontiguousarray(status, np.int8)
        m = np.ascontiguousarray(medians, np.float64)
        if st.shape != m.shape:
            raise ValueError("status and medians differ in length")
        L.check(L.lib().rsac_scan_lmeds(C.byref(self.st), st.ctypes.data, m.ctypes.data, st.size))
        return self

    best = property(lambda self: int(self.st.best))
    best_median = property(lambda self: float(self.st.best_median))
    iter = property(lambda self: int(self.st.iter))
    done = property(lambda self: bool(self.st.done))


class Scan:
    """OpenCV's sequential best-model scan (rsac_scan of include/rsac.h) over counts produced
    elsewhere -- the multi-GPU driver feeds it each round's gathered counts."""

    def __init__(self, max_iters: int, n_points: int, confidence: float = 0.99, model_points: int = 4):
        self.st = L.ScanState()
        L.lib().rsac_scan_init(C.byref(self.st), int(max_iters))
        self.n = int(n_points)
        self.conf = float(confidence)
        self.s = int(model_points)

    def step(self, counts, status):
        c = np.ascontiguousarray(counts, np.int32)
        st = np.ascontiguousarray(status, np.int8)
        if c.shape != st.shape:
            raise ValueError("counts and status differ in length")
        L.check(L.lib().rsac_scan(C.byref(self.st), c.ctypes.data, st.ctypes.data, c.size, self.n, self.s, self.conf))
        return self

    def step_until_best(self, counts, status) -> int:
        """Scan until a new best (LO-RANSAC); returns how many entries were consumed (the
        new best is the last of them when ``improved``)."""
        c = np.ascontiguousarray(counts, np.int32)
        st = np.ascontiguousarray(status, np.int8)
        before = self.iters
        imp = C.c_int32(0)
        L.check(L.lib().rsac_scan_until_best(C.byref(self.st), c.ctypes.data, st.ctypes.data, c.size, self.n, self.s,
                                             self.conf, C.byref(imp)))
        self.improved = bool(imp.value)
        return self.iters - before

    def step_rows(self, rows, count: int, stop_on_improve: bool = False) -> int:
        """Consume the first ``count`` {status, count} rows of an (m, 2) int32 array or tensor (a
        gathered multi-GPU round).  GPU tensors are scanned on the device (rsac_scan_device: only
        the improvements come to the host).  Returns the rows consumed (``improved`` is set when
        stop_on_improve stopped at a new best)."""
        before = self.iters
        if _is_torch(rows) and rows.is_cuda:
            import torch
            r = rows[:count]
            if not r.is_contiguous() or r.dtype != torch.int32:
                r = r.to(torch.int32).contiguous()
            imp = C.c_int32(0)
            ctx = L.context(r.device.index)
            with ctx.lock:
                L.check(L.lib().rsac_scan_device(ctx.handle, C.byref(self.st), C.c_void_p(r.data_ptr()), int(count),
                                                 self.n, self.s, self.conf, 1 if stop_on_improve else 0, C.byref(imp),
                                                 C.c_void_p(torch.cuda.current_stream(r.device).cuda_stream)))
            self.improved = bool(imp.value)
            return self.iters - before
        a = np.asarray(rows.cpu() if _is_torch(rows) else rows)[:count]
        if stop_on_improve:
            return self.step_until_best(a[:, 1], a[:, 0].astype(np.int8))
        self.step(a[:, 1], a[:, 0].astype(np.int8))
        self.improved = False
        return self.iters - before

    def raise_count(self, count: int):
        """Apply a locally optimised inlier count."""
        L.check(L.lib().rsac_scan_raise(C.byref(self.st), int(count), self.n, self.s, self.conf))

    done = property(lambda self: bool(self.st.done))
    best = property(lambda self: int(self.st.best))
    max_good = property(lambda self: int(self.st.max_good))
    iters = property(lambda self: int(self.st.iter))
    niters = property(lambda self: int(self.st.niters))



# ---------------------------------------------------------------------------
# Essential matrix from five points
# ---------------------------------------------------------------------------
def _K2_arg(K2):
    """(pointer or None, keepalive) of the optional second view's intrinsics"""
    if K2 is None:
        return None, None
    k = _K9(K2)
    return k.ctypes.data, k


def _em_refine_arg(refine, what: str):
    if refine in (False, None):
        return False
    if refine is True:
        return True
    if isinstance(refine, str) and refine in ("pose", "lo"):
        return refine
    raise ValueError(f"{what}: refine must be False, True, 'pose' or 'lo', got {refine!r}")


def _lo_thresh_arg(reproj_thresh, max_rounds):
    """the threshold of a local optimisation, after the checks every family shares"""
    if int(max_rounds) < 1:
        raise ValueError("max_rounds must be >= 1")
    thr = float(reproj_thresh)
    if not (np.isfinite(thr) and thr > 0.0):
        raise ValueError("reproj_thresh must be finite and positive")
    return thr


def _E9(E, what="E"):
    e = np.ascontiguousarray(np.asarray(E.cpu() if _is_torch(E) else E, np.float64).reshape(-1))
    if e.shape[0] != 9:
        raise ValueError(f"{what} must have 9 elements")
    return e


def _model_rows(models, what):
    """the (P, 9) model rows of a batched call: None -> zeros (no model)"""
    rows = np.zeros((len(models), 9))
    for p, M in enumerate(models):
        if M is not None:
            rows[p] = _E9(M, what)
    return rows


def _per_problem_K(k, P, name):
    k = np.asarray(k, np.float64)
    if k.size == 9:
        k = np.broadcast_to(k.reshape(1, 9), (P, 9))
    elif k.size != 9 * P:
        raise ValueError(f"{name} must be (3,3) or (P,3,3)")
    return np.ascontiguousarray(k.reshape(P, 9))


@dataclass
class EssentialFitInfo:
    """What essential_refine(return_info=True) appends: the F of the E returned (K2^-T E K^-1 at unit
    norm), the final sum of squared Sampson residuals over the mask (px^2), the masked points and
    the accepted LM steps."""
    F: object
    cost: float
    count: int
    steps: int


def essential_to_fundamental(E, K, K2=None):
    """F = K2^-T E K^-1 at unit Frobenius norm (rsac_essential_to_fundamental; host only): the
    pixel-space matrix of an essential matrix by the formula the refit and the local optimisation
    use.  None for a zero or non-finite product."""
    E9 = _E9(E)
    K9 = _K9(K)
    k2p, k2keep = _K2_arg(K2)
    F = np.zeros(9)
    code = L.check(L.lib().rsac_essential_to_fundamental(E9.ctypes.data, K9.ctypes.data, k2p, F.ctypes.data))
    return F.reshape(3, 3) if code == L.OK else None


def essential_refine(pts1, pts2, K, E, mask=None, *, K2=None, device=None, return_info: bool = False):
    """The calibrated refit of an essential matrix -> E (3,3) at unit Frobenius norm, or
    None without a model.

    Levenberg-Marquardt on the Sampson residuals of F = K2^-T [t]x R K^-1 over the masked points
    (mask None = all), five parameters, started from the decomposition of E: the result is an
    essential matrix and the least-squares fit at once, and its cost is never above the start's.
    No model: fewer than 5 masked points, a non-finite coordinate under the mask, an E that is not
    finite or has rank < 2.  return_info=True -> (E, EssentialFitInfo).

    NumPy inputs with device=None run the host twin (rsac_essential_refine, no GPU needed); torch
    device tensors (with a device mask) or device=<index> run the kernel
    (rsac_essential_refine_device).  Both return the same bits; with a GPU at hand device=0 is the
    faster route for NumPy inputs as well (0.24 against 0.66 ms on 2000 matches)."""
    E9 = _E9(E)
    K9 = _K9(K)
    k2p, k2keep = _K2_arg(K2)
    Eo, Fo = np.zeros(9), np.zeros(9)
    cost, cnt, steps = C.c_double(0.0), C.c_int32(0), C.c_int32(0)
    on_device = _is_torch(pts1) and pts1.is_cuda
    if not on_device and device is None:
        a, b, _ = _fm_host_args(pts1.cpu() if _is_torch(pts1) else pts1, pts2.cpu() if _is_torch(pts2) else pts2,
                                np.zeros(9))
        m = None if mask is None else _host_mask_arg(mask, a.shape[0])
        code = L.check(L.lib().rsac_essential_refine(a.ctypes.data, b.ctypes.data, a.shape[0], K9.ctypes.data, k2p,
                                                     None if m is None else m.ctypes.data, E9.ctypes.data,
                                                     Eo.ctypes.data, Fo.ctypes.data, C.byref(cost), C.byref(cnt),
                                                     C.byref(steps)))
    else:
        a = _hom_in(pts1)
        b = _hom_in(pts2)
        if a.n != b.n:
            raise ValueError("pts1 and pts2 differ in length")
        if a.device != b.device:
            raise ValueError("pts1 and pts2 must both be on the host or both on the device")
        mptr, keep = _fit_mask_arg(a, mask, a.n)
        ctx = L.context(_device_of(a, device))
        with ctx.lock:
            code = L.check(L.lib().rsac_essential_refine_device(ctx.handle, C.c_void_p(a.ptr), C.c_void_p(b.ptr), a.n,
                                                                K9.ctypes.data, k2p, C.c_void_p(mptr), E9.ctypes.data,
                                                                _in_flags(a), Eo.ctypes.data, Fo.ctypes.data,
                                                                C.byref(cost), C.byref(cnt), C.byref(steps),
                                                                _stream_of(a)))
        del keep
    ok = code == L.OK
    out = Eo.reshape(3, 3) if ok else None
    if not return_info:
        return out
    return out, EssentialFitInfo(Fo.reshape(3, 3) if ok else None, float(cost.value), int(cnt.value), int(steps.value))


def essential_refine_batched(pts1_list, pts2_list, K, E_list, mask_list=None, *, K2=None, device=0,
                             return_info: bool = False, _batch=None):
    """essential_refine of P independent problems in one launch whatever P
    (rsac_essential_refine_batched_device) -> [E (3,3) | None]; every E has the bits of the single
    host refit of that problem.  K (and K2): (3,3) for every problem or (P,3,3).  E_list[p] None (or
    all zeros) and problems with fewer than 5 masked points give None.  Lists of device tensors (with
    device masks) are fitted in place.  return_info=True -> [(E, EssentialFitInfo)]."""
    bt = _batch if _batch is not None else _FmBatch(pts1_list, pts2_list, device)  # _batch: essential_ransac_batched's
    E_list = list(E_list)
    if len(E_list) != bt.P:
        raise ValueError("E_list and pts1_list differ in length")
    if bt.P < 1:
        return []
    Ein = _model_rows(E_list, "every E")
    K1s = _per_problem_K(K, bt.P, "K")
    K2s = None if K2 is None else _per_problem_K(K2, bt.P, "K2")
    mptr, keep = bt.masks_arg(mask_list)
    ctx = L.context(bt.device)
    Eo, Fo = np.zeros((bt.P, 9)), np.zeros((bt.P, 9))
    cost = np.zeros(bt.P)
    cnt, steps, status = np.zeros(bt.P, np.int32), np.zeros(bt.P, np.int32), np.zeros(bt.P, np.int32)
    with ctx.lock:
        L.check(L.lib().rsac_essential_refine_batched_device(
            ctx.handle, C.c_void_p(bt.ptrs[0]), C.c_void_p(bt.ptrs[1]), bt.off.ctypes.data, bt.P, K1s.ctypes.data,
            None if K2s is None else K2s.ctypes.data, C.c_void_p(mptr), Ein.ctypes.data, bt.flags, Eo.ctypes.data,
            Fo.ctypes.data, cost.ctypes.data, cnt.ctypes.data, steps.ctypes.data, status.ctypes.data, bt.stream()))
    del keep
    out = []
    for p in range(bt.P):
        ok = status[p] == L.OK
        E = Eo[p].reshape(3, 3) if ok else None
        if return_info:
            out.append((E, EssentialFitInfo(Fo[p].reshape(3, 3) if ok else None, float(cost[p]), int(cnt[p]),
                                            int(steps[p]))))
        else:
            out.append(E)
    return out


def essential_local_opt(pts1, pts2, K, E, reproj_thresh: float = 1.0, *, K2=None, max_rounds: int = 4, device=None):
    """Local optimisation of an essential matrix on the GPU (rsac_essential_local_opt) ->
    (E (3,3) | None, mask, count, steps).

    From E: the inlier mask of K2^-T E K^-1 at reproj_thresh (essential_ransac's test), the
    calibrated refit (essential_refine) from E on it, the refit's mask, ... -- a round is accepted
    only when its inlier count rises strictly, at most max_rounds are accepted.  Returns the last
    accepted model (E itself after 0 steps), its mask and count, and the number of accepted rounds;
    an E the refit cannot start from (zeros, non-finite, rank < 2) gives (None, zero mask, 0, 0).
    The mask stays on the device for device inputs."""
    thr = _lo_thresh_arg(reproj_thresh, max_rounds)
    E9 = _E9(E)
    a = _hom_in(pts1)
    b = _hom_in(pts2)
    if a.n != b.n:
        raise ValueError("pts1 and pts2 differ in length")
    if a.n < 1:
        raise ValueError("no points")
    K9 = _K9(K)
    k2p, k2keep = _K2_arg(K2)
    ctx = L.context(_device_of(a, device))
    mask, mptr, mflag = _mask_buffer(a, a.n)
    Eo = np.zeros(9)
    cnt, steps = C.c_int32(0), C.c_int32(0)
    with ctx.lock:
        L.check(L.lib().rsac_essential_local_opt(ctx.handle, C.c_void_p(a.ptr), C.c_void_p(b.ptr), a.n, K9.ctypes.data,
                                                 k2p, E9.ctypes.data, thr, int(max_rounds), _in_flags(a) | mflag,
                                                 Eo.ctypes.data, C.byref(cnt), C.byref(steps), C.c_void_p(mptr),
                                                 _stream_of(a)))
    return Eo.reshape(3, 3) if Eo.any() else None, _finish_mask(mask, a.n), int(cnt.value), int(steps.value)


def essential_local_opt_batched(pts1_list, pts2_list, K, E_list, reproj_thresh: float = 1.0, *, K2=None,
                                max_rounds: int = 4, device=0, _batch=None):
    """essential_local_opt of P independent problems side by side (rsac_essential_local_opt_batched)
    -> [(E (3,3) | None, mask, count, steps)].

    Every round is one batched mask, one batched refit and one host synchronisation for the problems
    whose count is still rising; each problem follows exactly the loop and acceptance rule of the
    single call.  K (and K2): (3,3) for every problem or (P,3,3).  E_list[p] None (or all zeros): no
    model -> (None, zero mask, 0, 0)."""
    thr = _lo_thresh_arg(reproj_thresh, max_rounds)
    bt = _batch if _batch is not None else _FmBatch(pts1_list, pts2_list, device)
    E_list = list(E_list)
    if len(E_list) != bt.P:
        raise ValueError("E_list and pts1_list differ in length")
    if bt.P < 1:
        return []
    Ein = _model_rows(E_list, "every E")
    K1s = _per_problem_K(K, bt.P, "K")
    K2s = None if K2 is None else _per_problem_K(K2, bt.P, "K2")
    ctx = L.context(bt.device)
    mask, mptr, mflag = bt.mask_buffer()
    Eo = np.zeros((bt.P, 9))
    cnt = np.zeros(bt.P, np.int32)
    steps = np.zeros(bt.P, np.int32)
    with ctx.lock:
        L.check(L.lib().rsac_essential_local_opt_batched(
            ctx.handle, C.c_void_p(bt.ptrs[0]), C.c_void_p(bt.ptrs[1]), bt.off.ctypes.data, bt.P, K1s.ctypes.data,
            None if K2s is None else K2s.ctypes.data, Ein.ctypes.data, thr, int(max_rounds), bt.flags | mflag,
            Eo.ctypes.data, cnt.ctypes.data, steps.ctypes.data, C.c_void_p(mptr), bt.stream()))
    masks = bt.split(mask)
    return [(Eo[p].reshape(3, 3) if Eo[p].any() else None, masks[p], int(cnt[p]), int(steps[p])) for p in range(bt.P)]


def essential_ransac(pts1, pts2, K, reproj_thresh: float = 1.0, *, K2=None, max_iters: int = 1000,
                     confidence: float = 0.999, seed: int = 0x5EED, adaptive: bool = True, device=None,
                     return_info: bool = False, exact_only: bool = False, score: str = "count", refine=False,
                     return_F: bool = False):
    """Essential matrix RANSAC from five-point samples (rsac_essential_ransac).

    pts1, pts2 (N,2) pixels, K (3,3) the first view's intrinsics, K2 the second's (None: K for both).
    Returns (E (3,3) unit Frobenius norm or None, mask); x2^T K2^-T E K^-1 x1 = 0.  A hypothesis is
    the pixel-space F = K2^-T E K^-1, so reproj_thresh is in pixels on the Sampson distance, as for
    fundamental_ransac (cv2.findEssentialMat measures otherwise; no parity is claimed).  A sample
    owns ten records: max_iters and info.iters count samples, info.best_hyp is the record index
    (sample best_hyp // 10, root best_hyp % 10), the iteration bound uses model_points = 5, n >= 5.
    score: "count" or "msac", as fundamental_ransac.  refine=True returns the least-squares
    fundamental_fit on the winner's mask projected onto the essential manifold (a fit without a
    model, always under 8 inliers, keeps the minimal model).  return_F=True appends the F returned
    (E = essential_from_fundamental(F, K, K2)) after the mask.

    refine="pose" and refine="lo"  run the loop as refine=False and then a second
    call from the winner: "pose" is essential_refine from the winner's E on the winner's mask (the
    mask returned stays the RANSAC phase's; a refit without a model keeps the minimal E); "lo" is
    essential_local_opt from the winner (the mask and info.n_inliers are the optimised model's,
    info.lo_improvements the accepted rounds).  With either, return_F's F is
    essential_to_fundamental of the E returned: one model.  Any other value raises ValueError."""
    refine = _em_refine_arg(refine, "essential_ransac")
    msac = _score_flag(score, "essential_ransac")
    a = _hom_in(pts1)
    b = _hom_in(pts2)
    if a.n != b.n:
        raise ValueError("pts1 and pts2 differ in length")
    ctx = L.context(_device_of(a, device))
    flags = _flags(adaptive, False, "philox", exact_only) | _in_flags(a) | msac
    if refine is True:
        flags |= L.F_REFINE
    mask, mptr, mflag = _mask_buffer(a, a.n)
    flags |= mflag
    K9 = _K9(K)
    k2p, k2keep = _K2_arg(K2)
    E = np.zeros(9)
    F = np.zeros(9)
    st = L.Stats()
    with ctx.lock:
        code = L.check(L.lib().rsac_essential_ransac(ctx.handle, C.c_void_p(a.ptr), C.c_void_p(b.ptr), a.n,
                                                     K9.ctypes.data, k2p, int(max_iters), float(reproj_thresh),
                                                     float(confidence), int(seed) & (2**64 - 1), flags, E.ctypes.data,
                                                     F.ctypes.data, C.c_void_p(mptr), C.byref(st), _stream_of(a)))
        cost = int(_last_costs(ctx, 1)[0]) if msac and return_info else -1
    m = _finish_mask(mask, a.n)
    ok = code == L.OK
    info = _info(code, st)
    if ok and refine in ("pose", "lo"):  # a second call from the winner, as fundamental_lmeds(refine=True) composes
        E3 = E.reshape(3, 3)
        if refine == "pose":
            # on the device the loop ran on: measured faster than the host twin for NumPy inputs too (§25)
            Er = essential_refine(pts1, pts2, K, E3, m, K2=K2, device=_device_of(a, device))
            E3 = E3 if Er is None else Er  # a refit without a model keeps the minimal E
        else:
            El, ml, cl, sl = essential_local_opt(pts1, pts2, K, E3, reproj_thresh, K2=K2, device=device)
            if El is not None:
                E3, m = El, ml
                info.n_inliers, info.lo_improvements = cl, sl
        Fr = essential_to_fundamental(E3, K, K2)  # E and F returned are one model
        E = E3.reshape(9)
        F = F if Fr is None else Fr.reshape(9)
    out = (E.reshape(3, 3) if ok else None, m)
    if return_F:
        out = out + (F.reshape(3, 3) if ok else None,)
    if not return_info:
        return out
    if msac:
        info.cost = cost
        info.cost_px2 = cost / 2.0 ** msac_shift(float(reproj_thresh)) if cost >= 0 else float("nan")
    return out + (info,)


def essential_ransac_batched(pts1_list, pts2_list, K, reproj_thresh: float = 1.0, *, K2=None, max_iters: int = 500,
                             confidence: float = 0.999, seed: int = 0x5EED, adaptive: bool = True,
                             score: str = "count", refine=False, exact_only: bool = False, device=0,
                             return_F: bool = False):
    """P independent essential_ransac calls in one launch sequence (rsac_essential_ransac_batched)
    -> [(E | None, mask, n_inliers)]; return_F=True appends F, score="msac" the winner's cost (-1
    without a model).  K (and K2): (3,3) for every problem or (P,3,3).  Problem p returns the bits
    of essential_ransac on its points and intrinsics.  max_iters defaults to 500: the hypothesis
    buffers hold P x 10 x max_iters records.  Every problem needs >= 5 correspondences.
    refine="pose" / "lo": as essential_ransac, through essential_refine_batched /
    essential_local_opt_batched from the winners ("lo": masks and n_inliers of the optimised models)."""
    refine = _em_refine_arg(refine, "essential_ransac_batched")
    msac = _score_flag(score, "essential_ransac_batched")
    pts1_list, pts2_list = list(pts1_list), list(pts2_list)
    bt = _FmBatch(pts1_list, pts2_list, device)
    if bt.P < 1:
        return []
    if bt.counts.min() < 5:
        raise ValueError("every problem needs >= 5 correspondences")

    K1s = _per_problem_K(K, bt.P, "K")
    K2s = None if K2 is None else _per_problem_K(K2, bt.P, "K2")
    ctx = L.context(bt.device)
    flags = _flags(adaptive, False, "philox", exact_only) | bt.flags | msac
    if refine is True:
        flags |= L.F_REFINE
    mask, mptr, mflag = bt.mask_buffer()
    E = np.zeros((bt.P, 9))
    F = np.zeros((bt.P, 9))
    status = np.zeros(bt.P, np.int32)
    ninl = np.zeros(bt.P, np.int32)
    with ctx.lock:
        L.check(L.lib().rsac_essential_ransac_batched(ctx.handle, C.c_void_p(bt.ptrs[0]), C.c_void_p(bt.ptrs[1]),
                                                      bt.off.ctypes.data, bt.P, K1s.ctypes.data,
                                                      None if K2s is None else K2s.ctypes.data, int(max_iters),
                                                      float(reproj_thresh), float(confidence), int(seed) & (2**64 - 1),
                                                      flags | mflag, E.ctypes.data, F.ctypes.data, status.ctypes.data,
                                                      ninl.ctypes.data, C.c_void_p(mptr), bt.stream()))
        costs = _last_costs(ctx, bt.P) if msac else None
    masks = bt.split(mask)
    if refine in ("pose", "lo"):  # a second batched call from the winners
        done = [False] * bt.P
        E_list = [E[p].reshape(3, 3) if status[p] == L.OK else None for p in range(bt.P)]
        if refine == "pose":
            new = essential_refine_batched(pts1_list, pts2_list, K1s, E_list, masks, K2=K2s, device=bt.device,
                                           return_info=True, _batch=bt)
            for p, (Er, fi) in enumerate(new):
                if Er is not None:  # a refit without a model keeps the minimal E
                    E[p] = Er.reshape(9)
                    F[p] = fi.F.reshape(9)  # the record's F: essential_to_fundamental of this E, bit for bit
                    done[p] = True
        else:
            new = essential_local_opt_batched(pts1_list, pts2_list, K1s, E_list, reproj_thresh, K2=K2s,
                                              device=bt.device, _batch=bt)
            for p, (El, ml, cl, sl) in enumerate(new):
                if El is not None:
                    E[p] = El.reshape(9)
                    masks[p] = ml
                    ninl[p] = cl
        for p in range(bt.P):  # E and F returned are one model
            if status[p] == L.OK and not done[p]:
                Fr = essential_to_fundamental(E[p], K1s[p], None if K2s is None else K2s[p])
                if Fr is not None:
                    F[p] = Fr.reshape(9)
    out = []
    for p in range(bt.P):
        ok = status[p] == L.OK
        row = (E[p].reshape(3, 3) if ok else None, masks[p], int(ninl[p]))
        if return_F:
            row = row + (F[p].reshape(3, 3) if ok else None,)
        out.append(row + (int(costs[p]),) if msac else row)
    return out


def _essential_hypotheses(a, b, K, K2, hyp_begin, n_hyps, reproj_thresh, seed, device, exact_only, costs):
    if K is None:
        raise ValueError("hypotheses('essential', ...) needs K")
    A = _hom_in(a)
    B = _hom_in(b)
    if A.n != B.n:
        raise ValueError("pts1 and pts2 differ in length")
    rows = 10 * int(n_hyps)
    ctx = L.context(_device_of(A, device))
    flags = _in_flags(A) | (L.F_EXACT_ONLY if exact_only else 0)
    counts = np.zeros(rows, np.int32)
    status = np.zeros(rows, np.int8)
    models = np.zeros((rows, 16))
    cost = np.zeros(rows, np.int64) if costs else None
    K9 = _K9(K)
    k2p, k2keep = _K2_arg(K2)
    with ctx.lock:
        L.check(L.lib().rsac_essential_hypotheses(ctx.handle, C.c_void_p(A.ptr), C.c_void_p(B.ptr), A.n, K9.ctypes.data,
                                                  k2p, int(hyp_begin), int(n_hyps), float(reproj_thresh),
                                                  int(seed) & (2**64 - 1), flags, counts.ctypes.data,
                                                  status.ctypes.data, models.ctypes.data,
                                                  None if cost is None else cost.ctypes.data, _stream_of(A)))
    return (status, counts, models, cost) if costs else (status, counts, models)


def poly_real_roots(c) -> np.ndarray:
    """The real roots of c[0] + c[1] x + .. + c[d] x^d, d <= 10, in ascending order, on the host
    (rsac_poly_real_roots; no device needed): the five-point solver's root finder, whose bits the
    kernel reproduces.  Zero leading coefficients lower the degree; roots of even multiplicity are
    not reported."""
    cc = np.ascontiguousarray(np.asarray(c, np.float64).reshape(-1))
    if not 1 <= cc.size <= 11:
        raise ValueError("poly_real_roots takes 1 .. 11 coefficients (degree <= 10)")
    roots = np.zeros(10)
    n = L.lib().rsac_poly_real_roots(cc.ctypes.data, cc.size - 1, roots.ctypes.data)
    return roots[:n].copy()


def essential_minimal5(pts1, pts2, K, K2=None, *, return_E: bool = False):
    """The five-point minimal solver on the host (rsac_em_minimal5; no device needed): 5
    correspondences (pixels) -> the list of 0 .. 10 models F (3,3) = K2^-T E K^-1 at unit Frobenius
    norm in ascending root order -- the bits record 10 s + r of hypotheses("essential", ...) holds for
    that sample.  return_E=True: -> (Fs, Es), Es the solver's E at unit norm."""
    a = np.ascontiguousarray(np.asarray(pts1, np.float64).reshape(-1, 2))
    b = np.ascontiguousarray(np.asarray(pts2, np.float64).reshape(-1, 2))
    if a.shape[0] != 5 or b.shape[0] != 5:
        raise ValueError("essential_minimal5 takes exactly 5 correspondences")
    K9 = _K9(K)
    k2p, k2keep = _K2_arg(K2)
    F = np.zeros(90)
    E = np.zeros(90)
    n = C.c_int32(0)
    L.check(L.lib().rsac_em_minimal5(a.ctypes.data, b.ctypes.data, K9.ctypes.data, k2p, F.ctypes.data, E.ctypes.data,
                                     C.byref(n)))
    Fs = [F[9 * r:9 * r + 9].reshape(3, 3).copy() for r in range(int(n.value))]
    if not return_E:
        return Fs
    return Fs, [E[9 * r:9 * r + 9].reshape(3, 3).copy() for r in range(int(n.value))]


def essential_from_fundamental(F, K, K2=None):
    """K2^T F K projected onto the essential manifold (rsac_essential_from_fundamental; host only):
    singular values (1, 1, 0) / sqrt 2, the largest-magnitude entry (the first in row-major order)
    positive.  None when the product has rank < 2."""
    F9 = np.ascontiguousarray(np.asarray(F, np.float64).reshape(9))
    K9 = _K9(K)
    k2p, k2keep = _K2_arg(K2)
    E = np.zeros(9)
    code = L.check(L.lib().rsac_essential_from_fundamental(F9.ctypes.data, K9.ctypes.data, k2p, E.ctypes.data))
    return E.reshape(3, 3) if code == L.OK else None


def recover_pose(pts1, pts2, K, E, mask=None, *, K2=None, return_counts: bool = False):
    """(R, t) with x2 ~ R x1 + t, det R = +1, |t| = 1 from an essential matrix
    (rsac_essential_recover_pose; host only): of the four candidates (R_a, +t), (R_a, -t), (R_b, +t),
    (R_b, -t) the one with the most masked points (mask None: all) at positive depth in both cameras,
    ties keeping the earlier.  -> (R, t, n_front), or (None, None, 0) when no point is in front for
    any candidate; return_counts=True appends the four candidates' counts."""
    a = np.ascontiguousarray(np.asarray(pts1.cpu() if _is_torch(pts1) else pts1, np.float64).reshape(-1, 2))
    b = np.ascontiguousarray(np.asarray(pts2.cpu() if _is_torch(pts2) else pts2, np.float64).reshape(-1, 2))
    if a.shape[0] != b.shape[0]:
        raise ValueError("pts1 and pts2 differ in length")
    n = a.shape[0]
    mk = None
    if mask is not None:
        mk = _host_mask_arg(mask.cpu() if _is_torch(mask) else mask, n)
    K9 = _K9(K)
    k2p, k2keep = _K2_arg(K2)
    E9 = np.ascontiguousarray(np.asarray(E, np.float64).reshape(9))
    R = np.zeros(9)
    t = np.zeros(3)
    front = np.zeros(4, np.int32)
    code = L.check(L.lib().rsac_essential_recover_pose(a.ctypes.data, b.ctypes.data, n, K9.ctypes.data, k2p,
                                                       E9.ctypes.data, None if mk is None else mk.ctypes.data,
                                                       R.ctypes.data, t.ctypes.data, front.ctypes.data))
    out = (R.reshape(3, 3), t, int(front.max())) if code == L.OK else (None, None, 0)
    return out + (front,) if return_counts else out
