"""The homography refit on the device (k_hom_fit) against its host twin and the oracle -- equality
of the f64 bit patterns -- through rsac_homography_fit_device, the batched call, the drivers'
RSAC_F_REFINE on device-resident inputs, and local optimisation against the loop restated on the
oracle (tests/homfitref.py).  NaN results are compared by position: the host's and the device's
default NaNs differ in sign and payload."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import homfitref as R  # noqa: E402
import pyoracle as O  # noqa: E402
import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu


def _same(a, b):
    """bit patterns equal; NaNs by position"""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def _torch():
    import torch
    assert torch.cuda.is_available(), "the gpu tests need a HIP device"
    return torch


@contextlib.contextmanager
def _fit_mode(mode):
    """RSAC_DBG_HOM_FIT around a driver call: 1 the host tail, 2 the device fit, 0 the policy"""
    ctx = L.context(0)
    ctx.debug_set(L.DBG_HOM_FIT, mode)
    try:
        yield
    finally:
        ctx.debug_set(L.DBG_HOM_FIT, 0)


def _forms(src, dst, mask):
    """the three input forms of one case -> [(name, src, dst, mask, kwargs)]"""
    torch = _torch()
    dev = torch.device("cuda:0")
    ts, td = torch.tensor(src, dtype=torch.float64, device=dev), torch.tensor(dst, dtype=torch.float64, device=dev)
    tm = None if mask is None else torch.tensor(np.asarray(mask) != 0, device=dev)
    fs = torch.tensor(np.ascontiguousarray(src.T), dtype=torch.float32, device=dev)
    fd = torch.tensor(np.ascontiguousarray(dst.T), dtype=torch.float32, device=dev)
    return [("host", src, dst, mask, dict(device=0)), ("device", ts, td, tm, {}), ("soa", fs, fd, tm, {})]


def _check_fit(src, dst, mask, what, forms=("host", "device", "soa")):
    host = rsac.homography_fit(src, dst, mask)
    orc = R.fit(O.soa_hom(src, dst), mask)
    assert (host is None) == (orc is None), what
    if host is not None:
        assert _same(host, orc), what
    for name, s, d, m, kw in _forms(src, dst, mask):
        if name not in forms:
            continue
        H = rsac.homography_fit(s, d, m, **kw)
        assert (H is None) == (host is None), (what, name)
        if host is not None:
            assert _same(H, host), (what, name, H, host)
    return host


@pytest.mark.parametrize("m", R.SIZES)
def test_device_fit_equals_host_fit(m):
    """every masked count around the 64-point staging chunk, every noise level (the LM's accept-only
    path at 0; lambda -> 0, the restart and rejected steps from 0.01; the iteration cap at 3 px with
    planted errors: the census of DESIGN.md), masks of all ones, every third point dropped, one
    whole chunk masked out; the three input forms"""
    for shape in ("ones", "third") + (("chunk",) if m >= 128 else ()):
        for noise in R.NOISES:
            src, dst, mask = R.case(m, shape, noise)
            # every form at the extremes of the noise range, the f32 SoA form throughout
            forms = ("host", "device", "soa") if noise in (0.0, 3.0) else ("soa",)
            assert _check_fit(src, dst, mask, (m, shape, noise), forms) is not None


def test_exactly_four_ones_and_no_model():
    for n in (130, 4097):
        assert _check_fit(*R.four_ones(n), ("four", n)) is not None
        assert _check_fit(*R.three_ones(n), ("three", n)) is None
    for which in ("src", "dst"):
        assert _check_fit(*R.equal_x(65, which), ("equal x", which)) is None
    # the ABI's codes: RSAC_NO_MODEL with H_out zero
    src, dst, mask = R.three_ones(130)
    ctx = L.context(0)
    H = np.full(9, 7.0)
    m8 = np.ascontiguousarray(mask, np.uint8)
    s, d = np.ascontiguousarray(src), np.ascontiguousarray(dst)
    with ctx.lock:
        code = L.lib().rsac_homography_fit_device(ctx.handle, s.ctypes.data, d.ctypes.data, 130, m8.ctypes.data, 0,
                                                  H.ctypes.data, None)
    assert code == L.NO_MODEL and not H.any()


def test_translation_stops_on_the_residuals():
    src, dst, mask = R.translation()
    H = _check_fit(src, dst, mask, "translation")
    assert np.allclose(H, [[1, 0, 5], [0, 1, -3], [0, 0, 1]], atol=1e-9)


def test_debuglog_blocks():
    blocks = R.debuglog_blocks()
    assert len(blocks) == 24
    for k, (src, dst, mask) in enumerate(blocks):
        assert _check_fit(src, dst, mask, ("block", k), ("host", "device")) is not None


def _batch(P):
    """sizes 4 .. 40 mixed; some problems with fewer than 4 masked points, one degenerate"""
    rng = np.random.default_rng(77 + P)
    srcs, dsts, masks = [], [], []
    for p in range(P):
        n = 4 + (p * 7) % 37
        pr = R.problem(n, 0.0, 500 + p, [0.0, 0.5, 3.0][p % 3])
        mask = rng.uniform(size=n) < 0.8
        if p % 11 == 3:
            mask[:] = False
            mask[:3] = True  # three ones
        if p == min(5, P - 1):
            pr["dst"][:, 1] = pr["dst"][0, 1]  # degenerate: a zero deviation sum
            mask[:] = True
        srcs.append(pr["src"])
        dsts.append(pr["dst"])
        masks.append(mask)
    return srcs, dsts, masks


@pytest.mark.parametrize("P", [1, 2, 65, 458])
def test_batched_fit(P):
    srcs, dsts, masks = _batch(P)
    got = rsac.homography_fit_batched(srcs, dsts, masks)
    none = 0
    for p in range(P):
        want = rsac.homography_fit(srcs[p], dsts[p], masks[p]) if len(srcs[p]) >= 4 else None
        assert (got[p] is None) == (want is None), p
        if want is None:
            none += 1
        else:
            assert _same(got[p], want), p
    assert (got[min(5, P - 1)] is None) and (P < 65 or none >= 6)
    # the raw call: no-model rows are zero with status RSAC_NO_MODEL
    s, d = np.ascontiguousarray(np.concatenate(srcs)), np.ascontiguousarray(np.concatenate(dsts))
    m = np.ascontiguousarray(np.concatenate(masks), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(x) for x in srcs])]).astype(np.int64)
    H, st = np.full((P, 9), 7.0), np.full(P, -1, np.int32)
    ctx = L.context(0)
    with ctx.lock:
        code = L.lib().rsac_homography_fit_batched_device(ctx.handle, s.ctypes.data, d.ctypes.data, off.ctypes.data, P,
                                                          m.ctypes.data, 0, H.ctypes.data, st.ctypes.data, None)
    assert code == (L.OK if any(g is not None for g in got) else L.NO_MODEL)
    for p in range(P):
        assert st[p] == (L.NO_MODEL if got[p] is None else L.OK)
        assert not H[p].any() if got[p] is None else _same(H[p], got[p])
    # mask_list None = all points
    got_all = rsac.homography_fit_batched(srcs[:2], dsts[:2])
    for p in range(min(P, 2)):
        want = rsac.homography_fit(srcs[p], dsts[p])
        assert (got_all[p] is None) == (want is None) and (want is None or _same(got_all[p], want))


@pytest.mark.parametrize("n", [200, 2000])
def test_drivers_refit_on_the_device(n):
    """refine=True from device tensors: H is the host fit on the returned mask; mask, count and info
    are those of refine=False"""
    torch = _torch()
    pr = R.problem(n, 0.3, 21 + n, 1.0)
    ts, td = (torch.tensor(pr[k], dtype=torch.float64, device="cuda:0") for k in ("src", "dst"))
    for call in (rsac.homography_ransac, rsac.homography_lmeds):
        H0, m0, i0 = call(ts, td, refine=False, return_info=True)
        with _fit_mode(2):  # the device fit from the mask where it lies
            H1, m1, i1 = call(ts, td, refine=True, return_info=True)
        Hp, mp = call(ts, td, refine=True)  # the measured policy: whichever it picks, the same bits
        assert H0 is not None and H1 is not None and _same(Hp, H1) and np.array_equal(mp.cpu().numpy(), m1.cpu().numpy())
        mask = m1.cpu().numpy()
        assert np.array_equal(mask, m0.cpu().numpy())
        assert (i1.n_inliers, i1.best_hyp, i1.iters, i1.hyps_scored) == (i0.n_inliers, i0.best_hyp, i0.iters,
                                                                         i0.hyps_scored)
        assert _same(H1, rsac.homography_fit(pr["src"], pr["dst"], mask))
        assert _same(H1, R.fit(O.soa_hom(pr["src"], pr["dst"]), mask))
        # ... and the host-input form returns the same bits
        H2, m2 = call(pr["src"], pr["dst"], refine=True)
        assert _same(H2, H1) and np.array_equal(m2, mask)


def test_batched_driver_refit():
    P = 65
    srcs, dsts = [], []
    for p in range(P):
        pr = R.problem(30 + 3 * p, 0.3, 900 + p, 1.0)
        srcs.append(pr["src"])
        dsts.append(pr["dst"])
    for mode in (2, 1, 0):
        with _fit_mode(mode):
            out = rsac.homography_ransac_batched(srcs, dsts, refine=True)
        for p, (H, mask, ninl) in enumerate(out):
            assert H is not None
            assert _same(H, O.hom_refine(O.soa_hom(srcs[p], dsts[p]), mask, np.eye(3))), (mode, p)


def test_batch_past_the_policy_threshold():
    """8 problems of 2000 points: the policy's own pick of the device fit; the host tail's bits"""
    srcs, dsts = [], []
    for p in range(8):
        pr = R.problem(2000, 0.3, 950 + p, 1.0)
        srcs.append(pr["src"])
        dsts.append(pr["dst"])
    out = rsac.homography_ransac_batched(srcs, dsts, refine=True)
    with _fit_mode(1):
        host = rsac.homography_ransac_batched(srcs, dsts, refine=True)
    for p in range(8):
        assert out[p][0] is not None and _same(out[p][0], host[p][0]) and np.array_equal(out[p][1], host[p][1])
        assert _same(out[p][0], O.hom_refine(O.soa_hom(srcs[p], dsts[p]), out[p][1], np.eye(3))), p


@pytest.mark.parametrize("key", R.INPUTS, ids=[str(k[0]) for k in R.INPUTS])
def test_local_opt_matches_the_restated_loop(key):
    torch = _torch()
    r, pr = R.row(key), R.problem(*key)
    assert R.table_row(key) == R.TABLE[key]
    src, dst = pr["src"], pr["dst"]
    for cap in (1, 4):
        rH, rmask, rcount, rsteps = r["lo"][cap]
        for name, s, d, _, _ in _forms(src, dst, None):
            H, mask, count, steps = rsac.homography_local_opt(s, d, r["H0"], R.THR, max_rounds=cap)
            if name != "host":
                assert torch.is_tensor(mask) and mask.is_cuda  # RSAC_F_DEVICE_OUT
                mask = mask.cpu().numpy()
            assert (count, steps) == (rcount, rsteps), (name, cap)
            assert np.array_equal(mask, rmask) and _same(H, rH), (name, cap)


def test_local_opt_zero_rounds_and_bad_arguments():
    key = R.INPUTS[0]
    pr = R.problem(*key)
    far = np.array([[1.0, 0, 5000.0], [0, 1.0, 5000.0], [0, 0, 1.0]])
    H, mask, count, steps = rsac.homography_local_opt(pr["src"], pr["dst"], far, R.THR)
    rH, rmask, rcount, rsteps = R.local_opt(R.soa_of(key), far, R.THR, 4)
    assert steps == rsteps == 0 and count == rcount and _same(H, far) and np.array_equal(mask, rmask)
    s, d = np.ascontiguousarray(pr["src"]), np.ascontiguousarray(pr["dst"])
    Hin, Hout = np.ascontiguousarray(R.row(key)["H0"]).reshape(9), np.zeros(9)
    cnt, st = C.c_int32(0), C.c_int32(0)
    ctx = L.context(0)

    def raw(thr, rounds):
        with ctx.lock:
            return L.lib().rsac_homography_local_opt(ctx.handle, s.ctypes.data, d.ctypes.data, len(s), Hin.ctypes.data,
                                                     thr, rounds, 0, Hout.ctypes.data, C.byref(cnt), C.byref(st), None,
                                                     None)

    assert raw(R.THR, 0) == L.EINVAL and raw(R.THR, -3) == L.EINVAL
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        assert raw(thr, 4) == L.EINVAL
    assert raw(R.THR, 4) == L.OK and (cnt.value, st.value) == R.row(key)["lo"][4][2:]


def test_local_opt_from_an_all_zero_model():
    """the start rule of the single call: every row is a model, all zeros too.  No point passes the test
    of H = 0 (a non-finite projection), and a fit on no points has no model: zeros, a zero mask, count
    0, no steps"""
    pr = R.problem(*R.INPUTS[0])
    assert len(pr["src"]) == 40
    for name, s, d, _, _ in _forms(pr["src"], pr["dst"], None):
        H, mask, count, steps = rsac.homography_local_opt(s, d, np.zeros((3, 3)), R.THR, max_rounds=8)
        mask = mask.cpu().numpy() if name != "host" else mask
        print("homography_local_opt(H = 0):", name, H.tolist(), int(mask.sum()), count, steps)
        assert _same(H, np.zeros((3, 3))) and (count, steps) == (0, 0), name
        assert np.array_equal(mask, np.zeros(40, bool)), name


@pytest.mark.parametrize("key", [R.INPUTS[0], R.INPUTS[3]], ids=["40", "300"])
def test_refine_lo(key):
    """refine="lo": homography_local_opt from the winner's minimal model; the mask is the optimised
    model's and info.lo_improvements the accepted rounds"""
    torch = _torch()
    r, pr = R.row(key), R.problem(*key)
    rH, rmask, rcount, rsteps = r["lo"][4]
    ts, td = (torch.tensor(pr[k], dtype=torch.float64, device="cuda:0") for k in ("src", "dst"))
    for s, d in ((pr["src"], pr["dst"]), (ts, td)):
        H, mask, info = rsac.homography_ransac(s, d, R.THR, refine="lo", return_info=True)
        mask = mask.cpu().numpy() if torch.is_tensor(mask) else mask
        assert _same(H, rH) and np.array_equal(mask, rmask)
        assert (info.n_inliers, info.lo_improvements) == (rcount, rsteps)
    # LMedS: the loop at thr = sigma from the LMedS winner
    H0, m0, i0 = rsac.homography_lmeds(pr["src"], pr["dst"], refine=False, return_info=True)
    sigma = rsac.lmeds_sigma(i0.median, len(pr["src"]), 4)
    want = R.local_opt(R.soa_of(key), H0, sigma, 4)
    H, mask, info = rsac.homography_lmeds(pr["src"], pr["dst"], refine="lo", return_info=True)
    assert _same(H, want[0]) and np.array_equal(mask, want[1])
    assert (info.n_inliers, info.lo_improvements) == (want[2], want[3])
