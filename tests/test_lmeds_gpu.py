"""LMedS homography on the GPU (k_hom_median, k_hom_median_lane, rsac_homography_lmeds): every
comparison is exact equality with the chain of tests/lmedsref.py -- the unchanged CPU oracle for
subsets, models, status and refit, the NumPy restatement for medians, scan, sigma and masks.  A NaN
median compares as NaN.  Data: synth.homography_problem at its default noise.

Sizes: kLaneKeyPts = 32 (keys in LDS / recomputed, one lane per hypothesis), kLanePts = 256 (lane /
wave kernel), 64 (one wave), 512 = 64 * kMedP (keys in registers / recomputed), odd and even.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lmedsref as M  # noqa: E402
import pyoracle as O  # noqa: E402
import rsac  # noqa: E402
import rsac.cv2compat as cv2c  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = range(len(M.TABLE))
SIZES = [5, 6, 12, 32, 33, 63, 64, 65, 256, 257, 511, 512, 513, 2049, 5000]


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def _case(n):
    return (n, 0.0 if n <= 6 else 0.3, 100 + n)


def _check_probe_mwc(n, H):
    key = _case(n)
    pr = M.problem(*key)
    subs, sst = O.mwc_subsets(n, H, 4, hom=O.soa_hom(pr["src"], pr["dst"]))
    assert (sst == 1).all()
    rs, rmed, rm, _ = M.hypotheses_case(*key, H)
    st, med, mdl = rsac.hypotheses("homography", pr["src"], pr["dst"], n_hyps=H, subsets=subs, medians=True)
    np.testing.assert_array_equal(st, rs)
    assert _bits_equal(mdl[:, :9], rm[:, :9])
    assert med.dtype == np.float64 and _same(med, rmed)
    assert (med[st > 0] >= 0).all()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("H", [3, 55])
def test_medians_per_hypothesis(n, H):
    _check_probe_mwc(n, H)


# 257 hypotheses: more than one block of the lane kernel, 65 blocks of the wave kernel
@pytest.mark.parametrize("n", [s for s in SIZES if s <= 513])
def test_medians_257_hypotheses(n):
    _check_probe_mwc(n, 257)


@pytest.mark.parametrize("n", [12, 64, 513, 2049])
def test_medians_philox_from_hyp_begin_4096(n):
    key = _case(n)
    pr = M.problem(*key)
    rs, rmed, rm, _ = M.hypotheses_case(*key, 55, "philox", 4096)
    st, med, mdl = rsac.hypotheses("homography", pr["src"], pr["dst"], hyp_begin=4096, n_hyps=55, seed=M.SEED,
                                   medians=True)
    np.testing.assert_array_equal(st, rs)
    assert _bits_equal(mdl[:, :9], rm[:, :9])
    assert _same(med, rmed)


def _check_full(pr, ref, **kw):
    H, mask, info = rsac.homography_lmeds(pr["src"], pr["dst"], return_info=True, **kw)
    assert (info.best_hyp, info.median, info.n_inliers, info.iters) == (ref["best"], ref["median"], ref["n_inliers"],
                                                                        ref["iters"])
    np.testing.assert_array_equal(np.asarray(mask), ref["mask"])
    if ref["best"] < 0:
        assert H is None and not info.ok
    else:
        assert info.ok and _bits_equal(H, ref["H"])
    return H, mask, info


@pytest.mark.parametrize("refine", [True, False])
@pytest.mark.parametrize("row", ROWS)
def test_full_call_equals_table_and_chain(row, refine):
    key, (best, median, ones) = M.TABLE[row]
    ref = M.lmeds_case(*key, refine=refine)
    assert (ref["best"], ref["median"], ref["n_inliers"]) == (best, median, ones)
    _, _, info = _check_full(M.problem(*key), ref, refine=refine)
    assert info.hyps_scored == 55 and info.score_ms > 0.0  # k_hom_median is what score_ms times


@pytest.mark.parametrize("n", [12, 257, 2049])
def test_full_call_philox(n):
    key = _case(n)
    _check_full(M.problem(*key), M.lmeds_case(*key, sampler="philox"), sampler="philox")


def test_full_call_2000_hypotheses():
    key = M.TABLE[5][0]  # 2049 points
    ref = M.lmeds_case(*key, n_iters=2000)
    assert ref["iters"] == 2000
    _check_full(M.problem(*key), ref, n_iters=2000)


def test_torch_device_inputs_and_device_mask():
    import torch
    key = M.TABLE[4][0]  # 257 points
    pr, ref = M.problem(*key), M.lmeds_case(*key)
    s = torch.tensor(pr["src"], dtype=torch.float64, device="cuda")
    d = torch.tensor(pr["dst"], dtype=torch.float64, device="cuda")
    H, mask, info = rsac.homography_lmeds(s, d, return_info=True)
    assert mask.is_cuda and mask.dtype == torch.bool
    np.testing.assert_array_equal(mask.cpu().numpy(), ref["mask"])
    assert (info.best_hyp, info.median) == (ref["best"], ref["median"]) and _bits_equal(H, ref["H"])


def _collinear(n):
    x = np.arange(n, dtype=np.float64)
    src = np.c_[x, 2 * x + 1]
    return src, src * 3.0 + 7.0


def _batch_problems(sizes):
    prs = [M.problem(*(_case(n) if n != 4 else (4, 0.0, 104))) for n in sizes]
    return [np.asarray(p["src"]) for p in prs], [np.asarray(p["dst"]) for p in prs]


@pytest.mark.parametrize("sizes", [(4, 5, 12, 65, 257), (12, 4, 5, 33)])  # wave kernel / lane kernel
@pytest.mark.parametrize("refine", [True, False])
def test_batched_mixed_sizes_direct_branch_and_no_model(sizes, refine):
    srcs, dsts = _batch_problems(sizes)
    cs, cd = _collinear(20)  # no subset passes checkSubset: status -1 from hypothesis 0, no model
    srcs.insert(2, cs)
    dsts.insert(2, cd)
    out = rsac.homography_lmeds_batched(srcs, dsts, refine=refine)
    assert len(out) == len(srcs)
    for p, (H, mask, ninl, med) in enumerate(out):
        ref = M.lmeds(srcs[p], dsts[p], refine=refine)
        np.testing.assert_array_equal(mask, ref["mask"])
        assert (ninl, med) == (ref["n_inliers"], ref["median"]), p
        if ref["best"] < 0:
            assert H is None
        else:
            assert _bits_equal(H, ref["H"]), p
    H, mask, ninl, med = out[2]
    assert H is None and not mask.any() and (ninl, med) == (0, -1.0)
    p4 = sizes.index(4) + (1 if sizes.index(4) >= 2 else 0)
    assert out[p4][1].all() and out[p4][2:] == (4, 0.0)  # the direct branch: mask ones, median 0


def test_every_hypothesis_without_a_model():
    # explicit subsets with a repeated point: the minimal solve fails, status 0, median -1; the
    # scan then finds no model
    key = _case(65)
    pr = M.problem(*key)
    subs = np.tile(np.array([[0, 0, 1, 2]], np.int32), (55, 1))
    rs, rmed, _, _ = M.hypotheses(pr["src"], pr["dst"], 55, subsets=subs)
    assert (rs == 0).all() and (rmed == -1.0).all()
    st, med, _ = rsac.hypotheses("homography", pr["src"], pr["dst"], n_hyps=55, subsets=subs, medians=True)
    np.testing.assert_array_equal(st, rs)
    assert _same(med, rmed)
    sc = rsac.LmedsScan(55).step(st, med)
    assert (sc.best, sc.iter, sc.done) == (-1, 55, True)


@pytest.mark.parametrize("n_bad,n,nan_only", [(5, 9, False), (7, 12, True), (40, 70, False), (301, 600, False),
                                              (301, 600, True)])
def test_more_than_half_the_errors_nan_or_inf(n_bad, n, nan_only):
    # the first n - n_bad points are a clean problem, sampled by the explicit subsets; the others
    # have an infinite src (a NaN error under every model) or dst (an infinite error) coordinate
    pr = M.problem(n, 0.0, 300 + n)
    src, dst = np.array(pr["src"]), np.array(pr["dst"])
    good = n - n_bad
    if nan_only:  # the median itself is a NaN
        src[good:, 0] = np.inf
    else:  # ... an infinity: the NaN keys rank above the infinite ones
        src[good::2, 0] = np.inf
        dst[good + 1::2, 1] = np.inf
    rng = np.random.default_rng(n)
    subs = np.array([rng.choice(good, 4, replace=False) for _ in range(55)], np.int32)
    rs, rmed, rm, soa = M.hypotheses(src, dst, 55, subsets=subs)
    e = M.hom_err(rm[0, :9], soa)
    assert np.isnan(e).any() and (nan_only or np.isinf(e).any()) and (~np.isfinite(e)).sum() == n_bad
    assert (rs > 0).all() and (np.isnan(rmed) if nan_only else np.isinf(rmed)).all()
    st, med, mdl = rsac.hypotheses("homography", src, dst, n_hyps=55, subsets=subs, medians=True)
    np.testing.assert_array_equal(st, rs)
    assert _bits_equal(mdl[:, :9], rm[:, :9])
    assert _same(med, rmed)
    sc = rsac.LmedsScan(55).step(st, med)
    assert sc.best == -1  # neither an infinite nor a NaN median wins
    # fewer than half bad: the same ranks, finite medians
    src[good + 2:, 0] = pr["src"][good + 2:, 0]
    dst[good + 2:, 1] = pr["dst"][good + 2:, 1]
    rs, rmed, rm, soa = M.hypotheses(src, dst, 55, subsets=subs)
    assert np.isfinite(rmed[rs > 0]).all()
    st, med, mdl = rsac.hypotheses("homography", src, dst, n_hyps=55, subsets=subs, medians=True)
    np.testing.assert_array_equal(st, rs)
    assert _same(med, rmed)


def test_c_abi_argument_checks():
    pr = M.problem(*M.TABLE[1][0])
    with pytest.raises(rsac.RsacError, match="confidence"):
        rsac.homography_lmeds(pr["src"], pr["dst"], confidence=1.0)
    with pytest.raises(rsac.RsacError) as ei:
        rsac.homography_lmeds(pr["src"][:3], pr["dst"][:3])
    assert ei.value.code == rsac._lib.ETOOFEW
    import ctypes as C
    from rsac import _lib as L
    ctx = L.context(0)
    s = np.ascontiguousarray(pr["src"])
    d = np.ascontiguousarray(pr["dst"])
    H, mask = np.zeros(9), np.zeros(len(s), np.uint8)
    code = L.lib().rsac_homography_lmeds(ctx.handle, s.ctypes.data, d.ctypes.data, len(s), 2000, 0.995, 1,
                                         L.F_MSAC, H.ctypes.data, mask.ctypes.data, None, None, None)
    assert code == L.EINVAL and b"RSAC_F_MSAC" in L.lib().rsac_last_error()


@pytest.mark.parametrize("row", ROWS)
def test_shim_lmeds_equals_the_restatement_bit_for_bit(row):
    key = M.TABLE[row][0]
    pr, ref = M.problem(*key), M.lmeds_case(*key)
    H, mask = cv2c.findHomography(pr["src"], pr["dst"], cv2c.LMEDS)
    H2, mask2 = rsac.homography_lmeds(pr["src"], pr["dst"])
    assert mask.shape == (key[0], 1) and mask.dtype == np.uint8
    np.testing.assert_array_equal(mask[:, 0].astype(bool), ref["mask"])
    np.testing.assert_array_equal(mask[:, 0].astype(bool), mask2)
    assert _bits_equal(H, ref["H"]) and _bits_equal(H, H2)
    # the threshold is ignored, as in OpenCV
    H3, mask3 = cv2c.findHomography(pr["src"], pr["dst"], cv2c.LMEDS, 75.0)
    assert _bits_equal(H3, H) and np.array_equal(mask3, mask)


def test_shim_other_methods_are_unchanged():
    key = M.TABLE[3][0]
    pr = M.problem(*key)
    with pytest.raises(NotImplementedError, match="RHO"):
        cv2c.findHomography(pr["src"], pr["dst"], cv2c.RHO)
    for thr in (3.0, 75.0):
        ref = O.hom_ransac(pr["src"], pr["dst"], thr, 0.995, 2000, sampler="opencv", refine=True)
        H, mask = cv2c.findHomography(pr["src"], pr["dst"], cv2c.RANSAC, thr)
        np.testing.assert_array_equal(mask[:, 0].astype(bool), ref["mask"])
        assert _bits_equal(H, ref["H_refined"])
    # 4 points: the direct branch whatever the method
    p4 = M.problem(4, 0.0, 104)
    Ha, ma = cv2c.findHomography(p4["src"], p4["dst"], cv2c.LMEDS)
    Hb, mb = cv2c.findHomography(p4["src"], p4["dst"], cv2c.RANSAC)
    assert _bits_equal(Ha, Hb) and ma.all() and mb.all()
    assert _bits_equal(Ha, M.lmeds(p4["src"], p4["dst"])["H"])
