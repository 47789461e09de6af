"""Fundamental-matrix f32 Sampson pre-filter on the GPU: on every scene of
fmbandref (threshold ladders, ill-conditioned model families, frame and threshold edges) and on
every shape of the work queue, the default path (k_fm_score_q behind fm_write_record's band), the
all-f64 kernel (exact_only) and the CPU oracle must agree on every status and every count, and the
models must equal the oracle's bit for bit.  There are no tolerances.  The CPU side
(test_fm_prefilter.py) shows that the ladder scenes put pairs where the band matters.
"""
import functools
import os

import numpy as np
import pytest

import fmbandref as R
import pyoracle as O
import rsac
from rsac import synth

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
H_SCENE, HYP0 = 1500, 11


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _gpu(p1, p2, thr, hyp0, H, seed, exact_only=False):
    return rsac.hypotheses("fundamental", p1, p2, None, hyp0, H, thr, seed=seed, exact_only=exact_only)


def _check_three_ways(p1, p2, thr, hyp0=HYP0, H=H_SCENE, seed=R.SEED):
    soa = O.soa_hom(p1, p2)
    st_f, c_f, m_f = _gpu(p1, p2, thr, hyp0, H, seed)
    st_e, c_e, m_e = _gpu(p1, p2, thr, hyp0, H, seed, exact_only=True)
    oc, ost = O.fm_hypotheses_mt(soa, thr, seed, H, hyp0, threads=THREADS)
    _, _, om = O.fm_hypotheses(soa, thr, seed, H, hyp0, models=True)
    np.testing.assert_array_equal(st_e, ost)
    np.testing.assert_array_equal(c_e, oc)
    np.testing.assert_array_equal(st_f, ost)
    bad = np.nonzero(c_f != oc)[0]
    assert bad.size == 0, (f"{bad.size} counts differ from the exact kernel and the oracle; first: hypothesis "
                           f"{hyp0 + bad[0]}: pre-filter {c_f[bad[0]]}, exact {oc[bad[0]]}")
    assert _bits_equal(m_f[:, :9], om[:, :9]) and _bits_equal(m_e[:, :9], om[:, :9])
    return oc, ost


@pytest.mark.parametrize("name", list(R.all_scenes()))
def test_scene_counts_equal_exact_kernel_and_oracle(name):
    p1, p2, thr, kind = R.all_scenes()[name]
    # thr 0, inf and NaN: the count call takes every value (thr2 becomes 0, +inf, NaN in f32) and
    # must still count as the f64 test does
    oc, ost = _check_three_ways(p1, p2, thr)
    if kind in ("ladder", "family"):
        assert (ost > 0).any() and oc.max() >= R.LADDER0  # clean samples see every exact correspondence


@pytest.mark.parametrize("name", ["A_1.5", "C_far_1e+06_y2"])
def test_ransac_end_to_end_equals_oracle(name):
    p1, p2, thr, _ = R.all_scenes()[name]
    F, m, info = rsac.fundamental_ransac(p1, p2, thr, max_iters=3000, return_info=True)
    ref = O.fm_ransac(p1, p2, thr, 0.99, 3000)
    assert (info.best_hyp, info.n_inliers, info.iters) == (ref["best"], ref["n_inliers"], ref["iters"])
    assert _bits_equal(F, ref["F"])
    np.testing.assert_array_equal(m, ref["mask"])


# ---------------------------------------------------------------------------------------------
# queue geometry
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _h_big():
    """More tiles than k_fm_score_q can have resident blocks, and a partial last tile.  A block is 256
    threads = 4 waves, one per SIMD of its CU; the kernel is built for at most 8 waves per SIMD, so a
    CU holds at most 8 blocks and `resident` (launch_fm_score) is at most 8 CUs.  H_big has
    8 CUs + 4 tiles of 32 hypotheses, the last of them with 7: at least 4 tiles go out as whole-tile
    units (tb > 0), the rest by cells."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    h = 32 * (8 * cus) + 32 * 3 + 7
    assert 8 * cus * 32 < h
    return h


@pytest.mark.parametrize("n", [256, 257, 2047, 2048, 2049, 4097])
def test_queue_geometry(n):
    # n: both sides of kLanePts (256: k_fm_score_lane), of one cell of 256 x 8 points and of two
    pr = synth.fundamental_problem(n, 0.5, seed=n)
    p1, p2 = pr["pts1"], pr["pts2"]
    soa = O.soa_hom(p1, p2)
    for hyp0 in (0, 11):
        for H in (1, 31, 33):
            _check_three_ways(p1, p2, 1.5, hyp0, H, seed=7)
        H = _h_big()
        st_f, c_f, m_f = _gpu(p1, p2, 1.5, hyp0, H, 7)
        st_e, c_e, m_e = _gpu(p1, p2, 1.5, hyp0, H, 7, exact_only=True)
        np.testing.assert_array_equal(st_f, st_e)
        np.testing.assert_array_equal(c_f, c_e)
        assert _bits_equal(m_f[:, :9], m_e[:, :9])
        assert c_e.max() >= 8
        for lo in (0, H - 2048):  # the first and the last 2048 against the oracle
            oc, ost = O.fm_hypotheses_mt(soa, 1.5, 7, 2048, hyp0 + lo, threads=THREADS)
            np.testing.assert_array_equal(st_f[lo:lo + 2048], ost)
            np.testing.assert_array_equal(c_f[lo:lo + 2048], oc)


def test_same_call_twice_gives_the_same_counts():
    # the atomic adds go onto zeroed counts and the queue counters are reset per launch: a second
    # call on the same context (same buffers) must not see the first
    p1, p2, thr, _ = R.all_scenes()["A_1.5"]
    first = _gpu(p1, p2, thr, HYP0, H_SCENE, R.SEED)
    pr = synth.fundamental_problem(2049, 0.5, seed=2049)
    big = [_gpu(pr["pts1"], pr["pts2"], 1.5, 0, _h_big(), 7) for _ in range(2)]
    second = _gpu(p1, p2, thr, HYP0, H_SCENE, R.SEED)
    for a, b in ((first, second), big):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        assert _bits_equal(a[2], b[2])
