"""MSAC scoring for homographies on the GPU (RSAC_F_MSAC through hom_core; k_hom_cost,
k_hom_cost_lane): every comparison of counts, costs, masks and models is exact equality with the
chain of tests/hmsacref.py -- the unchanged CPU oracle for subsets, models, status and refit,
lmedsref.hom_err and msacref's cost and scan on top.  Data: synth.homography_problem at its default
noise, 8 px threshold (k = 13, Q = 524288), seed 0x5EED; the location search at 75 px (k = 7).

Sizes: kLanePts = 256 (lane / tile kernel), 512 = one wave's tile, 2048 = one pass of the block's four
waves, each plus one; 8200 points for a cost above 2^32.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hmsacref as M  # noqa: E402
import pyoracle as O  # noqa: E402
import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

THR, SEED = M.THR, M.SEED
ROWS = range(len(M.TABLE))


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _case(n):
    return (n, 0.0 if n <= 6 else 0.3, 100 + n)


def _check_hypotheses(key, H, hyp0=0, mwc=False):
    pr = M.problem(*key)
    subs = None
    if mwc:  # caller subsets: OpenCV's MWC sequence from the oracle
        subs, sst = O.mwc_subsets(key[0], H, 4, hom=O.soa_hom(pr["src"], pr["dst"]))
        assert (sst == 1).all()
        rs, rc, rcost, rm = M.hypotheses(pr["src"], pr["dst"], THR, H, subsets=subs)
    else:
        rs, rc, rcost, rm = M.hypotheses_case(*key, H, "philox", hyp0)
    st, cnt, mdl, cost = rsac.homography_costs(pr["src"], pr["dst"], hyp0, H, THR, seed=SEED, subsets=subs)
    np.testing.assert_array_equal(st, rs)
    assert _bits_equal(mdl[:, :9], rm[:, :9])
    np.testing.assert_array_equal(cnt, rc)
    assert cost.dtype == np.int64
    np.testing.assert_array_equal(cost, rcost)
    assert (cost[st <= 0] == -1).all() and (cnt[st <= 0] == 0).all()
    # the counts are the count kernels' own
    st2, cnt2, mdl2 = rsac.hypotheses("homography", pr["src"], pr["dst"], None, hyp0, H, THR, seed=SEED, subsets=subs)
    np.testing.assert_array_equal(st2, st)
    np.testing.assert_array_equal(cnt2, cnt)
    assert _bits_equal(mdl2[:, :9], mdl[:, :9])
    return cost


@pytest.mark.parametrize("n", [5, 12, 13, 256, 257, 512, 513, 2048, 2049])
def test_costs_per_hypothesis(n):
    cost = _check_hypotheses(_case(n), 512)
    assert cost.max() > 0


@pytest.mark.parametrize("n", [12, 257])
@pytest.mark.parametrize("H", [1, 100])
def test_costs_h_not_a_multiple_of_the_block(n, H):
    _check_hypotheses(_case(n), H)


@pytest.mark.parametrize("n", [12, 513])
def test_costs_from_hyp_begin_4096(n):
    _check_hypotheses(_case(n), 100, hyp0=4096)


@pytest.mark.parametrize("n", [13, 256, 257, 2049])
def test_costs_caller_subsets(n):
    _check_hypotheses(_case(n), 100, mwc=True)


@pytest.mark.parametrize("H", [1, 33])
@pytest.mark.parametrize("n", [5, 256, 257, 2048, 2049])
def test_plain_counts_equal_the_host_count(n, H):
    """The count kernels without MSAC (k_hom_score_lane up to 256 points, k_hom_score above; 2048 =
    one pass of the block's four waves; one hypothesis, and one past a block of 32) against the
    count rsac_hom_cost_host returns for each record's model."""
    pr = M.problem(*_case(n))
    st, cnt, mdl = rsac.hypotheses("homography", pr["src"], pr["dst"], None, 0, H, THR, seed=SEED)
    for h in range(H):
        want = rsac.homography_cost(pr["src"], pr["dst"], mdl[h, :9], THR)[0] if st[h] > 0 else 0
        assert cnt[h] == want, (n, H, h)


def test_costs_accumulate_in_64_bits():
    cost = _check_hypotheses(M.BIG, 64)
    assert cost.max() > 2**32


def _check_ransac(pr, ref, **kw):
    H, mask, info = rsac.homography_ransac(pr["src"], pr["dst"], THR, seed=SEED, score="msac", return_info=True, **kw)
    assert (info.best_hyp, info.cost, info.n_inliers, info.iters) == (ref["best"], ref["cost"], ref["n_inliers"],
                                                                      ref["iters"])
    mask = mask.cpu().numpy() if hasattr(mask, "cpu") else np.asarray(mask)
    np.testing.assert_array_equal(mask, ref["mask"])
    if ref["best"] < 0:
        assert H is None and not info.ok and info.cost == -1 and np.isnan(info.cost_px2)
    else:
        assert info.ok and _bits_equal(H, ref["H"] if kw.get("refine", True) else ref["H0"])
        assert info.cost_px2 == ref["cost"] / 2.0**13
        assert info.score_ms > 0.0  # the cost kernel is what score_ms times
    return info


@pytest.mark.parametrize("refine", [True, False])
@pytest.mark.parametrize("row", ROWS)
def test_homography_ransac_msac_equals_table_and_chain(row, refine):
    (sampler, key), want = M.TABLE[row]
    ref = M.ransac_case(sampler, *key, refine=refine)
    assert (ref["best"], ref["cost"], ref["n_inliers"], ref["iters"]) == want
    pr = M.problem(*key)
    _check_ransac(pr, ref, sampler=sampler, refine=refine)
    if row in M.COUNT_BEST and refine:  # the count rule still picks its own winner here
        infoc = rsac.homography_ransac(pr["src"], pr["dst"], THR, seed=SEED, sampler=sampler, score="count",
                                       return_info=True)[2]
        assert infoc.best_hyp == M.COUNT_BEST[row] != want[0] and infoc.cost == -1 and np.isnan(infoc.cost_px2)


@pytest.mark.parametrize("row", [0, 2, 4])
def test_homography_ransac_msac_fixed_budget(row):
    """adaptive=False scores all max_iters hypotheses in one round; the scan over them is the same
    sequential scan, so the result is the adaptive call's."""
    (sampler, key), _ = M.TABLE[row]
    info = _check_ransac(M.problem(*key), M.ransac_case(sampler, *key), sampler=sampler, adaptive=False)
    assert info.hyps_scored == M.MAX_ITERS and info.rounds == 1


@pytest.mark.parametrize("row", [1, 3])
def test_homography_ransac_msac_torch_device_inputs(row):
    import torch
    (sampler, key), _ = M.TABLE[row]
    pr = M.problem(*key)
    dev = dict(src=torch.as_tensor(pr["src"].copy(), device="cuda"), dst=torch.as_tensor(pr["dst"].copy(), device="cuda"))
    _check_ransac(dev, M.ransac_case(sampler, *key), sampler=sampler)


def test_four_points_take_the_direct_branch():
    pr = M.problem(4, 0.0, 7)
    ref = M.ransac(pr["src"], pr["dst"], THR)
    assert ref["best"] == 0 and ref["cost"] == -1 and ref["mask"].all()
    H, mask, info = rsac.homography_ransac(pr["src"], pr["dst"], THR, seed=SEED, score="msac", return_info=True)
    assert info.ok and info.cost == -1 and np.isnan(info.cost_px2) and info.n_inliers == 4
    assert _bits_equal(H, ref["H"]) and np.asarray(mask).all()


@pytest.mark.parametrize("sampler", ["opencv", "philox"])
def test_no_eligible_model_gives_no_model(sampler):
    """collinear source points: no subset passes the sampler's check, every status is < 0"""
    src = np.c_[np.linspace(-0.5, 0.5, 12), np.zeros(12)]
    dst = np.random.default_rng(3).uniform(0, 1000, (12, 2))
    ref = M.ransac(src, dst, THR, sampler=sampler)
    assert ref["best"] == -1
    _check_ransac(dict(src=src, dst=dst), ref, sampler=sampler)


BATCH = [(4, 0.0, 7), (5, 0.0, 105), (12, .25, 5), (300, .6, 4)]


@pytest.mark.parametrize("adaptive", [True, False])
def test_batched_mixed_sizes_equal_the_single_calls(adaptive):
    """max_n = 300 selects the tile kernel for the 4-, 5- and 12-point problems too"""
    prs = [M.problem(*k) for k in BATCH]
    out = rsac.homography_ransac_batched([p["src"] for p in prs], [p["dst"] for p in prs], THR, seed=SEED,
                                         score="msac", adaptive=adaptive)
    assert len(out) == len(BATCH)
    for key, pr, res in zip(BATCH, prs, out):
        H, mask, ninl, cost = res
        ref = M.ransac_case("opencv", *key)
        assert (cost, ninl) == (ref["cost"], ref["n_inliers"]), key
        np.testing.assert_array_equal(mask, ref["mask"])
        assert _bits_equal(H, ref["H"]), key
        H1, mask1, info1 = rsac.homography_ransac(pr["src"], pr["dst"], THR, seed=SEED, score="msac",
                                                  return_info=True)
        assert _bits_equal(H, H1) and np.array_equal(mask, np.asarray(mask1)) and cost == info1.cost
    assert out[0][3] == -1 and out[3][3] == M.TABLE[2][1][1]


def test_location_search_msac():
    pr, rows, err = M.location_case(0, 40)
    moved = [l for l, r in enumerate(rows) if r["best"] != r["count_best"]]
    assert len(moved) >= 1  # 18 of these 40 locations (244 of 458 at the full size)
    res = rsac.location_search(pr["pos3d"], pr["pixels"], pr["locations"], 75.0, score="msac")
    assert res.cost is not None and res.cost.dtype == np.int64 and res.cost.shape == (40,)
    for l, r in enumerate(rows):
        assert res.ok[l] == (r["best"] >= 0)
        assert (int(res.cost[l]), int(res.n_inliers[l])) == (r["cost"], r["n_inliers"]), l
        np.testing.assert_array_equal(res.mask[l], r["mask"])
        if r["best"] >= 0:
            assert _bits_equal(res.H[l], r["H"]), l
    # err1 / err2 come from the unchanged f64 scoring kernel on these H and masks; its sums against
    # NumPy's literal loops are compared as tests/test_gpu_parity.py compares them
    np.testing.assert_allclose(res.err, err, rtol=1e-9, atol=1e-9)
    assert res.best == O.best_location(err)
    # the count rule picks other hypotheses at the `moved` locations: without the refit their models differ
    m0 = rsac.location_search(pr["pos3d"], pr["pixels"], pr["locations"], 75.0, score="msac", refine=False)
    c0 = rsac.location_search(pr["pos3d"], pr["pixels"], pr["locations"], 75.0, refine=False)
    assert c0.cost is None
    differ = [l for l in range(40) if not _bits_equal(m0.H[l], c0.H[l])]
    assert len(differ) >= 1 and set(differ) <= set(moved)  # (two indices may hold the same subset)
    from rsac.location import find_homographies
    recs = [{"pos3d": p, "pixel": px} for p, px in zip(pr["pos3d"], pr["pixels"])]
    nm = find_homographies(recs, [{"grid_code": 1, "pos3d": q} for q in pr["locations"]], 75.0, score="msac")
    np.testing.assert_array_equal(nm, res.err)  # the keyword reaches location_search


def test_score_count_is_the_default():
    (sampler, key), _ = M.TABLE[4]
    pr = M.problem(*key)
    a = rsac.homography_ransac(pr["src"], pr["dst"], THR, seed=SEED, sampler=sampler, return_info=True)
    b = rsac.homography_ransac(pr["src"], pr["dst"], THR, seed=SEED, sampler=sampler, score="count", return_info=True)
    assert _bits_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert (a[2].best_hyp, a[2].iters, a[2].n_inliers, a[2].cost) == (b[2].best_hyp, b[2].iters, b[2].n_inliers, -1)
    ref = O.hom_ransac(pr["src"], pr["dst"], THR, M.CONF, M.MAX_ITERS, SEED, sampler=sampler)
    assert a[2].best_hyp == ref["best"] and _bits_equal(a[0], ref["H_refined"])
    prs = [M.problem(*k) for k in BATCH]
    ba = rsac.homography_ransac_batched([p["src"] for p in prs], [p["dst"] for p in prs], THR)
    bb = rsac.homography_ransac_batched([p["src"] for p in prs], [p["dst"] for p in prs], THR, score="count")
    for x, y in zip(ba, bb):
        assert len(x) == len(y) == 3 and _bits_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2]
    lp = M.location_case(0, 40)[0]
    la = rsac.location_search(lp["pos3d"], lp["pixels"], lp["locations"], 75.0)
    lb = rsac.location_search(lp["pos3d"], lp["pixels"], lp["locations"], 75.0, score="count")
    assert la.cost is None and lb.cost is None
    assert _bits_equal(la.H, lb.H) and _bits_equal(la.err, lb.err) and np.array_equal(la.mask, lb.mask)


def test_c_level_contracts():
    (sampler, key), (best, cost, count, iters) = M.TABLE[2]
    pr = M.problem(*key)
    n = key[0]
    s = np.ascontiguousarray(pr["src"], np.float64)
    d = np.ascontiguousarray(pr["dst"], np.float64)
    Hm, mask = np.zeros(9), np.zeros(n, np.uint8)
    ctx = L.context(0)
    lib = L.lib()
    base = L.F_SAMPLER_OPENCV | L.F_ADAPTIVE

    def call(flags, thr=THR):
        with ctx.lock:
            return lib.rsac_homography_ransac(ctx.handle, s.ctypes.data, d.ctypes.data, n, M.MAX_ITERS, thr, M.CONF,
                                              SEED, flags, Hm.ctypes.data, mask.ctypes.data, None, None)

    def last(P):
        out = np.zeros(P, np.int64)
        with ctx.lock:
            return lib.rsac_last_costs(ctx.handle, out.ctypes.data, P), out

    for bad in (L.F_LO, L.F_ASYNC):
        assert call(base | L.F_MSAC | bad) == L.EINVAL
        assert b"RSAC_F_MSAC" in lib.rsac_last_error()
    for thr in (float("nan"), float("inf")):
        assert call(base | L.F_MSAC, thr) == L.EINVAL
        assert b"threshold" in lib.rsac_last_error()
    assert call(base | L.F_MSAC) == L.OK
    code, costs = last(1)
    assert code == L.OK and costs[0] == cost
    assert last(2)[0] == L.EINVAL
    assert b"PnP" not in lib.rsac_last_error()
    assert call(base) == L.OK  # a count call leaves the costs as it found them
    code, costs = last(1)
    assert code == L.OK and costs[0] == cost
    assert call(base | L.F_MSAC, 0.0) == L.OK  # thr <= 0: findHomography's 3 px default, then the check
    assert last(1)[0] == L.OK
    # the count probe rejects the flag; the cost probe requires its output
    cnt, st = np.zeros(8, np.int32), np.zeros(8, np.int8)
    with ctx.lock:
        code = lib.rsac_homography_hypotheses(ctx.handle, s.ctypes.data, d.ctypes.data, n, 0, 8, THR, SEED, L.F_MSAC,
                                              None, cnt.ctypes.data, st.ctypes.data, None, None)
    assert code == L.EINVAL and b"RSAC_F_MSAC" in lib.rsac_last_error()
    with ctx.lock:
        code = lib.rsac_homography_hypotheses_msac(ctx.handle, s.ctypes.data, d.ctypes.data, n, 0, 8, THR, SEED, 0,
                                                   None, cnt.ctypes.data, st.ctypes.data, None, None, None)
    assert code == L.EINVAL and b"costs_out" in lib.rsac_last_error()
