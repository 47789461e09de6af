"""MSAC scoring on the GPU (RSAC_F_MSAC, k_pnp_cost): every comparison is exact equality with the
reference chain of tests/msacref.py -- the unchanged CPU oracle for models, status and refit, the
NumPy restatement for counts, costs, scan and masks.  Data: synth.pnp_problem, 8 px threshold,
seed 0x5EED; costs in units of 2^-13 px^2 (k = 13, Q = 524288).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import msacref as M  # noqa: E402
import pyoracle as O  # noqa: E402
import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

THR, SEED = M.THR, M.SEED
ROWS = range(len(M.TABLE))


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _check_hypotheses(n, outl, seed, H, hyp0=0):
    pr = M.problem(n, outl, seed)
    st, cnt, mdl, cost = rsac.hypotheses("pnp", pr["points3d"], pr["points2d"], pr["K"], hyp0, H, THR, seed=SEED,
                                         costs=True)
    rs, rc, rcost, rm = M.hypotheses_case(n, outl, seed, H, hyp0)
    np.testing.assert_array_equal(st, rs)
    assert _bits_equal(mdl[:, :12], rm[:, :12])
    np.testing.assert_array_equal(cnt, rc)
    assert cost.dtype == np.int64
    np.testing.assert_array_equal(cost, rcost)
    assert (cost[st <= 0] == -1).all() and (cnt[st <= 0] == 0).all()
    return cost


# n: below one wave, one wave, both sides of 256, no multiple of the 512-point tile, several tiles
# per wave; H = 512 is a multiple of the block's 32 hypotheses
@pytest.mark.parametrize("row", ROWS)
def test_hypotheses_exhaustive(row):
    cost = _check_hypotheses(*M.TABLE[row][0], 512)
    assert cost.max() > 0


def test_hypotheses_h_not_a_multiple_of_the_block():
    _check_hypotheses(1000, .5, 5, 5000)


def test_hypotheses_from_hyp_begin_4096():
    _check_hypotheses(333, .5, 4, 512, hyp0=4096)


def test_costs_accumulate_in_64_bits():
    cost = _check_hypotheses(*M.BIG, 64)
    assert cost.max() > 2**32 and int(cost.max()) == 4297588736
    rs, rc, rcost, _ = M.hypotheses_case(*M.BIG, 64)
    assert M.scan(rcost, rc, rs, M.BIG[0], 4, 0.99, 64)[:2] == (15, 2284265089)
    pr = M.problem(*M.BIG)
    info = rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 64, THR, seed=SEED, score="msac",
                           return_info=True)[3]
    assert (info.best_hyp, info.cost) == (15, 2284265089)


@pytest.mark.parametrize("row", ROWS)
def test_pnp_ransac_msac_equals_table_and_chain(row):
    (n, outl, seed), (best, cost, count, iters) = M.TABLE[row]
    pr = M.problem(n, outl, seed)
    ref = M.ransac_case(n, outl, seed)
    assert (ref["best"], ref["cost"], ref["n_inliers"], ref["iters"]) == (best, cost, count, iters)
    R, t, mask, info = rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 5000, THR, seed=SEED, score="msac",
                                       return_info=True)
    assert R is not None
    assert (info.best_hyp, info.cost, info.n_inliers, info.iters) == (best, cost, count, iters)
    assert info.cost_px2 == cost / 2.0**13
    np.testing.assert_array_equal(mask, ref["mask"])
    assert int(mask.sum()) == count
    assert _bits_equal(R, ref["R"]) and _bits_equal(t, ref["t"])
    assert info.score_ms > 0.0  # k_pnp_cost is what score_ms times
    R0, t0, mask0, info0 = rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 5000, THR, seed=SEED,
                                           score="msac", refine=False, return_info=True)
    assert (info0.best_hyp, info0.cost, info0.n_inliers, info0.iters) == (best, cost, count, iters)
    np.testing.assert_array_equal(mask0, ref["mask"])
    assert _bits_equal(R0, ref["R0"]) and _bits_equal(t0, ref["t0"])
    if row in M.COUNT_BEST:  # the count rule still picks its own winner here
        infoc = rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 5000, THR, seed=SEED, score="count",
                                return_info=True)[3]
        assert infoc.best_hyp == M.COUNT_BEST[row] != best and infoc.cost == -1


def test_pnp_ransac_msac_opencv_sampler_epnp5():
    n, outl, seed = M.TABLE[4][0]
    pr = M.problem(n, outl, seed)
    ref = M.ransac_case(n, outl, seed, max_iters=1000, reference_mode=True)
    assert ref["best"] >= 0
    R, t, mask, info = rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 1000, THR, seed=SEED, score="msac",
                                       sampler="opencv", minimal="epnp5", return_info=True)
    assert (info.best_hyp, info.cost, info.n_inliers, info.iters) == (ref["best"], ref["cost"], ref["n_inliers"],
                                                                      ref["iters"])
    np.testing.assert_array_equal(mask, ref["mask"])
    assert _bits_equal(R, ref["R"]) and _bits_equal(t, ref["t"])


def test_pnp_ransac_msac_torch_device_inputs():
    import torch
    (n, outl, seed), (best, cost, count, iters) = M.TABLE[6]
    pr = M.problem(n, outl, seed)
    ref = M.ransac_case(n, outl, seed)
    p2 = torch.as_tensor(pr["points2d"].copy(), device="cuda")
    p3 = torch.as_tensor(pr["points3d"].copy(), device="cuda")
    R, t, mask, info = rsac.pnp_ransac(p2, p3, pr["K"], 5000, THR, seed=SEED, score="msac", return_info=True)
    assert mask.is_cuda
    assert (info.best_hyp, info.cost, info.n_inliers, info.iters) == (best, cost, count, iters)
    np.testing.assert_array_equal(mask.cpu().numpy(), ref["mask"])
    assert _bits_equal(R, ref["R"]) and _bits_equal(t, ref["t"])


@pytest.mark.parametrize("adaptive", [False, True])
def test_batched_equals_single_problem_reference(adaptive):
    """Fixed or adaptive budget: the scan is the same sequential scan over max_iters hypotheses (the
    budget rule only changes how many are evaluated per round), so both equal the single-problem chain."""
    prs = [M.problem(*row[0]) for row in M.TABLE]
    out = rsac.pnp_ransac_batched([p["points2d"] for p in prs], [p["points3d"] for p in prs], [p["K"] for p in prs],
                                  5000, THR, seed=SEED, score="msac", adaptive=adaptive)
    assert len(out) == len(M.TABLE)
    for (key, (best, cost, count, iters)), res in zip(M.TABLE, out):
        ref = M.ransac_case(*key)
        R, t, mask, ninl, c = res
        assert (c, ninl) == (cost, count), key
        np.testing.assert_array_equal(mask, ref["mask"])
        assert _bits_equal(R, ref["R"]) and _bits_equal(t, ref["t"]), key  # the winner, refined
    off = np.r_[0, np.cumsum([len(p["points2d"]) for p in prs])]
    flat = rsac.pnp_ransac_batched_flat(np.concatenate([p["points2d"] for p in prs]),
                                        np.concatenate([p["points3d"] for p in prs]), off,
                                        np.stack([p["K"] for p in prs]), 5000, THR, seed=SEED, score="msac",
                                        adaptive=adaptive)
    assert len(flat) == 6 and flat[5].dtype == np.int64
    assert list(flat[5]) == [row[1][1] for row in M.TABLE]
    assert list(flat[3]) == [row[1][2] for row in M.TABLE]


def test_score_poses_costs():
    n, outl, seed = 333, .5, 4
    pr = M.problem(n, outl, seed)
    soa, cam = O.soa_pnp(pr["points3d"], pr["points2d"]), O.cam_from_K(pr["K"])
    ref = M.ransac_case(n, outl, seed)
    rng = np.random.default_rng(21)
    poses = []
    for i in range(40):  # the refined winner, then rotations of the camera about its centre, growing
        dR = rsac.rodrigues(rng.normal(0, 1, 3) * 5e-5 * i)  # to ~2 mrad: from every inlier kept to none
        poses.append(np.r_[(dR @ ref["R"]).reshape(9), dR @ ref["t"]])
    poses = np.array(poses)
    cnt, cost = rsac.score_poses(pr["points2d"], pr["points3d"], pr["K"], poses, THR, costs=True)
    rcost, rcnt = M.costs(poses, np.ones(40, np.int8), soa, cam, THR)
    np.testing.assert_array_equal(cnt, rcnt)
    np.testing.assert_array_equal(cost, rcost)
    assert len(set(cost.tolist())) > 20 and cnt.max() > cnt.min()


@pytest.mark.parametrize("row", [1, 6])
def test_default_is_the_count_rule(row):
    n, outl, seed = M.TABLE[row][0]
    pr = M.problem(n, outl, seed)
    ref = O.pnp_ransac(pr["points3d"], pr["points2d"], pr["K"], THR, 0.99, 5000, SEED)
    info = rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 5000, THR, seed=SEED, return_info=True)[3]
    assert info.cost == -1 and np.isnan(info.cost_px2)
    assert (info.best_hyp, info.iters, info.n_inliers) == (ref["best"], ref["iters"], ref["n_inliers"])


def test_c_level_einval():
    pr = M.problem(64, .3, 7)
    p3 = np.ascontiguousarray(pr["points3d"], np.float64)
    p2 = np.ascontiguousarray(pr["points2d"], np.float64)
    K9 = np.ascontiguousarray(pr["K"], np.float64).reshape(9)
    R, t, mask = np.zeros(9), np.zeros(3), np.zeros(64, np.uint8)
    ctx = L.context(0)
    lib = L.lib()

    def call(flags):
        with ctx.lock:
            return lib.rsac_pnp_ransac(ctx.handle, p3.ctypes.data, p2.ctypes.data, 64, K9.ctypes.data, 1000, THR,
                                       0.99, SEED, flags, R.ctypes.data, t.ctypes.data, mask.ctypes.data, None, None)

    assert call(L.F_MSAC | L.F_LO) == L.EINVAL
    assert b"RSAC_F_MSAC" in lib.rsac_last_error()
    assert call(L.F_MSAC | L.F_ASYNC) == L.EINVAL
    assert b"RSAC_F_MSAC" in lib.rsac_last_error()
    key, model = C.c_int64(0), np.zeros(12)
    with ctx.lock:
        code = lib.rsac_pnp_evaluate_range(ctx.handle, p3.ctypes.data, p2.ctypes.data, 64, K9.ctypes.data, 0, 64, THR,
                                           SEED, L.F_MSAC, C.byref(key), model.ctypes.data, None, None, None)
    assert code == L.EINVAL and b"RSAC_F_MSAC" in lib.rsac_last_error()
    costs = np.zeros(1, np.int64)
    assert call(L.F_MSAC | L.F_ADAPTIVE) == L.OK
    with ctx.lock:
        assert lib.rsac_last_costs(ctx.handle, costs.ctypes.data, 1) == L.OK
    assert costs[0] == M.TABLE[1][1][1]
    assert call(L.F_ADAPTIVE) == L.OK  # a count call: no costs to report afterwards
    with ctx.lock:
        assert lib.rsac_last_costs(ctx.handle, costs.ctypes.data, 1) == L.EINVAL
