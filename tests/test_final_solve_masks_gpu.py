"""The final pose solves on the GPU under structured masks (tests/finalsolveref.py): k_pnp_refine
through rsac.refine_pose_device, the one entry that takes a caller's mask, over the mask catalogue
and the block caps that select each layout of its reducer (one range / several ranges staged once /
tiles re-staged per pass with a carried slot offset / the multi-block hand-off); k_pnp_epnp_s1 /
_s3 through pnp_ransac on problems shaped until RANSAC's mask is the wanted set; and the centre
rule for a non-finite first point.  Every comparison is equality of the f64 bits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import finalsolveref as F  # noqa: E402
import pyoracle as O  # noqa: E402
import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu


class _cap:
    """DBG_REFIT_MAX_BLOCKS for the block: -> the blocks a refit of n points launches.  The cap
    goes to rsac.context(), the context refine_pose_device and pnp_ransac run on"""

    def __init__(self, n, cap):
        self.n, self.cap, self.ctx = n, cap, rsac.context()

    def __enter__(self):
        assert self.ctx is L.context(0)  # what refine_pose_device(device=None) uses
        nr = F.lm_blocks(self.n)
        ranges, limit = self.ctx.refit_blocks(self.n)  # uncapped: min(ranges, the device's limit)
        assert ranges == nr and 1 <= limit <= nr
        self.ctx.debug_set(L.DBG_REFIT_MAX_BLOCKS, self.cap)
        got = self.ctx.refit_blocks(self.n)
        assert got == (nr, min(self.cap or nr, nr, limit)), (got, limit)
        return got[1]

    def __exit__(self, *exc):
        self.ctx.debug_set(L.DBG_REFIT_MAX_BLOCKS, 0)
        return False


def _device_refit(p3, px, K, mask, R0, t0, n, cap):
    with _cap(n, cap) as blocks:
        R, t = rsac.refine_pose_device(px, p3, K, R0, t0, mask=mask)
    return R, t, blocks


# ---------------------------------------------------------------------------------------------
# 1. LM refit under the mask catalogue
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,cap", F.LM_CAPPED, ids=F.LM_CAPPED_IDS)
def test_device_refit_equals_restatement(case, cap):
    pr, _, _, R0, t0 = F.lm_inputs(case.n)
    mask = F.lm_mask(case.n, case.mask)
    Re, te = F.lm_expected(case.n, case.mask)
    ones = int(mask.sum())
    if ones >= 6:  # not a vacuous pass: the fit moved
        assert not (F.bits_equal(Re, R0) and F.bits_equal(te, t0))
    if ones == 0:
        assert F.bits_equal(Re, R0) and F.bits_equal(te, t0)
    R, t, blocks = _device_refit(pr["points3d"], pr["points2d"], pr["K"], mask, R0, t0, case.n, cap)
    assert F.bits_equal(R, Re) and F.bits_equal(t, te), (blocks, F.layout(case.n, blocks)[:2])
    assert rsac.context().refit_blocks(case.n)[1] >= blocks  # the cap is gone


def test_the_cap_cases_run_capped_and_mix_the_layouts():
    # what the launches above ran, from refit_blocks and the span arithmetic of set_ranges
    ctx = rsac.context()
    limit = ctx.refit_blocks(262145)[1]
    for n, cap, want in [(8200, 1, ["tile path"]), (8200, 2, ["tile path", "staged once"]),
                         (8200, 3, ["staged once"] * 3), (65537, 7, ["tile path"] * 7),
                         (262145, 3, ["tile path"] * 3)]:
        with _cap(n, cap) as blocks:
            assert blocks == min(cap, limit)
            if blocks == cap:
                assert [lay for _, _, lay in F.layout(n, blocks)] == want
    assert ctx.refit_blocks(8200) == (9, min(9, limit))


# ---------------------------------------------------------------------------------------------
# 2. EPnP on the inliers under shaped masks
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(F.EP_CASES)), ids=F.EP_IDS)
def test_epnp_final_solve_on_shaped_masks(i):
    c, d = F.EP_CASES[i], F.ep_case(i)
    np.testing.assert_array_equal(d["ransac"]["mask"], d["S"])  # a condition on the inputs
    assert int(d["S"].sum()) == c.inliers and d["Re"] is not None
    R, t, m = rsac.pnp_ransac(d["px"], d["p3"], d["K"], c.iters, F.THR, refine="epnp")
    np.testing.assert_array_equal(m, d["S"])
    assert F.bits_equal(R, d["Re"]) and F.bits_equal(t, d["te"])
    R, t, m = rsac.pnp_ransac(d["px"], d["p3"], d["K"], c.iters, F.THR, refine="epnp+lm")
    np.testing.assert_array_equal(m, d["S"])
    assert F.bits_equal(R, d["Rl"]) and F.bits_equal(t, d["tl"])


def test_epnp_final_solve_batched_on_shaped_masks():
    ds = [F.ep_case(i) for i in F.EP_BATCH]
    iters = {F.EP_CASES[i].iters for i in F.EP_BATCH}
    assert len(ds) == 3 and len(iters) == 1
    out = rsac.pnp_ransac_batched([d["px"] for d in ds], [d["p3"] for d in ds], [d["K"] for d in ds], iters.pop(),
                                  F.THR, refine="epnp")
    for d, (R, t, m, ninl) in zip(ds, out):
        np.testing.assert_array_equal(m, d["S"])
        assert ninl == int(d["S"].sum())
        assert F.bits_equal(R, d["Re"]) and F.bits_equal(t, d["te"])


# ---------------------------------------------------------------------------------------------
# 3. a non-finite first point
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(F.BAD_FIRST))
@pytest.mark.parametrize("n,name,cap", [(600, "iid50", 0), (8200, "iid50", 0), (8200, "iid50", 2),
                                        (8200, "lastofrange", 0)])
def test_device_refit_centres_on_the_lowest_masked_point(n, name, cap, kind):
    # the check that does not lean on the restatement: the refit equals that of the problem whose
    # point 0 is the lowest masked point (the unchanged finite path, the same centre and order).
    # 8200 points: nine blocks (two under the cap), each of which finds the index on its own
    pr, _, _, R0, t0 = F.lm_inputs(n)
    mask, bad, moved = F.centre_pair(n, name, kind)
    R, t, blocks = _device_refit(bad, pr["points2d"], pr["K"], mask, R0, t0, n, cap)
    Rm, tm, _ = _device_refit(moved, pr["points2d"], pr["K"], mask, R0, t0, n, cap)
    assert np.isfinite(R).all() and np.isfinite(t).all()
    assert F.bits_equal(R, Rm) and F.bits_equal(t, tm), blocks
    assert not (F.bits_equal(R, R0) and F.bits_equal(t, t0))
    Ro, to, _ = O.pnp_refine(O.soa_pnp(bad, pr["points2d"]), mask, O.cam_from_K(pr["K"]), R0, t0)
    assert F.bits_equal(R, Ro) and F.bits_equal(t, to)


@pytest.mark.parametrize("kind", sorted(F.BAD_FIRST))
@pytest.mark.parametrize("refine", [False, True, "epnp", "epnp+lm"])
def test_pnp_ransac_with_a_non_finite_first_point(refine, kind):
    # refine=False: the RANSAC phase alone.  The one-problem set-up centres the scoring frame on the
    # first point too (k_pnp_setup_fc); a NaN there once staged every point as a decided outlier
    pr = F.e2e_problem(kind)
    ref, Re, te = F.ransac_chain(pr["points3d"], pr["points2d"], pr["K"], 2000, refine)
    assert ref["n_inliers"] == 419 and not ref["mask"][0]
    R, t, m, info = rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 2000, F.THR, refine=refine,
                                    return_info=True)
    np.testing.assert_array_equal(m, ref["mask"])
    assert info.best_hyp == ref["best"] and info.n_inliers == 419
    assert np.isfinite(R).all() and np.isfinite(t).all()
    assert F.bits_equal(R, Re) and F.bits_equal(t, te)


def test_pnp_ransac_with_a_nan_first_point_from_device_tensors():
    import torch
    pr = F.e2e_problem()
    ref, Re, te = F.ransac_chain(pr["points3d"], pr["points2d"], pr["K"], 2000, True)
    p2 = torch.tensor(pr["points2d"], dtype=torch.float64, device="cuda")
    p3 = torch.tensor(pr["points3d"], dtype=torch.float64, device="cuda")
    R, t, m = rsac.pnp_ransac(p2, p3, pr["K"], 2000, F.THR, refine=True)
    np.testing.assert_array_equal(m.cpu().numpy(), ref["mask"])
    assert F.bits_equal(R, Re) and F.bits_equal(t, te)


@pytest.mark.parametrize("kind", sorted(F.BAD_FIRST))
@pytest.mark.parametrize("key,bad_lead", [(F.E2E_KEY, 1), ((5000, 0.5, 9), 1), ((5000, 0.5, 9), 3), ((600, 0.3, 9), 300)])
def test_pose_counts_with_non_finite_leading_points(key, bad_lead, kind):
    # the scoring side alone: counts of given poses against the exact count.  bad_lead: the first
    # that many points are non-finite (1; 3: the centre moves to point 3; 300: past the 256 points
    # the set-up looks at, so it centres on the origin).  2048 poses: past the small round, so the
    # MFMA scorer where the frame allows; 5000 points: 20 set-up blocks, which must agree
    pr = F.e2e_problem(None, key)
    P3 = np.array(pr["points3d"])
    k, v = F.BAD_FIRST[kind]
    P3[:bad_lead, k] = v
    rng = np.random.default_rng(7)
    poses = np.array([np.r_[pr["R"].reshape(9), pr["t"] + rng.normal(size=3) * s] for s in (0, .05, .05, .5, .5, 5)])
    soa, cam = O.soa_pnp(P3, pr["points2d"]), O.cam_from_K(pr["K"])
    ref = [O.pnp_count(p[:9].reshape(3, 3), p[9:], soa, cam, F.THR) for p in poses]
    assert ref[0] >= (int(pr["inlier"].sum()) - bad_lead) * 0.9 > 100
    batch = np.resize(poses, (2048, 12))
    fast = rsac.score_poses(pr["points2d"], P3, pr["K"], batch, F.THR)
    np.testing.assert_array_equal(fast, np.resize(ref, len(batch)))


@pytest.mark.parametrize("refine", [True, "epnp"])
def test_batched_with_a_nan_first_point_in_the_second_problem(refine):
    prs = [F.problem(300, 31), F.e2e_problem(), F.problem(513, 32)]
    a = ([p["points2d"] for p in prs], [p["points3d"] for p in prs], [p["K"] for p in prs])
    out = rsac.pnp_ransac_batched(*a, 2000, F.THR, refine=refine)
    assert len(out) == 3
    for p, (R, t, m, ninl) in zip(prs, out):
        R1, t1, m1 = rsac.pnp_ransac(p["points2d"], p["points3d"], p["K"], 2000, F.THR, refine=refine)
        ref, Re, te = F.ransac_chain(p["points3d"], p["points2d"], p["K"], 2000, refine)
        np.testing.assert_array_equal(m, m1)
        np.testing.assert_array_equal(m, ref["mask"])
        assert ninl == ref["n_inliers"]
        assert np.isfinite(R).all() and np.isfinite(t).all()
        assert F.bits_equal(R, R1) and F.bits_equal(t, t1)
        assert F.bits_equal(R, Re) and F.bits_equal(t, te)


def test_lo_ransac_with_a_nan_first_point():
    pr = F.e2e_problem()
    lo = O.pnp_ransac_lo(pr["points3d"], pr["points2d"], pr["K"], F.THR, F.CONF, 5000)
    R, t, m, info = rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 5000, F.THR, refine=False, lo=True,
                                    return_info=True)
    _, _, _, plain = rsac.pnp_ransac(pr["points2d"], pr["points3d"], pr["K"], 5000, F.THR, refine=False,
                                     return_info=True)
    assert np.isfinite(R).all() and np.isfinite(t).all()
    assert F.bits_equal(R, lo["R"]) and F.bits_equal(t, lo["t"])
    np.testing.assert_array_equal(m, lo["mask"])
    assert info.lo_improvements == lo["lo_improvements"]
    assert info.n_inliers == lo["n_inliers"] >= plain.n_inliers > 0
