"""The final pose solves under structured masks, without a GPU (tests/finalsolveref.py): the host
twins (rsac.refine_pose, rsac.epnp_pose: the source the kernels run) against the CPU restatement bit
for bit over the mask catalogue, the catalogue's own arithmetic (ranges, spans, the conditions on
the shaped EPnP problems), and the centre rule for a non-finite first point, checked without the
restatement: the refit equals the refit of the problem whose point 0 is the lowest masked point."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import finalsolveref as F  # noqa: E402
import pyoracle as O  # noqa: E402
import rsac  # noqa: E402


def test_ranges_and_layouts_of_the_catalogue():
    assert [F.lm_blocks(n) for n in (3, 600, 4096, 4097, 8200, 65537, 262145)] == [1, 1, 1, 5, 9, 64, 64]
    assert F.ranges(4097)[0] == (0, 820) and F.ranges(4097)[-1] == (3280, 4097)
    assert F.lm_chunk(8200) == 912 and F.ranges(8200)[-1] == (7296, 8200)  # the last: 904
    assert F.lm_chunk(65537) == 1025 == 2 * F.LM_THREADS + 1
    assert F.lm_chunk(262145) == 4097 == F.LM_STAGE + 1 and F.ranges(262145)[-1] == (258111, 262145)  # 4034
    assert F.lm_blocks(262144) == 64 and F.lm_chunk(262144) == F.LM_STAGE  # the largest n of one-tile ranges
    # C: cap 1 walks all nine ranges tile by tile; cap 2: block 0 five ranges on the tile path and block 1
    # four staged once, in one launch; cap 3: three ranges a block, staged once; no cap: one range a block
    assert F.layout(8200, 1) == [(9, 8200, "tile path")]
    assert F.layout(8200, 2) == [(5, 4552, "tile path"), (4, 3648, "staged once")]
    assert F.layout(8200, 3) == [(3, 2736, "staged once"), (3, 2736, "staged once"), (3, 2728, "staged once")]
    assert set(F.layout(8200, 9)) == {(1, 912, "staged once"), (1, 904, "staged once")}
    assert all(lay == "staged once" for _, _, lay in F.layout(4097, 5))
    # D: 64 blocks of one range; 7 blocks of 10 or 9 ranges, all on the tile path
    assert all(lay == "staged once" for _, _, lay in F.layout(65537, 64))
    assert [(k, lay) for k, _, lay in F.layout(65537, 7)] == [(10, "tile path")] + [(9, "tile path")] * 6
    # E: a range is a tile and one index: the tile path even with one range a block (the last
    # range, 4034 indices, is staged once: both layouts in one launch again)
    assert [lay for _, _, lay in F.layout(262145, 64)] == ["tile path"] * 63 + ["staged once"]
    assert {lay for _, _, lay in F.layout(262145, 3)} == {"tile path"}


def test_masks_of_the_catalogue_have_the_stated_structure():
    ones = {c: int(F.lm_mask(c.n, c.mask).sum()) for c in F.LM_CASES}
    by = {(c.n, c.mask): v for c, v in ones.items()}
    assert [by[(600, f"k{k}")] for k in range(4)] == [0, 1, 2, 3]
    assert (by[(4096, "last7")], by[(4096, "thread125")], by[(4096, "mod8is7")], by[(4096, "lastwave")],
            by[(4096, "first512+last")]) == (7, 8, 512, 512, 513)
    assert (by[(4097, "range2")], by[(4097, "idx4096")], by[(4097, "ranges0and4")]) == (820, 1, 820 + 817)
    assert (by[(8200, "oddempty")], by[(8200, "lastofrange")]) == (4 * 912 + 904, 9)
    assert (by[(262145, "lastofrange")], by[(262145, "first511+lastofrange")]) == (64, 64 * 512)
    m = F.lm_mask(262145, "first511+lastofrange")
    two_tiles = F.ranges(262145)[:-1]  # (the last range, 4034 indices, is one tile)
    for lo, hi in two_tiles:  # 511 points in the range's first tile, one in its second: carried offset 511
        assert int(m[lo:lo + F.LM_STAGE].sum()) == 511 and int(m[lo + F.LM_STAGE:hi].sum()) == 1
    m = F.lm_mask(262145, "lastofrange")
    assert not any(m[lo:lo + F.LM_STAGE].any() for lo, _ in two_tiles)  # every first tile is empty
    for n in (8200, 262145):  # i.i.d.: every range holds points, none is full
        m = F.lm_mask(n, "iid50")
        assert all(0 < int(m[lo:hi].sum()) < hi - lo for lo, hi in F.ranges(n))


@pytest.mark.parametrize("case", F.LM_CASES, ids=F.LM_IDS)
def test_host_refit_equals_restatement(case):
    pr, _, _, R0, t0 = F.lm_inputs(case.n)
    mask = F.lm_mask(case.n, case.mask)
    Re, te = F.lm_expected(case.n, case.mask)
    ones = int(mask.sum())
    if ones >= 6:  # not a vacuous pass: the fit moved
        assert not (F.bits_equal(Re, R0) and F.bits_equal(te, t0))
        assert np.isfinite(Re).all() and np.isfinite(te).all()
    if ones == 0:  # nothing to fit: the start, bit for bit
        assert F.bits_equal(Re, R0) and F.bits_equal(te, t0)
    R, t = rsac.refine_pose(pr["points2d"], pr["points3d"], pr["K"], R0, t0, mask=mask)
    assert F.bits_equal(R, Re) and F.bits_equal(t, te)


@pytest.mark.parametrize("i", range(len(F.EP_CASES)), ids=F.EP_IDS)
def test_host_epnp_equals_restatement_on_shaped_masks(i):
    c, d = F.EP_CASES[i], F.ep_case(i)
    # conditions on the inputs: the restatement's RANSAC mask is the wanted set
    assert int(d["S"].sum()) == c.inliers
    np.testing.assert_array_equal(d["ransac"]["mask"], d["S"])
    assert d["Re"] is not None and np.isfinite(d["Re"]).all() and np.isfinite(d["te"]).all()
    R, t = rsac.epnp_pose(d["px"], d["p3"], d["K"], mask=d["S"].astype(np.uint8))
    assert R is not None and F.bits_equal(R, d["Re"]) and F.bits_equal(t, d["te"])
    assert not (F.bits_equal(d["Rl"], d["Re"]) and F.bits_equal(d["tl"], d["te"]))  # the LM after it moves


# ---------------------------------------------------------------------------------------------
# a non-finite first point
# ---------------------------------------------------------------------------------------------
def _lm_oracle(p3, px, K, mask, R0, t0):
    R, t, _ = O.pnp_refine(O.soa_pnp(p3, px), mask, O.cam_from_K(K), R0, t0)
    return R, t


def _lm_host(p3, px, K, mask, R0, t0):
    return rsac.refine_pose(px, p3, K, R0, t0, mask=mask)


def _ep_oracle(p3, px, K, mask, R0=None, t0=None):
    return O.pnp_epnp(O.soa_pnp(p3, px), mask, O.cam_from_K(K))


def _ep_host(p3, px, K, mask, R0=None, t0=None):
    return rsac.epnp_pose(px, p3, K, mask=mask)


CENTRE_SOLVERS = {"oracle-lm": _lm_oracle, "host-lm": _lm_host, "oracle-epnp": _ep_oracle, "host-epnp": _ep_host}


@pytest.mark.parametrize("kind", sorted(F.BAD_FIRST))
@pytest.mark.parametrize("n,name", [(600, "iid50"), (8200, "iid50"), (8200, "lastofrange"), (4097, "range2")])
@pytest.mark.parametrize("solver", sorted(CENTRE_SOLVERS))
def test_non_finite_first_point_hands_the_centre_to_the_lowest_masked(solver, n, name, kind):
    pr, _, _, R0, t0 = F.lm_inputs(n)
    mask, bad, moved = F.centre_pair(n, name, kind)
    assert not np.isfinite(bad[0]).all() and np.isfinite(bad[1:]).all() and np.isfinite(moved).all()
    f = CENTRE_SOLVERS[solver]
    R, t = f(bad, pr["points2d"], pr["K"], mask, R0, t0)
    Rm, tm = f(moved, pr["points2d"], pr["K"], mask, R0, t0)
    assert R is not None and Rm is not None
    assert np.isfinite(R).all() and np.isfinite(t).all()
    assert F.bits_equal(R, Rm) and F.bits_equal(t, tm)
    assert not (F.bits_equal(R, R0) and F.bits_equal(t, t0))


@pytest.mark.parametrize("kind", sorted(F.BAD_FIRST))
def test_host_twins_equal_restatement_with_a_non_finite_first_point(kind):
    pr, _, _, R0, t0 = F.lm_inputs(600)
    mask, bad, _ = F.centre_pair(600, "iid50", kind)
    for oracle, host in ((_lm_oracle, _lm_host), (_ep_oracle, _ep_host)):
        Ro, to = oracle(bad, pr["points2d"], pr["K"], mask, R0, t0)
        Rh, th = host(bad, pr["points2d"], pr["K"], mask, R0, t0)
        assert np.isfinite(to).all() and F.bits_equal(Rh, Ro) and F.bits_equal(th, to)
    # a masked non-finite point 0 is its own lowest masked index: as before, no finite pose
    m1 = np.array(mask)
    m1[0] = 1
    Ro, to = _lm_oracle(bad, pr["points2d"], pr["K"], m1, R0, t0)
    Rh, th = _lm_host(bad, pr["points2d"], pr["K"], m1, R0, t0)
    assert np.array_equal(Ro, Rh, equal_nan=True) and np.array_equal(to, th, equal_nan=True)


def test_a_non_finite_point_elsewhere_and_a_finite_first_point_keep_their_bits():
    # the rule reads point 0 alone: a NaN at index 5 (masked out) changes nothing, and a finite point
    # 0 stays the centre whether it is masked or not
    pr, soa, cam, R0, t0 = F.lm_inputs(600)
    mask = np.array(F.lm_mask(600, "iid50"))
    mask[[0, 5]] = 0
    ref = _lm_oracle(pr["points3d"], pr["points2d"], pr["K"], mask, R0, t0)
    q = np.array(pr["points3d"])
    q[5, 0] = np.nan
    for f in (_lm_oracle, _lm_host):
        R, t = f(q, pr["points2d"], pr["K"], mask, R0, t0)
        assert F.bits_equal(R, ref[0]) and F.bits_equal(t, ref[1])
    # centred elsewhere, the same fit has other bits: point 0 is the centre, not the lowest masked
    j = int(np.flatnonzero(mask)[0])
    moved = F.with_first_point(pr["points3d"], pr["points3d"][j])
    Rm, tm = _lm_oracle(moved, pr["points2d"], pr["K"], mask, R0, t0)
    assert not (F.bits_equal(Rm, ref[0]) and F.bits_equal(tm, ref[1]))


@pytest.mark.parametrize("kind", sorted(F.BAD_FIRST))
@pytest.mark.parametrize("refine", [True, "epnp", "epnp+lm"])
def test_restated_chain_on_the_seed_9_problem_is_finite(refine, kind):
    pr = F.e2e_problem(kind)
    ref, R, t = F.ransac_chain(pr["points3d"], pr["points2d"], pr["K"], 2000, refine)
    assert ref["n_inliers"] == 419 and not ref["mask"][0]
    assert np.isfinite(ref["R"]).all() and np.isfinite(ref["t"]).all()
    assert R is not None and np.isfinite(R).all() and np.isfinite(t).all()
    # the RANSAC phase does not see the poisoned point: the clean problem's mask but for index 0
    clean = F.e2e_problem(None)
    cref = O.pnp_ransac(clean["points3d"], clean["points2d"], clean["K"], F.THR, F.CONF, 2000, F.SEED)
    np.testing.assert_array_equal(cref["mask"][1:], ref["mask"][1:])


def test_restated_lo_ransac_on_the_seed_9_problem_is_finite():
    pr = F.e2e_problem()
    lo = O.pnp_ransac_lo(pr["points3d"], pr["points2d"], pr["K"], F.THR, F.CONF, 5000)
    plain = O.pnp_ransac(pr["points3d"], pr["points2d"], pr["K"], F.THR, F.CONF, 5000, F.SEED)
    assert np.isfinite(lo["R"]).all() and np.isfinite(lo["t"]).all()
    assert lo["n_inliers"] >= plain["n_inliers"] > 0
