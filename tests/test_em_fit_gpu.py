"""The calibrated essential-matrix refit and its local optimisation on the GPU (k_em_refine;
rsac_essential_refine_device, _batched_device, rsac_essential_local_opt, _batched, and
refine="pose" / "lo" of essential_ransac): every comparison of model bits, costs, masks, counts and
rounds is exact equality with the library's host refit, which tests/test_em_fit.py ties to the
independent reference of tests/emfitref.py, and with that file's restated loop.

Sizes: the summation order cuts the points into ranges of 4096 (walked by the problem's one block)
of 512 slots (one thread each) in waves of 64 -- 5 / 6 the model's minimum, 64 / 65 a wave, 512 / 513
a pass of the slots, 4096 / 4097 the first range boundary, 8193 the second.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import emfitref as R  # noqa: E402
import rsac  # noqa: E402
from rsac import synth  # noqa: E402

pytestmark = pytest.mark.gpu

SEED, CONF = 0x5EED, 0.999
K2 = np.array([[900.0, 0, 700.0], [0, 950.0, 500.0], [0, 0, 1]])
SIZES = [5, 6, 64, 65, 512, 513, 4096, 4097, 8193]


def _bits_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _same(got, want):
    """(E, EssentialFitInfo) pairs: every field to the bit"""
    (Eg, ig), (Ew, iw) = got, want
    return (_bits_equal(Eg, Ew) and _bits_equal(ig.F, iw.F) and _bits_equal([ig.cost], [iw.cost]) and
            ig.count == iw.count and ig.steps == iw.steps)


def _np(m):
    return m.cpu().numpy() if hasattr(m, "cpu") else np.asarray(m)


def _dev(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device="cuda", dtype=dtype)


def _second_view(pts2, K):
    """the second view's pixels under the intrinsics K2 instead of K"""
    return (np.c_[pts2, np.ones(len(pts2))] @ (K2 @ np.linalg.inv(K)).T)[:, :2]


@functools.lru_cache(maxsize=None)
def _problem(n):
    pr = synth.essential_problem(n, 0.0 if n < 20 else 0.3, seed=100 + n)
    E0 = R.start_of(pr, 1.0, n)
    return pr["pts1"], pr["pts2"], pr["K"], E0, pr["E"]


def _masks(p1, p2, K, Et):
    """None = all, every third point dropped, and a winner's mask: the true model's at 1 px"""
    n = len(p1)
    return {"ones": None, "third": np.arange(n) % 3 != 0, "winner": R.mask_of(p1, p2, rsac.essential_to_fundamental(Et, K))}


@pytest.mark.parametrize("n", SIZES)
def test_device_refit_equals_host_refit(n):
    import torch
    p1, p2, K, E0, Et = _problem(n)
    q2 = _second_view(p2, K)
    t1, t2, s1, s2 = _dev(p1), _dev(p2), _dev(p1.T, torch.float32), _dev(p2.T, torch.float32)
    tq, sq = _dev(q2), _dev(q2.T, torch.float32)
    models = 0
    for name, mask in _masks(p1, p2, K, Et).items():
        dm = None if mask is None else _dev(mask)
        for k2, b, tb, sb in ((None, p2, t2, s2), (K2, q2, tq, sq)):
            want = rsac.essential_refine(p1, b, K, E0, mask, K2=k2, return_info=True)
            ones = n if mask is None else int(mask.sum())
            assert want[1].count == ones and (ones >= 5 or want[0] is None), (name, ones)
            models += want[0] is not None
            assert _same(rsac.essential_refine(p1, b, K, E0, mask, K2=k2, device=0, return_info=True), want), name  # AoS host
            assert _same(rsac.essential_refine(t1, tb, K, E0, dm, K2=k2, return_info=True), want), name  # device tensors
            assert _same(rsac.essential_refine(s1, sb, K, E0, dm, K2=k2, return_info=True), want), name  # f32 SoA
    assert models >= (6 if n >= 64 else 2)  # n = 5, 6: "third" leaves 3 and 4 points


def test_device_refit_edge_cases():
    p1, p2, K, E0, _ = (np.copy(a) for a in _problem(4097))
    mask = np.arange(4097) % 3 != 0
    want = rsac.essential_refine(p1, p2, K, E0, mask, return_info=True)
    p1[0], p2[3], p1[4095, 1], p2[4092, 0] = np.nan, np.inf, -np.inf, np.nan  # indices with i % 3 == 0: never read
    assert _same(rsac.essential_refine(_dev(p1), _dev(p2), K, E0, _dev(mask), return_info=True), want)
    p1[4096, 0] = np.nan  # under the mask, the second range's only point: no model on both sides
    assert rsac.essential_refine(p1, p2, K, E0, mask) is None
    E, info = rsac.essential_refine(_dev(p1), _dev(p2), K, E0, _dev(mask), return_info=True)
    assert E is None and info.count == int(mask.sum())
    q1, q2 = _problem(65)[:2]
    a, b = np.array([1.0, 2, 3]), np.array([-0.5, 0.25, 1])
    for Ebad in (np.outer(a, b), np.zeros((3, 3)), np.full((3, 3), np.nan)):  # rank 1, zero, NaN: the block leaves at once
        E, info = rsac.essential_refine(q1, q2, K, Ebad, device=0, return_info=True)
        assert E is None and info.count == 0
    Ks = K.copy()
    Ks[1] = 2.0 * Ks[0]
    with pytest.raises(rsac.RsacError):
        rsac.essential_refine(q1, q2, Ks, E0, device=0)
    with pytest.raises(rsac.RsacError):
        rsac.essential_local_opt(q1, q2, K, E0, K2=Ks)


def _batch(P):
    """P problems of mixed sizes with per-problem intrinsics; problem 1 has fewer than 5 masked
    points and problem 2's E is missing (where the batch has them)"""
    sizes = [SIZES[(4 * p + 2) % len(SIZES)] for p in range(P)]
    p1s, p2s, Ks, K2s, Es, masks = [], [], [], [], [], []
    for p, n in enumerate(sizes):
        p1, p2, K, E0, Et = _problem(n)
        k2 = K2 if p % 2 else K
        p1s.append(p1)
        p2s.append(_second_view(p2, K) if p % 2 else p2)
        Ks.append(K)
        K2s.append(k2)
        m = R.mask_of(p1, p2s[-1], rsac.essential_to_fundamental(Et, K, k2)) if p % 3 else np.arange(n) % 3 != 0
        if p == 1:
            m = np.zeros(n, bool)
            m[:4] = True
        masks.append(m)
        Es.append(None if p == 2 else E0)
    return p1s, p2s, np.array(Ks), np.array(K2s), Es, masks


@pytest.mark.parametrize("P", [1, 3, 17])
def test_batched_refit_equals_single(P):
    p1s, p2s, Ks, K2s, Es, masks = _batch(P)
    want = [rsac.essential_refine(p1s[p], p2s[p], Ks[p], np.zeros(9) if Es[p] is None else Es[p], masks[p], K2=K2s[p],
                                  return_info=True) for p in range(P)]
    if P > 1:
        assert want[1][0] is None and want[1][1].count == 4
    if P > 2:
        assert want[2][0] is None
    assert sum(w[0] is not None for w in want) >= P - 4
    got = rsac.essential_refine_batched(p1s, p2s, Ks, Es, masks, K2=K2s, return_info=True)
    assert len(got) == P and all(_same(got[p], want[p]) for p in range(P))
    dev = rsac.essential_refine_batched([_dev(a) for a in p1s], [_dev(a) for a in p2s], Ks, Es, [_dev(m) for m in masks],
                                        K2=K2s, return_info=True)
    assert all(_same(dev[p], want[p]) for p in range(P))
    # no masks: every point of every problem
    all_pts = rsac.essential_refine_batched(p1s, p2s, Ks, Es, None, K2=K2s)
    for p in range(P):
        single = None if Es[p] is None else rsac.essential_refine(p1s[p], p2s[p], Ks[p], Es[p], K2=K2s[p])
        assert _bits_equal(all_pts[p], single)


@functools.lru_cache(maxsize=None)
def _lo_case(key, rounds):
    pr = R.problem(key)
    E0 = R.start_of(pr, *R.STARTS[1])
    return pr, E0, R.local_opt(pr["pts1"], pr["pts2"], pr["K"], E0, R.THR, rounds)


@pytest.mark.parametrize("key", R.INPUTS)
@pytest.mark.parametrize("rounds", [2, 8])
def test_local_opt_equals_restated_loop(key, rounds):
    pr, E0, (E, mask, count, steps, trail) = _lo_case(key, rounds)
    p1, p2, K = pr["pts1"], pr["pts2"], pr["K"]
    assert steps >= 1 and count > trail[0]
    got = rsac.essential_local_opt(p1, p2, K, E0, R.THR, max_rounds=rounds)
    assert _bits_equal(got[0], E) and np.array_equal(got[1], mask) and got[2:] == (count, steps)
    dev = rsac.essential_local_opt(_dev(p1), _dev(p2), K, E0, R.THR, max_rounds=rounds)
    assert _bits_equal(dev[0], E) and np.array_equal(_np(dev[1]), mask) and dev[2:] == (count, steps)
    assert dev[1].is_cuda


def test_local_opt_batched_equals_single_and_freezes():
    """the six inputs side by side: their loops end after 6, 2, 5, 5, 1 and 8 accepted rounds, so all
    but the last are frozen while others still rise; a missing E and a problem of 4 points ride along"""
    want, p1s, p2s, Es = [], [], [], []
    for key in R.INPUTS:
        pr, E0, (E, mask, count, steps, _) = _lo_case(key, 8)
        want.append((E, mask, count, steps))
        p1s.append(pr["pts1"])
        p2s.append(pr["pts2"])
        Es.append(E0)
    assert len({w[3] for w in want}) >= 4
    K = R.problem(R.INPUTS[0])["K"]
    p1s += [p1s[0], p1s[1][:4]]
    p2s += [p2s[0], p2s[1][:4]]
    Es += [None, Es[1]]
    got = rsac.essential_local_opt_batched(p1s, p2s, K, Es, R.THR, max_rounds=8)
    for p, w in enumerate(want):
        assert _bits_equal(got[p][0], w[0]) and np.array_equal(got[p][1], w[1]) and got[p][2:] == w[2:], p
    assert got[6][0] is None and not got[6][1].any() and got[6][2:] == (0, 0)
    four = rsac.essential_local_opt(p1s[7], p2s[7], K, Es[7], R.THR, max_rounds=8)
    assert _bits_equal(got[7][0], four[0]) and np.array_equal(got[7][1], four[1]) and got[7][2:] == four[2:]
    assert four[3] == 0 and four[2] <= 4 and _bits_equal(four[0], Es[7])
    dev = rsac.essential_local_opt_batched([_dev(a) for a in p1s], [_dev(a) for a in p2s], K, Es, R.THR, max_rounds=8)
    for p in range(len(p1s)):
        assert _bits_equal(dev[p][0], got[p][0]) and np.array_equal(_np(dev[p][1]), got[p][1]) and dev[p][2:] == got[p][2:]


@pytest.mark.parametrize("key", [(200, .3, 3, .5), (2000, .5, 2, .5)])
def test_ransac_refine_pose_and_lo(key):
    pr = R.problem(key)
    p1, p2, K = pr["pts1"], pr["pts2"], pr["K"]
    kw = dict(seed=SEED, confidence=CONF, max_iters=200)
    E0, m0, F0, i0 = rsac.essential_ransac(p1, p2, K, R.THR, refine=False, return_F=True, return_info=True, **kw)
    assert E0 is not None
    E, m, F, info = rsac.essential_ransac(p1, p2, K, R.THR, refine="pose", return_F=True, return_info=True, **kw)
    want = rsac.essential_refine(p1, p2, K, E0, m0)
    assert want is not None and _bits_equal(E, want) and np.array_equal(m, m0) and info.n_inliers == i0.n_inliers
    Fn = np.linalg.inv(K).T @ E @ np.linalg.inv(K)
    assert _bits_equal(F, rsac.essential_to_fundamental(E, K)) and R.sign_distance(F, Fn / np.linalg.norm(Fn)) <= 1e-12
    dE, dm, dF = rsac.essential_ransac(_dev(p1), _dev(p2), K, R.THR, refine="pose", return_F=True, **kw)
    assert _bits_equal(dE, E) and np.array_equal(_np(dm), m0) and _bits_equal(dF, F)
    E, m, F, info = rsac.essential_ransac(p1, p2, K, R.THR, refine="lo", return_F=True, return_info=True, **kw)
    lo = rsac.essential_local_opt(p1, p2, K, E0, R.THR)
    assert _bits_equal(E, lo[0]) and np.array_equal(m, lo[1]) and (info.n_inliers, info.lo_improvements) == lo[2:]
    assert info.n_inliers >= i0.n_inliers and info.n_inliers == int(m.sum())
    assert _bits_equal(F, rsac.essential_to_fundamental(E, K))
    # refine=False / True are what they were: the first call's outputs again, and the projected 8-point fit
    Et, mt, Ft = rsac.essential_ransac(p1, p2, K, R.THR, refine=True, return_F=True, **kw)
    assert np.array_equal(mt, m0) and _bits_equal(Et, rsac.essential_from_fundamental(Ft, K))
    assert _bits_equal(Ft, rsac.fundamental_fit(p1, p2, m0))


def test_ransac_batched_refine_pose_and_lo():
    keys = [(200, .3, 3, .5), (500, .5, 4, .5), (64, .3, 2, .5)]
    p1s = [R.problem(k)["pts1"] for k in keys]
    K = R.problem(keys[0])["K"]
    K2s = np.array([K, K2, K])
    p2s = [R.problem(k)["pts2"] if i != 1 else _second_view(R.problem(k)["pts2"], K) for i, k in enumerate(keys)]
    kw = dict(seed=SEED, confidence=CONF, max_iters=200, K2=K2s, return_F=True)
    base = rsac.essential_ransac_batched(p1s, p2s, K, R.THR, refine=False, **kw)
    pose = rsac.essential_ransac_batched(p1s, p2s, K, R.THR, refine="pose", **kw)
    lo = rsac.essential_ransac_batched(p1s, p2s, K, R.THR, refine="lo", **kw)
    for p in range(len(keys)):
        E0, m0, c0, F0 = base[p]
        assert E0 is not None
        single = rsac.essential_ransac(p1s[p], p2s[p], K, R.THR, K2=K2s[p], seed=SEED, confidence=CONF, max_iters=200)
        assert _bits_equal(single[0], E0) and np.array_equal(single[1], m0)
        E, m, c, F = pose[p]
        assert _bits_equal(E, rsac.essential_refine(p1s[p], p2s[p], K, E0, m0, K2=K2s[p])) and np.array_equal(m, m0) and c == c0
        assert _bits_equal(F, rsac.essential_to_fundamental(E, K, K2s[p]))
        E, m, c, F = lo[p]
        want = rsac.essential_local_opt(p1s[p], p2s[p], K, E0, R.THR, K2=K2s[p])
        assert _bits_equal(E, want[0]) and np.array_equal(m, want[1]) and c == want[2] >= c0
        assert _bits_equal(F, rsac.essential_to_fundamental(E, K, K2s[p]))


def _pose_errors(pr, E, mask):
    Rm, t, _ = rsac.recover_pose(pr["pts1"], pr["pts2"], pr["K"], E, mask)
    if Rm is None:
        return float("nan"), float("nan")
    rot = np.degrees(np.arccos(np.clip((np.trace(Rm @ pr["R"].T) - 1.0) / 2.0, -1.0, 1.0)))
    tt = pr["t"] / np.linalg.norm(pr["t"])
    return float(rot), float(np.degrees(np.arccos(np.clip(t @ tt, -1.0, 1.0))))


def test_end_to_end_report():
    """(2000, .5, 2, .5) at 1 px: the counts at 1 px and the pose errors of recover_pose for the four
    refine modes are printed; asserted is only what follows by construction.  The "pose" cost is
    compared with NumPy's evaluation of the minimal model's cost on the same mask, which differs from
    the library's own pass 0 by rounding alone (1e-14 relative measured; the slack is
    tests/test_em_fit.py's COST_MARGIN)."""
    key = (2000, .5, 2, .5)
    pr = R.problem(key)
    p1, p2, K = pr["pts1"], pr["pts2"], pr["K"]
    out = {}
    for mode in (False, True, "pose", "lo"):
        E, m, F = rsac.essential_ransac(p1, p2, K, R.THR, seed=SEED, refine=mode, return_F=True)
        assert E is not None
        reached = int(R.mask_of(p1, p2, rsac.essential_to_fundamental(E, K)).sum())
        rot, tr = _pose_errors(pr, E, m)
        out[mode] = (E, m, reached)
        print(f"refine={mode!r}: mask {int(m.sum())} inliers at 1 px of the E returned {reached} "
              f"true {int((m & pr['inlier']).sum())} rotation {rot:.4f} deg translation {tr:.4f} deg")
    E0, m0, _ = out[False]
    Ep, mp, _ = out["pose"]
    assert np.array_equal(mp, m0)
    assert R.cost_of(Ep, p1, p2, K, None, m0) <= R.cost_of(E0, p1, p2, K, None, m0) * (1.0 + 100 * 1.31e-13)
    assert int(out["lo"][1].sum()) >= int(m0.sum()) and out["lo"][2] == int(out["lo"][1].sum())
