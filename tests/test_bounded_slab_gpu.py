"""The slab body of the bounded sequence's pass 1 against the CPU oracle.

Where pass 1 is cut short (n1 < N) it no longer counts exactly: a pair is counted unless one
coordinate alone proves it an outlier, so a hypothesis's pass-1 figure is an upper bound of its
count, the survivors are recounted over every point, and the call's key, model and mask must still
be the oracle's.  RSAC_DBG_BOUND_SLAB = 1 runs the exact body as before.  The bounded sequence is
forced on (RSAC_DBG_BOUND = 1) at small shapes; threshold and seed as tests/test_bounded_score_gpu.py.

The edge-winner test asserts that the moved pixels lie within thr 2^-11 px of the threshold: the
offsets it is built from, thr (1 -+ 2^-12), are 0.0073 px from it at thr = 30, so that is the
tightest figure the construction allows (2^-10 px would be 0.00098 px).
"""
import numpy as np
import pytest
import torch

import pyoracle as O
import rsac
from rsac import _lib as L
from rsac import parallel as par
from rsac import synth

pytestmark = pytest.mark.gpu

THR, SEED, H0, DELTA = 30.0, 0x5EED, 256, 128


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


@pytest.fixture()
def ctx():
    c = L.Context(0)  # a fresh context per test: no record of an earlier call
    c.debug_set(L.DBG_BOUND, 1)
    yield c
    c.close()


_ORACLE = {}


def _solve(pr, hb, H):
    """oracle counts / status / models of a problem's range and the winner's key, model and mask"""
    n = len(pr["points3d"])
    soa, cam = O.soa_pnp(pr["points3d"], pr["points2d"]), O.cam_from_K(pr["K"])
    oc, os_, om = O.pnp_hypotheses(soa, cam, THR, SEED, H, hyp0=hb, models=True)
    okey = par.best_key_of(oc, os_, hb)
    ocnt, obest = par.unpack_key(okey)
    omask = np.zeros(n, np.uint8)
    omodel = np.zeros(12)
    if okey > 0:
        _, omask = O.pnp_count(om[obest - hb, :9].reshape(3, 3), om[obest - hb, 9:12], soa, cam, THR, mask=True)
        assert int(omask.sum()) == ocnt
        omodel = om[obest - hb, :12]
    for a in (oc, os_, om, omask):
        a.setflags(write=False)
    return dict(pr=pr, soa=soa, cam=cam, oc=oc, os=os_, om=om, key=okey, best=obest, model=omodel, mask=omask,
                hb=hb, H=H)


def _oracle(n, outl, seed, hb, H, scale=1.0):
    k = (n, outl, seed, hb, H, scale)
    if k not in _ORACLE:
        pr = dict(synth.pnp_problem(n, outl, seed=seed))
        pr["points3d"] = pr["points3d"] * scale
        _ORACLE[k] = _solve(pr, hb, H)
    return _ORACLE[k]


def _b0_n1(o):
    """the plan's B0 and n1 (bound_n1_of, in the f16 range) from the oracle's first H0 counts"""
    n = len(o["mask"])
    B0 = int(np.where(o["os"][:H0] > 0, o["oc"][:H0], 0).max())
    return B0, (min(n, (n - B0 + DELTA + 255) // 256 * 256) if B0 > DELTA else n)


def _oracle_survivors(o):
    """the exact mode's list length: hypotheses past H0 with c1 + (N - n1) >= B0, c1 from pnp_count"""
    n = len(o["mask"])
    B0, n1 = _b0_n1(o)
    if n1 >= n:
        return 0
    head = tuple(np.ascontiguousarray(a[:n1]) for a in o["soa"])
    S = 0
    for j in range(H0, o["H"]):
        c1 = O.pnp_count(o["om"][j, :9].reshape(3, 3), o["om"][j, 9:12], head, o["cam"], THR) if o["os"][j] > 0 else 0
        S += c1 + (n - n1) >= B0
    return S


def _dev(o):
    pr = o["pr"]
    return (torch.from_numpy(np.ascontiguousarray(pr["points2d"])).cuda(),
            torch.from_numpy(np.ascontiguousarray(pr["points3d"])).cuda())


def _call(ctx, p2, p3, o):
    """one synchronous call -> (hinted, n1, S), after the comparison with the oracle"""
    key, model, mask = rsac.evaluate_range(p2, p3, o["pr"]["K"], o["hb"], o["H"], THR, with_mask=True, context=ctx)
    hinted = ctx.debug_get(L.DBG_BOUND_HINTED)
    n1, S = ctx.debug_get(L.DBG_BOUND_N1), ctx.debug_get(L.DBG_BOUND_SURVIVORS)
    print(f"hb={o['hb']} H={o['H']} slab_mode={ctx.debug_get(L.DBG_BOUND_SLAB)}: key={key} hinted={hinted} n1={n1} S={S}")
    assert key == (o["key"] if o["key"] > 0 else -1)
    if o["key"] > 0:
        assert _bits_equal(model, o["model"])
    np.testing.assert_array_equal(mask.cpu().numpy(), o["mask"])
    return hinted, n1, S


def test_slab_selftest(ctx):
    ctx.debug_set(L.DBG_SLAB_SELFTEST, 4 << 20)
    assert ctx.debug_get(L.DBG_SLAB_SELFTEST) == 0


@pytest.mark.parametrize("n,outl,seed,hb,H", [(1500, 0.5, 7, 0, 2048), (2500, 0.3, 8, 0, 2048),
                                              (2000, 0.8, 12, 703, 2048), (1501, 0.5, 7, 0, 2048),
                                              (20000, 0.5, 13, 0, 1024)])
def test_slab_on_and_off(n, outl, seed, hb, H):
    o = _oracle(n, outl, seed, hb, H)
    p2, p3 = _dev(o)
    B0, n1o = _b0_n1(o)
    assert n1o < n
    got = {}
    for mode in (1, 0):  # the exact body, then the slab: plain (five launches) and hinted calls, own contexts
        c = L.Context(0)
        try:
            c.debug_set(L.DBG_BOUND, 1)
            c.debug_set(L.DBG_BOUND_SLAB, mode)
            plain = _call(c, p2, p3, o)
            hinted = _call(c, p2, p3, o)
        finally:
            c.close()
        assert plain[0] == 0 and hinted[0] == 1 and plain[1:] == hinted[1:]
        assert plain[1] == n1o
        got[mode] = plain[2]
    assert got[1] == _oracle_survivors(o)
    assert got[1] <= got[0] < H - H0


def _edge_problem(sign):
    """(3000, 0.5, 7): every inlier of the best hypothesis past H0, but its four sample points, moved to
    its projection -+ thr (1 + sign 2^-12) in u and 0 in v -> the changed problem's oracle record"""
    k = ("edge", sign)
    if k in _ORACLE:
        return _ORACLE[k]
    base = _oracle(3000, 0.5, 7, 0, 2048)
    cnt = np.where(base["os"] > 0, base["oc"], 0)
    w = H0 + int(np.argmax(cnt[H0:]))
    R, t = base["om"][w, :9].reshape(3, 3), base["om"][w, 9:12]
    pr = dict(base["pr"])
    n = len(pr["points3d"])
    p3r = pr["points3d"].astype(np.float32).astype(np.float64)  # what the inlier test projects
    _, proj = O.reproj_errors(p3r, pr["points2d"], pr["K"], R, t, projections=True)
    _, inl = O.pnp_count(R, t, base["soa"], base["cam"], THR, mask=True)
    sample = O.philox_subset(SEED, 0, w, n, 4)
    move = np.flatnonzero(inl)
    move = move[~np.isin(move, sample)]
    off = THR * (1.0 + sign * 2.0 ** -12) * np.where(np.arange(len(move)) % 2 == 0, 1.0, -1.0)
    px = np.array(pr["points2d"], np.float64, copy=True)
    px[move, 0] = (proj[move, 0] + off).astype(np.float32)
    px[move, 1] = proj[move, 1].astype(np.float32)
    pr["points2d"] = px
    o = _solve(pr, 0, 2048)
    o["w"], o["moved"], o["proj"] = w, move, proj
    _ORACLE[k] = o
    return o


@pytest.mark.parametrize("sign", [-1, +1])
def test_winner_on_the_slabs_edge(ctx, sign):
    o = _edge_problem(sign)
    B0, n1 = _b0_n1(o)
    n = len(o["mask"])
    assert B0 > DELTA + 256 and n1 < n
    head = o["moved"][o["moved"] < n1]
    du = np.abs(o["pr"]["points2d"][head, 0].astype(np.float32).astype(np.float64) - o["proj"][head, 0])
    assert len(head) > 100 and np.all(np.abs(du - THR) <= THR * 2.0 ** -11)
    assert np.all(o["pr"]["points2d"][head, 1] == o["proj"][head, 1].astype(np.float32))
    _, m = O.pnp_count(o["om"][o["w"], :9].reshape(3, 3), o["om"][o["w"], 9:12], o["soa"], o["cam"], THR, mask=True)
    if sign < 0:  # the moved points are still inliers of the hypothesis, and the winner is still past H0
        assert o["best"] >= H0 and np.all(m[o["moved"]])
    else:  # ... its outliers
        assert not np.any(m[o["moved"]])
    p2, p3 = _dev(o)
    plain = _call(ctx, p2, p3, o)
    hinted = _call(ctx, p2, p3, o)
    assert plain[0] == 0 and hinted[0] == 1 and plain[1] == n1 and plain[1:] == hinted[1:]


def test_depth_edges(ctx):
    # for the good model: 64 points within 1e-6 of the camera plane and 64 mirrored behind the camera
    base = _oracle(1500, 0.5, 7, 0, 2048)
    if "depth" not in _ORACLE:
        pr = dict(base["pr"])
        R, t = pr["R"], pr["t"]
        rng = np.random.default_rng(5)
        on_plane = np.c_[rng.normal(size=(64, 2)) * 50.0, rng.uniform(-1e-6, 1e-6, 64)]
        good = np.flatnonzero(pr["inlier"])[:64]
        mirrored = -(pr["points3d"][good] @ R.T + t)
        extra_w = (np.concatenate([on_plane, mirrored]) - t) @ R
        pr["points3d"] = np.concatenate([pr["points3d"], extra_w])
        pr["points2d"] = np.concatenate([pr["points2d"], rng.uniform(0, 2000, size=(64, 2)), pr["points2d"][good]])
        _ORACLE["depth"] = _solve(pr, 0, 2048)
    o = _ORACLE["depth"]
    n = len(o["mask"])
    assert n == 1500 + 128 and _b0_n1(o)[1] < n
    p2, p3 = _dev(o)
    plain = _call(ctx, p2, p3, o)
    hinted = _call(ctx, p2, p3, o)
    assert plain[0] == 0 and hinted[0] == 1 and plain[1] < n and plain[1:] == hinted[1:]


@pytest.mark.parametrize("other", ["fallback", "out_of_range"])
@pytest.mark.parametrize("prune_first", [True, False])
def test_fallback_and_range_guards(ctx, other, prune_first):
    # (2000, 0.9, 9): no hypothesis of the first 256 passes delta, one whole exact pass;
    # (3000, 0.5, 7) x 1e3: outside the f16 operand range, one whole pass of the form-1 body.
    # Each before and after an in-range pruning problem in the same tensors.
    if other == "fallback":
        oo, op = _oracle(2000, 0.9, 9, 0, 2048), _oracle(2000, 0.5, 7, 0, 2048)
    else:
        oo, op = _oracle(3000, 0.5, 7, 0, 2048, 1e3), _oracle(3000, 0.5, 7, 0, 2048)
    n = len(oo["mask"])
    order = [op, oo] if prune_first else [oo, op]
    p2, p3 = _dev(order[0])
    first = _call(ctx, p2, p3, order[0])
    assert first[0] == 0
    q2, q3 = _dev(order[1])
    p2.copy_(q2)
    p3.copy_(q3)
    second = _call(ctx, p2, p3, order[1])  # under the first problem's hint
    assert second[0] == 1
    third = _call(ctx, p2, p3, order[1])
    assert third[0] == 1
    whole, pruned = (second, first) if prune_first else (first, second)
    assert pruned[1] <= n and pruned[2] < 2048 - H0
    if other == "out_of_range" or not prune_first:
        assert whole[1:] == (n, 0)  # (the fallback problem under a pruning hint keeps that hint's n1)
    if prune_first:
        assert third[1:] == (n, 0)
    else:
        assert third[1] < n and third[2] < 2048 - H0
