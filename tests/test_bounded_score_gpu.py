"""Bounded scoring of rsac_pnp_evaluate_range (DESIGN.md "Bounded scoring") against the CPU oracle.

The sequence (pass 0 over every point for the first hypotheses, pass 1 over the first n1 points,
pass 2 over the others for the hypotheses that can still reach pass 0's best count) is forced on
(RSAC_DBG_BOUND = 1) at small shapes.  Key, model and mask must equal the oracle's and the
unbounded call's (RSAC_DBG_BOUND = 2); the read-only hooks show that the call pruned, or fell back
to one whole pass, where the oracle's counts say it must.
"""
import numpy as np
import pytest

import pyoracle as O
import rsac
from rsac import _lib as L
from rsac import parallel as par
from rsac import synth

pytestmark = pytest.mark.gpu

THR, SEED, H0 = 30.0, 0x5EED, 256


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)  # its own context: the shared one keeps the default mode
    yield c
    c.close()


_ORACLE = {}


def _oracle(n, outl, seed, hb, H, scale=1.0):
    """problem, oracle counts / status, and the winner's key, model and mask (computed once)"""
    k = (n, outl, seed, hb, H, scale)
    if k not in _ORACLE:
        pr = dict(synth.pnp_problem(n, outl, seed=seed))
        pr["points3d"] = pr["points3d"] * scale
        soa, cam = O.soa_pnp(pr["points3d"], pr["points2d"]), O.cam_from_K(pr["K"])
        oc, os_, om = O.pnp_hypotheses(soa, cam, THR, SEED, H, hyp0=hb, models=True)
        okey = par.best_key_of(oc, os_, hb)
        ocnt, obest = par.unpack_key(okey)
        _, omask = O.pnp_count(om[obest - hb, :9].reshape(3, 3), om[obest - hb, 9:12], soa, cam, THR, mask=True)
        assert int(omask.sum()) == ocnt
        for a in (oc, os_, om, omask):
            a.setflags(write=False)
        _ORACLE[k] = dict(pr=pr, oc=oc, os=os_, key=okey, best=obest, model=om[obest - hb, :12], mask=omask)
    return _ORACLE[k]


def _run(ctx, o, hb, H, mode):
    ctx.debug_set(L.DBG_BOUND, mode)
    pr = o["pr"]
    key, model, mask = rsac.evaluate_range(pr["points2d"], pr["points3d"], pr["K"], hb, H, THR, with_mask=True,
                                           context=ctx)
    return key, model, mask, ctx.debug_get(L.DBG_BOUND_N1), ctx.debug_get(L.DBG_BOUND_SURVIVORS)


def _check(ctx, o, n, hb, H, prunes):
    key, model, mask, n1, S = _run(ctx, o, hb, H, 1)
    print(f"n={n} hb={hb} H={H}: n1={n1} survivors={S} of {H - H0}")
    assert key == o["key"]
    assert _bits_equal(model, o["model"])
    np.testing.assert_array_equal(mask, o["mask"])
    if prunes:
        assert n1 < n and S < H - H0
    else:
        assert n1 == n and S == 0
    key2, model2, mask2, n1_off, S_off = _run(ctx, o, hb, H, 2)
    assert (n1_off, S_off) == (n, 0)  # the unbounded call: one whole pass
    assert key2 == key and _bits_equal(model2, model)
    np.testing.assert_array_equal(mask2, mask)


# (n, outliers, seed, oracle best, B0 of the first 256, prunes): checked with the oracle
CASES = [(1500, 0.5, 7, 750, 750, True), (3000, 0.5, 7, 1502, 1502, True), (2500, 0.3, 8, 1752, 1752, True),
         (2000, 0.9, 9, 202, 8, False), (1000, 1.0, 10, 7, 7, False)]


@pytest.mark.parametrize("n,outl,seed,best,b0,prunes", CASES)
def test_bounded_equals_oracle_and_unbounded(ctx, n, outl, seed, best, b0, prunes):
    o = _oracle(n, outl, seed, 0, 2048)
    c = np.where(o["os"] > 0, o["oc"], 0)
    assert int(c.max()) == best and int(c[:H0].max()) == b0
    if not prunes and best > b0:
        assert o["best"] >= H0  # the fallback's winner lies outside pass 0
    _check(ctx, o, n, 0, 2048, prunes)


def test_bounded_odd_range(ctx):
    # a partial last tile in pass 1 and a partial last list tile in pass 2
    o = _oracle(3000, 0.5, 7, 3000, 2048 + 13)
    _check(ctx, o, 3000, 3000, 2048 + 13, True)


def test_bounded_winner_outside_pass0_while_pruning(ctx):
    # hypotheses [703, 703 + 2048) of this problem: pass 0's best (386) is below the range's best
    # (403, at index 462 of the range), so the winner is a survivor that pass 2 completes
    n, hb, H = 2000, 703, 2048
    o = _oracle(n, 0.8, 12, hb, H)
    c = np.where(o["os"] > 0, o["oc"], 0)
    b0, best = int(c[:H0].max()), int(c.max())
    assert o["best"] - hb >= H0 and b0 < best and b0 > 128 + 256  # n1 < N for any delta <= 128 rounded to 256
    _check(ctx, o, n, hb, H, True)


def test_bounded_n_not_multiple_of_64(ctx):
    o = _oracle(1501, 0.5, 7, 0, 2048)
    _check(ctx, o, 1501, 0, 2048, True)


def test_bounded_long_problem_all_cells(ctx):
    # above 16 384 points every tile of both passes runs by cells
    o = _oracle(20000, 0.5, 13, 0, 1024)
    _check(ctx, o, 20000, 0, 1024, True)


def test_bounded_async_equals_sync(ctx):
    import torch
    o = _oracle(3000, 0.5, 7, 0, 2048)
    pr = o["pr"]
    ctx.debug_set(L.DBG_BOUND, 1)
    p2, p3 = torch.from_numpy(pr["points2d"]).cuda(), torch.from_numpy(pr["points3d"]).cuda()
    key_t, model_t, mask_t = rsac.evaluate_range(p2, p3, pr["K"], 0, 2048, THR, with_mask=True, device_result=True,
                                                 context=ctx)
    torch.cuda.synchronize()
    n1, S = ctx.debug_get(L.DBG_BOUND_N1), ctx.debug_get(L.DBG_BOUND_SURVIVORS)
    assert n1 < 3000 and S < 2048 - H0
    key, model, mask, n1s, Ss = _run(ctx, o, 0, 2048, 1)
    assert (n1s, Ss) == (n1, S)
    assert int(key_t.item()) == key == o["key"]
    assert _bits_equal(model_t.cpu().numpy(), model)
    np.testing.assert_array_equal(mask_t.cpu().numpy(), mask)


def test_bounded_out_of_f16_range_falls_back(ctx):
    # centred coordinates above 2^15 (as test_pnp_batched_mixed_scales_equals_oracle builds them):
    # form-1 records, so the plan keeps the call to one whole pass
    o = _oracle(3000, 0.5, 7, 0, 2048, scale=1e3)
    assert int(np.where(o["os"] > 0, o["oc"], 0)[:H0].max()) > 1000  # (it would prune in range)
    _check(ctx, o, 3000, 0, 2048, False)
