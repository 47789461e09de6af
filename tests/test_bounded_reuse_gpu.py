"""Set-up reuse and the hinted bounded sequence of rsac_pnp_evaluate_range against
the CPU oracle.

Successive calls on one context with the same device tensors skip the per-problem set-up
(RSAC_F_POINTS_UNCHANGED) and take pass 1's n1 from the record the previous call left on the device
(pass 0 inside pass 1's launch, the plan inside select).  Every result must still equal the
oracle's (key equal, model bit-equal, mask equal), the read-only hooks RSAC_DBG_SETUP_REUSED and
RSAC_DBG_BOUND_HINTED must show which path ran, a stale hint must change nothing but n1 (and nothing at all outside the f16 range), and
everything that can change the set-up's inputs or outputs must bring the set-up back.  Also the
unbounded path under reuse (a one-tile range), calls without a mask, and inputs that can never be
reused (inference-mode tensors, inputs the wrapper copies).  As
tests/test_bounded_score_gpu.py: the bounded sequence forced on (RSAC_DBG_BOUND = 1), its
threshold and seed.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import pyoracle as O
import rsac
from rsac import _lib as L
from rsac import parallel as par
from rsac import synth

pytestmark = pytest.mark.gpu

THR, SEED, H0 = 30.0, 0x5EED, 256


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


@pytest.fixture()
def ctx():
    c = L.Context(0)  # a fresh context per test: no record of an earlier call
    c.debug_set(L.DBG_BOUND, 1)
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
        omask = np.zeros(n, np.uint8)
        omodel = np.zeros(12)
        if okey > 0:
            _, omask = O.pnp_count(om[obest - hb, :9].reshape(3, 3), om[obest - hb, 9:12], soa, cam, THR, mask=True)
            assert int(omask.sum()) == ocnt
            omodel = om[obest - hb, :12]
        for a in (oc, os_, om, omask):
            a.setflags(write=False)
        _ORACLE[k] = dict(pr=pr, oc=oc, os=os_, key=okey, best=obest, model=omodel, mask=omask)
    return _ORACLE[k]


def _dev(o):
    # contiguous (n, 2) and (n, 3) float64 tensors: the layout the wrapper hands over without a copy
    # (synth's pixel array is column-major from 16 384 points on; a copy per call is another tensor)
    pr = o["pr"]
    return (torch.from_numpy(np.ascontiguousarray(pr["points2d"])).cuda(),
            torch.from_numpy(np.ascontiguousarray(pr["points3d"])).cuda())


def _call(ctx, p2, p3, o, hb, H, **kw):
    """one synchronous call on device tensors -> (reused, hinted, n1, S), after the oracle comparison"""
    key, model, mask = rsac.evaluate_range(p2, p3, o["pr"]["K"], hb, H, THR, with_mask=True, context=ctx, **kw)
    reused, hinted = ctx.debug_get(L.DBG_SETUP_REUSED), ctx.debug_get(L.DBG_BOUND_HINTED)
    n1, S = ctx.debug_get(L.DBG_BOUND_N1), ctx.debug_get(L.DBG_BOUND_SURVIVORS)
    print(f"hb={hb} H={H}: key={key} reused={reused} hinted={hinted} n1={n1} S={S}")
    assert key == (o["key"] if o["key"] > 0 else -1)
    if o["key"] > 0:
        assert _bits_equal(model, o["model"])
    np.testing.assert_array_equal(mask.cpu().numpy(), o["mask"])
    return reused, hinted, n1, S


def test_same_problem_three_times(ctx):
    o = _oracle(3000, 0.5, 7, 0, 2048)
    p2, p3 = _dev(o)
    r1, h1, n1, S = _call(ctx, p2, p3, o, 0, 2048)
    assert (r1, h1) == (0, 0) and n1 < 3000 and S < 2048 - H0
    for _ in range(2):
        assert _call(ctx, p2, p3, o, 0, 2048) == (1, 1, n1, S)


def test_another_range_on_the_same_points(ctx):
    # the second range has a partial last tile and a partial last list tile
    o1, o2 = _oracle(3000, 0.5, 7, 0, 2048), _oracle(3000, 0.5, 7, 3000, 2048 + 13)
    p2, p3 = _dev(o1)
    assert _call(ctx, p2, p3, o1, 0, 2048)[:2] == (0, 0)
    r, h, n1, S = _call(ctx, p2, p3, o2, 3000, 2048 + 13)
    assert (r, h) == (1, 1) and n1 < 3000 and S < 2048 + 13 - H0


def test_winner_outside_the_first_256_reused(ctx):
    o = _oracle(2000, 0.8, 12, 703, 2048)
    assert o["best"] - 703 >= H0
    p2, p3 = _dev(o)
    first = _call(ctx, p2, p3, o, 703, 2048)
    assert first[:2] == (0, 0) and first[2] < 2000
    assert _call(ctx, p2, p3, o, 703, 2048) == (1, 1) + first[2:]


def test_in_place_change_of_the_points(ctx):
    # problem B copied into A's tensors: _version moves, the set-up runs again and the result is B's
    oa = _oracle(3000, 0.5, 7, 0, 2048)
    ob = _oracle(3000, 0.8, 11, 0, 2048)
    p2, p3 = _dev(oa)
    b2, b3 = _dev(ob)
    a2, a3 = p2.clone(), p3.clone()
    cb = np.where(ob["os"] > 0, ob["oc"], 0)
    assert int(cb[:H0].max()) > 128 + 256  # B prunes too, at a larger n1 than A (fewer inliers)
    _, _, n1a, _ = _call(ctx, p2, p3, oa, 0, 2048)
    p2.copy_(b2)
    p3.copy_(b3)
    r, h, n1, _ = _call(ctx, p2, p3, ob, 0, 2048)  # B under A's hint: too small, and still B's result
    assert (r, h, n1) == (0, 1, n1a)
    r, h, n1b, _ = _call(ctx, p2, p3, ob, 0, 2048)
    assert (r, h) == (1, 1) and n1a < n1b < 3000
    p3.copy_(a3)
    p2.copy_(a2)
    assert _call(ctx, p2, p3, oa, 0, 2048)[:3] == (0, 1, n1b)  # A under B's larger hint
    assert _call(ctx, p2, p3, oa, 0, 2048)[:3] == (1, 1, n1a)
    # reuse switched off by the caller (the hint does not depend on the points' values)
    assert _call(ctx, p2, p3, oa, 0, 2048, reuse_setup=False)[:3] == (0, 1, n1a)


def test_fallback_problem_twice(ctx):
    o = _oracle(2000, 0.9, 9, 0, 2048)
    p2, p3 = _dev(o)
    assert _call(ctx, p2, p3, o, 0, 2048) == (0, 0, 2000, 0)
    assert _call(ctx, p2, p3, o, 0, 2048) == (1, 1, 2000, 0)
    # an easy problem of the same n copied in: one call under the hint N, and the next one prunes
    oe = _oracle(2000, 0.5, 7, 0, 2048)
    e2, e3 = _dev(oe)
    p2.copy_(e2)
    p3.copy_(e3)
    assert _call(ctx, p2, p3, oe, 0, 2048) == (0, 1, 2000, 0)
    r, h, n1, S = _call(ctx, p2, p3, oe, 0, 2048)
    assert (r, h) == (1, 1) and n1 < 2000 and S < 2048 - H0


@pytest.mark.parametrize("n,outl,seed,H,scale,prunes", [(1501, 0.5, 7, 2048, 1.0, True),
                                                        (20000, 0.5, 13, 1024, 1.0, True),
                                                        (3000, 0.5, 7, 2048, 1e3, False)])
def test_edges_twice(ctx, n, outl, seed, H, scale, prunes):
    # n no multiple of 64; every tile by cells in both passes; out of the f16 range (one whole pass)
    o = _oracle(n, outl, seed, 0, H, scale)
    p2, p3 = _dev(o)
    r1 = _call(ctx, p2, p3, o, 0, H)
    r2 = _call(ctx, p2, p3, o, 0, H)
    assert r1[:2] == (0, 0) and r2[:2] == (1, 1) and r1[2:] == r2[2:]
    assert (r1[2] < n and r1[3] < H - H0) if prunes else r1[2:] == (n, 0)


def _ransac(c, p2, p3, o):
    """rsac_pnp_ransac (256 iterations, adaptive off, no refit) on device points through context c ->
    (code, R, t, mask bytes, inliers, best hypothesis)"""
    R, t, mask, st = np.zeros(9), np.zeros(3), np.zeros(p3.shape[0], np.uint8), L.Stats()
    K9 = np.ascontiguousarray(o["pr"]["K"], np.float64).reshape(9)
    with c.lock:
        code = L.check(L.lib().rsac_pnp_ransac(c.handle, C.c_void_p(p3.data_ptr()), C.c_void_p(p2.data_ptr()),
                                               p3.shape[0], K9.ctypes.data, 256, THR, 0.99, SEED, L.F_DEVICE_IN,
                                               R.ctypes.data, t.ctypes.data, mask.ctypes.data, C.byref(st), None))
    return code, R, t, mask.tobytes(), int(mask.sum()), st.best_hyp


def test_other_entry_points_invalidate(ctx):
    o = _oracle(3000, 0.5, 7, 0, 2048)
    other = synth.pnp_problem(500, 0.3, seed=3)
    p2, p3 = _dev(o)
    assert _call(ctx, p2, p3, o, 0, 2048)[:2] == (0, 0)
    assert _call(ctx, p2, p3, o, 0, 2048)[:2] == (1, 1)
    with ctx.lock:  # a hypothesis probe on other points through the same context
        cnt = np.zeros(64, np.int32)
        st = np.zeros(64, np.int8)
        q3 = np.ascontiguousarray(other["points3d"])
        q2 = np.ascontiguousarray(other["points2d"])
        K9 = np.ascontiguousarray(other["K"], np.float64).reshape(9)
        L.check(L.lib().rsac_pnp_hypotheses(ctx.handle, q3.ctypes.data, q2.ctypes.data, 500, K9.ctypes.data, 0, 64, THR,
                                            SEED, 0, None, cnt.ctypes.data, st.ctypes.data, None, None))
    # ... whose own result is the oracle's: the reused calls before it left nothing behind
    oc, os_ = O.pnp_hypotheses(O.soa_pnp(other["points3d"], other["points2d"]), O.cam_from_K(other["K"]), THR, SEED, 64,
                               hyp0=0)[:2]
    np.testing.assert_array_equal(st > 0, os_ > 0)
    np.testing.assert_array_equal(np.where(st > 0, cnt, 0), np.where(os_ > 0, oc, 0))
    assert _call(ctx, p2, p3, o, 0, 2048)[:2] == (0, 0)
    assert _call(ctx, p2, p3, o, 0, 2048)[:2] == (1, 1)
    # a whole RANSAC on the same device points through the same context: what a fresh context gives
    fresh = L.Context(0)
    try:
        want = _ransac(fresh, p2, p3, o)
    finally:
        fresh.close()
    got = _ransac(ctx, p2, p3, o)
    assert got[0] == want[0] == L.OK and got[3:] == want[3:] and got[4] > 1000
    assert _bits_equal(got[1], want[1]) and _bits_equal(got[2], want[2])
    assert _call(ctx, p2, p3, o, 0, 2048)[:2] == (0, 0)
    # the winner's re-derivation between ranges (the multi-GPU step) leaves the record alone
    key_t = torch.tensor([o["key"]], dtype=torch.int64, device=p3.device)
    model_t, mask_t = rsac.winner(p2, p3, o["pr"]["K"], key_t, THR, context=ctx)
    assert _bits_equal(model_t.cpu().numpy(), o["model"])
    np.testing.assert_array_equal(mask_t.cpu().numpy(), o["mask"])
    assert _call(ctx, p2, p3, o, 0, 2048)[:2] == (1, 1)


def _raw(ctx, p2, p3, o, thr, flags):
    key = C.c_int64(-1)
    model = np.zeros(12)
    mask = torch.empty(p3.shape[0], dtype=torch.uint8, device=p3.device)
    K9 = np.ascontiguousarray(o["pr"]["K"], np.float64).reshape(9)
    with ctx.lock:
        L.check(L.lib().rsac_pnp_evaluate_range(ctx.handle, C.c_void_p(p3.data_ptr()), C.c_void_p(p2.data_ptr()),
                                                p3.shape[0], K9.ctypes.data, 0, 2048, thr, SEED,
                                                L.F_DEVICE_IN | L.F_DEVICE_OUT | flags, C.byref(key),
                                                model.ctypes.data, C.c_void_p(mask.data_ptr()), None, None))
    return int(key.value), model, mask.cpu().numpy(), (ctx.debug_get(L.DBG_SETUP_REUSED),
                                                       ctx.debug_get(L.DBG_BOUND_HINTED))


def test_raw_flag(ctx):
    o = _oracle(3000, 0.5, 7, 0, 2048)
    p2, p3 = _dev(o)
    torch.cuda.synchronize()  # the raw calls run on the context's own stream
    # (the hint needs no promise about the points' values: hinted from the second call on)
    for flags, want in ((0, (0, 0)), (0, (0, 1)), (L.F_POINTS_UNCHANGED, (1, 1)), (L.F_POINTS_UNCHANGED, (1, 1))):
        key, model, mask, reused = _raw(ctx, p2, p3, o, THR, flags)
        assert reused == want
        assert key == o["key"] and _bits_equal(model, o["model"])
        np.testing.assert_array_equal(mask, o["mask"])
    # the flag with another threshold: ignored, and the result is that threshold's
    key, model, mask, reused = _raw(ctx, p2, p3, o, 12.0, L.F_POINTS_UNCHANGED)
    assert reused == (0, 0)
    pr = o["pr"]
    soa, cam = O.soa_pnp(pr["points3d"], pr["points2d"]), O.cam_from_K(pr["K"])
    oc, os_, om = O.pnp_hypotheses(soa, cam, 12.0, SEED, 2048, hyp0=0, models=True)
    okey = par.best_key_of(oc, os_, 0)
    _, obest = par.unpack_key(okey)
    _, omask = O.pnp_count(om[obest, :9].reshape(3, 3), om[obest, 9:12], soa, cam, 12.0, mask=True)
    assert key == okey and _bits_equal(model, om[obest, :12])
    np.testing.assert_array_equal(mask, omask)
    # ... and back: the record now describes the call at 12 px
    assert _raw(ctx, p2, p3, o, THR, L.F_POINTS_UNCHANGED)[3] == (0, 0)
    assert _raw(ctx, p2, p3, o, THR, L.F_POINTS_UNCHANGED)[3] == (1, 1)


def test_two_contexts_two_streams_alternating():
    # the benchmark's pattern: nothing waits until the end
    o = _oracle(3000, 0.5, 7, 0, 2048)
    p2, p3 = _dev(o)
    ctxs = [L.Context(0), L.Context(0)]
    streams = [torch.cuda.current_stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    out = []
    try:
        for c in ctxs:
            c.debug_set(L.DBG_BOUND, 1)
        for i in range(6):
            with torch.cuda.stream(streams[i % 2]):
                out.append(rsac.evaluate_range(p2, p3, o["pr"]["K"], 0, 2048, THR, with_mask=True, device_result=True,
                                               context=ctxs[i % 2]))
        torch.cuda.synchronize()
        assert [c.debug_get(L.DBG_SETUP_REUSED) for c in ctxs] == [1, 1]
        assert [c.debug_get(L.DBG_BOUND_HINTED) for c in ctxs] == [1, 1]
        for key_t, model_t, mask_t in out:
            assert int(key_t.item()) == o["key"]
            assert _bits_equal(model_t.cpu().numpy(), o["model"])
            np.testing.assert_array_equal(mask_t.cpu().numpy(), o["mask"])
    finally:
        for c in ctxs:
            c.close()


def test_reused_call_without_a_model(ctx):
    # no hypothesis of the range has a model (key 0), twice: the key the solve reset stays 0
    # (n 1000, outliers 1.0, seed 10 has models in every range; 1000 copies of its first point have none)
    n = 1000
    pr = dict(synth.pnp_problem(n, 1.0, seed=10))
    pr["points3d"] = np.repeat(pr["points3d"][:1], n, 0)
    pr["points2d"] = np.repeat(pr["points2d"][:1], n, 0)
    oc, os_ = O.pnp_hypotheses(O.soa_pnp(pr["points3d"], pr["points2d"]), O.cam_from_K(pr["K"]), THR, SEED, 2048,
                               hyp0=0)[:2]
    assert par.best_key_of(oc, os_, 0) == 0
    o = dict(pr=pr, key=0, mask=np.zeros(n, np.uint8))
    p2, p3 = _dev(o)
    for want in (0, 1):
        assert _call(ctx, p2, p3, o, 0, 2048) == (want, want, n, 0)


def test_one_tile_range_twice(ctx):
    # 32 hypotheses: below the bounded sequence's size and a small round (the 4-lane solve, the
    # scaled-form scorer), so the reused call's solve is the one that resets the key
    o = _oracle(3000, 0.5, 7, 0, 32)
    p2, p3 = _dev(o)
    assert _call(ctx, p2, p3, o, 0, 32) == (0, 0, 3000, 0)
    assert _call(ctx, p2, p3, o, 0, 32) == (1, 0, 3000, 0)
    # ... and between two bounded calls: the unbounded one leaves no hint behind
    ob = _oracle(3000, 0.5, 7, 0, 2048)
    assert _call(ctx, p2, p3, ob, 0, 2048)[:2] == (1, 0)
    assert _call(ctx, p2, p3, ob, 0, 2048)[:2] == (1, 1)
    assert _call(ctx, p2, p3, o, 0, 32)[:2] == (1, 0)
    assert _call(ctx, p2, p3, ob, 0, 2048)[:2] == (1, 0)


@pytest.mark.parametrize("H", [2048, 32])
def test_without_mask_twice(ctx, H):
    o = _oracle(3000, 0.5, 7, 0, H)
    p2, p3 = _dev(o)
    for want in (0, 1):
        key, model = rsac.evaluate_range(p2, p3, o["pr"]["K"], 0, H, THR, context=ctx)
        assert ctx.debug_get(L.DBG_SETUP_REUSED) == want
        assert key == o["key"] and _bits_equal(model, o["model"])
    # asynchronous, no mask: key and model on the device
    key_t, model_t = rsac.evaluate_range(p2, p3, o["pr"]["K"], 0, H, THR, device_result=True, context=ctx)
    torch.cuda.synchronize()
    assert ctx.debug_get(L.DBG_SETUP_REUSED) == 1
    assert int(key_t.item()) == o["key"] and _bits_equal(model_t.cpu().numpy(), o["model"])


def test_inference_mode_tensors_are_accepted_and_never_reused(ctx):
    # tensors made under torch.inference_mode() track no version: no reuse, no reference kept
    o = _oracle(3000, 0.5, 7, 0, 2048)
    with torch.inference_mode():
        p2, p3 = _dev(o)
        assert p3.is_inference()
        for _ in range(2):
            assert _call(ctx, p2, p3, o, 0, 2048)[0] == 0
            assert ctx.last_in is None
        assert _call(ctx, p2, p3, o, 0, 2048, reuse_setup=False)[0] == 0
    # a copy the wrapper has to make (float32 input) is not remembered either
    q2, q3 = _dev(o)
    f3 = q3.to(torch.float32)
    rsac.evaluate_range(q2, f3, o["pr"]["K"], 0, 2048, THR, context=ctx)
    assert ctx.last_in is None and ctx.debug_get(L.DBG_SETUP_REUSED) == 0
    # ... and ordinary tensors are, until a call that cannot be reused
    assert _call(ctx, q2, q3, o, 0, 2048)[0] == 0
    assert ctx.last_in is not None and ctx.last_in[0] is q3
    assert _call(ctx, q2, q3, o, 0, 2048)[0] == 1
    assert _call(ctx, q2, q3, o, 0, 2048, reuse_setup=False)[0] == 0
    assert ctx.last_in is None


def test_hint_from_an_in_range_problem_on_an_out_of_range_one(ctx):
    # the hint's validity ignores the points' values, the f16 operand range does not: a pruning call,
    # then the x1e3 problem copied into the same tensors (form-1 records, no pass 2).  The hinted call
    # must be one whole pass whatever the hint says; its winner lies outside the first 256
    # hypotheses, so a pass 1 cut at the hint would leave it a partial count.
    n, hb, H = 2000, 703, 2048
    oa, ob = _oracle(n, 0.8, 12, hb, H), _oracle(n, 0.8, 12, hb, H, scale=1e3)
    assert ob["best"] - hb >= H0
    p2, p3 = _dev(oa)
    b3 = _dev(ob)[1]
    a3 = p3.clone()
    r, h, n1a, _ = _call(ctx, p2, p3, oa, hb, H)
    assert (r, h) == (0, 0) and n1a < n
    p3.copy_(b3)
    assert _call(ctx, p2, p3, ob, hb, H) == (0, 1, n, 0)
    assert _call(ctx, p2, p3, ob, hb, H) == (1, 1, n, 0)
    # the reverse: back in range under the hint N, then pruning again
    p3.copy_(a3)
    assert _call(ctx, p2, p3, oa, hb, H) == (0, 1, n, 0)
    r, h, n1, S = _call(ctx, p2, p3, oa, hb, H)
    assert (r, h, n1) == (1, 1, n1a) and S < H - H0
    # in place (mul_), as a caller rescaling its units would
    p3.mul_(1e3)
    assert torch.equal(p3, b3)  # (one IEEE product per element, on the device as in numpy: the same problem)
    assert _call(ctx, p2, p3, ob, hb, H) == (0, 1, n, 0)
