"""The packed slab operands, pass 2's even shares and the slab guard of the bounded sequence
 against the CPU oracle.

Shapes, forcing and the comparison follow tests/test_bounded_slab_gpu.py (RSAC_DBG_BOUND = 1, thr 30,
seed 0x5EED, the oracle through pyoracle; its helpers and its cache of oracle records are used
here): every call's key, model bits and mask must equal the oracle's.  On top of that the count word
of every hypothesis is read back (RSAC_DBG_BOUND_COUNT) and held against the oracle's counts:

  * a hypothesis of the first 256, and every listed one, ends with its exact count over all points:
    a permutation of counts inside a tile, or a gap or a double cover of pass 2's shares, breaks it;
  * a hypothesis that is not listed keeps pass 1's figure: its exact count over [0, n1) where pass 1
    ran the exact body, and where it ran the slab a figure of at least that count and below the bar
    B0 - (N - n1) (a figure at the bar or above would have been listed).

Which hypotheses were listed is not read back; it follows from the counts: with c1 the exact count
over [0, n1), a hypothesis with c1 at the bar or above must be listed under either body.

The slab's partial iteration: whenever the slab runs, n1 is a multiple of 256 (bound_n1_of), one
block pass, so the slab body itself never ends inside an iteration through the API; the exact units
beside it (the first 256 hypotheses' tiles, pass 2) end at N, and N = 1501 covers those.

S against the unpacked body: tests/golden/bounded_pack_survivors.json holds (n1, S, key) of CASES
from a -DRSAC_BOUND_SLAB_PACK=0 build of the same tree (scripts/bound_pack_golden.py writes it).
"""
import json
import os

import numpy as np
import pytest

import pyoracle as O
from rsac import _lib as L

from test_bounded_slab_gpu import H0, THR, _b0_n1, _call, _dev, _oracle, _oracle_survivors

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bounded_pack_survivors.json")

# (n, outliers, seed, hyp_begin, H): 30 / 50 / 70 % outliers; 1200 points at 30 %: many survivors
# over 5 block passes, so that most shares of 4 straddle two tiles; 20 000 points: 79 block passes a
# tile, more than one recount window, every tile of both passes by cells (its shares stay short with
# so few survivors: test_segments_end_at_the_recount_window lengthens them);
# 1501: N no multiple of 64
CASES = {
    "o30": (2500, 0.3, 8, 0, 2048),
    "o50": (1500, 0.5, 7, 0, 2048),
    "o70": (1500, 0.7, 4, 0, 2048),
    "straddle": (1200, 0.3, 5, 0, 2048),
    "window": (20000, 0.5, 13, 0, 1024),
    "odd_n": (1501, 0.5, 7, 0, 2048),
}


def _head_counts(o):
    """exact counts over [0, n1) of every hypothesis of the range (0 without a model)"""
    if "c1" not in o:
        _, n1 = _b0_n1(o)
        head = tuple(np.ascontiguousarray(a[:n1]) for a in o["soa"])
        c1 = np.zeros(o["H"], np.int64)
        for j in range(o["H"]):
            if o["os"][j] > 0:
                c1[j] = O.pnp_count(o["om"][j, :9].reshape(3, 3), o["om"][j, 9:12], head, o["cam"], THR)
        c1.setflags(write=False)
        o["c1"] = c1
    return o["c1"]


def _counts(ctx, H):
    out = np.zeros(H, np.int64)
    for j in range(H):
        ctx.debug_set(L.DBG_BOUND_COUNT, j)
        out[j] = ctx.debug_get(L.DBG_BOUND_COUNT)
    return out


def _check_counts(ctx, o, n1, S, whole=False):
    """the module docstring's rules; n1 = the n1 the call ran with (its own plan's: not a stale hint's);
    whole: a problem outside the f16 operand range, one whole pass whatever B0 is"""
    n, H = len(o["mask"]), o["H"]
    B0, n1o = _b0_n1(o)
    assert n1 == (n if whole else n1o)
    ran = ctx.debug_get(L.DBG_BOUND_SLAB_RAN)
    full = np.where(o["os"] > 0, o["oc"], 0).astype(np.int64)
    got = _counts(ctx, H)
    np.testing.assert_array_equal(got[:H0], full[:H0])
    if n1 >= n:  # one whole pass
        assert ran == 0 and S == 0
        np.testing.assert_array_equal(got, full)
        return ran
    c1, bar = _head_counts(o), B0 - (n - n1)
    must = c1 >= bar
    must[:H0] = False
    print(f"ran={ran} bar={bar} must_list={int(must.sum())} S={S}")
    np.testing.assert_array_equal(got[must], full[must])
    rest = ~must
    rest[:H0] = False
    if ran:
        assert S >= int(must.sum())
        kept = (got >= c1) & (got < bar)
        bad = np.flatnonzero(rest & ~(kept | (got == full)))
    else:
        assert S == int(must.sum())
        bad = np.flatnonzero(rest & (got != c1))
    assert len(bad) == 0, (bad[:8], got[bad[:8]], c1[bad[:8]], full[bad[:8]])
    return ran


def _run(o, mode, counts=True, whole=False, p2_min=0):
    """a fresh context: one plain and one hinted call in slab mode `mode` (RSAC_DBG_BOUND_SLAB: 0 by
    the guard, 1 the exact body, 2 the slab whatever the guard says) -> (n1, S, ran)"""
    c = L.Context(0)
    try:
        c.debug_set(L.DBG_BOUND, 1)
        c.debug_set(L.DBG_BOUND_SLAB, mode)
        c.debug_set(L.DBG_BOUND_P2_MIN, p2_min)  # pass 2's shortest share in block passes (0: as built)
        p2, p3 = _dev(o)
        plain = _call(c, p2, p3, o)
        ran = _check_counts(c, o, plain[1], plain[2], whole) if counts else c.debug_get(L.DBG_BOUND_SLAB_RAN)
        hinted = _call(c, p2, p3, o)
        assert plain[0] == 0 and hinted[0] == 1 and plain[1:] == hinted[1:]
        assert c.debug_get(L.DBG_BOUND_SLAB_RAN) == ran
        if counts:
            _check_counts(c, o, hinted[1], hinted[2], whole)
    finally:
        c.close()
    return plain[1], plain[2], ran


def survivors_of(name):
    """(n1, S, key) of a call on CASES[name] with the slab forced (the golden file's entry)"""
    o = _oracle(*CASES[name])
    n1, S, _ = _run(o, 2, counts=False)
    return [int(n1), int(S), int(o["key"])]


def test_layout_as_built():
    fill, min_len, max_seg, packed = L.bound_layout(3)[:4]
    assert packed == 1 and fill >= 1 and min_len >= 1 and max_seg == 64


@pytest.mark.parametrize("name", sorted(CASES))
def test_counts_and_survivors(name):
    # the slab (packed operands; pass 2 over [0, N)) and the exact body (pass 2 over [n1, N), lo != 0):
    # per-hypothesis counts, and (n1, S, key) of the slab against the unpacked build's
    o = _oracle(*CASES[name])
    n = len(o["mask"])
    assert _b0_n1(o)[1] < n
    exact = _run(o, 1)
    slab = _run(o, 2)
    assert exact[2] == 0 and exact[1] == _oracle_survivors(o)
    assert slab[2] == 1 and slab[1] >= exact[1] and slab[0] == exact[0]
    # by the guard: its flag and S agree, whatever g is
    dflt = _run(o, 0, counts=False)
    assert dflt[:2] == (slab[:2] if dflt[2] else exact[:2])
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert gold["packed"] == 0  # (written by a build without the packed operands)
    assert [slab[0], slab[1], o["key"]] == gold[name]


# --- routing: the winner at every position of its tile; short last tiles ---

R70 = (1500, 0.7, 4)  # 70 % outliers: hypothesis 331 is the best of every range [hb, hb + 1024), hb < 32


def test_winner_at_every_tile_position():
    # 32 consecutive range starts move the one winner, past H0 in each, through the 32 positions of a
    # tile; plain and hinted, the slab running
    pos = set()
    for hb in range(32):
        o = _oracle(*R70, hb, 1024)
        assert _b0_n1(o)[1] < 1500 and o["best"] == 331
        n1, S, ran = _run(o, 2, counts=hb % 8 == 0)
        assert ran == 1
        pos.add((o["best"] - hb) % 32)
    assert len(pos) == 32 and 331 - 31 >= H0


@pytest.mark.parametrize("H", [1024 + 1, 1024 + 5, 1024 + 16, 1024 + 17, 1024 + 31])
def test_short_last_tile(H):
    # nh = 1, 5 (odd, group 1 all padding), 16 (group 1 all padding), 17, 31
    o = _oracle(*R70, 0, H)
    assert _run(o, 2)[2] == 1
    _run(o, 1)


# --- pass 2's shares ---

@pytest.mark.parametrize("hb,S", [(1568, 0), (1504, 1)])
def test_share_lines_empty_and_short(hb, S):
    # ranges of 544 hypotheses (17 tiles: the fewest the bounded sequence takes) of (2000, 0.8, 12)
    # whose exact list is empty / has one entry: no unit at all, and a line of one tile, far shorter
    # than the grid (shares of the minimum length)
    o = _oracle(2000, 0.8, 12, hb, 544)
    assert _oracle_survivors(o) == S
    exact = _run(o, 1)
    slab = _run(o, 2)
    print(f"hb={hb}: exact S={exact[1]}, slab S={slab[1]}")
    assert exact[1] == S and S <= slab[1] < 32 and slab[2] == 1


def test_segments_end_at_the_recount_window():
    # 20 000 points are 79 block passes a tile, more than one recount window (64).  With so few
    # survivors the shares as built are 4 block passes long, so RSAC_DBG_BOUND_P2_MIN makes them 100:
    # every share then runs over two tiles and its segments are cut at the window (the slab forced:
    # pass 2 over [0, N)); with the exact body pass 2 has 39 block passes a tile, a share runs over
    # three or four tiles.  Key, model, mask and every hypothesis's count against the oracle, plain
    # and hinted
    o = _oracle(*CASES["window"])
    n1, S, ran = _run(o, 2, p2_min=100)
    assert ran == 1 and S >= 64
    # the same line on the host (the grid only matters where it asks for longer shares than 100)
    tiles = (S + 31) // 32
    passes, length, n = L.bound_layout(1, tiles, 20000, 8, 0, 100)[:3]
    assert (passes, length) == (79, 100)
    segs, line = [], tiles * passes
    for u in range(n):
        pos, end = u * length, min(line, (u + 1) * length)
        while pos < end:
            seg = L.bound_layout(2, tiles, 20000, 8, 0, 100, u, pos)[2]
            segs.append(seg)
            pos += seg
    assert max(segs) == 64 and segs.count(64) >= 1
    assert _run(o, 1, p2_min=100)[:2] == (n1, _oracle_survivors(o))


# --- the guard ---

def _plain_flag(o):
    return _run(o, 0, counts=False)[2]


def test_decision_follows_the_points():
    # a 50 % problem, then a 70 % one in the same tensors, and back, hinted: the first call after a
    # change runs on the previous problem's decision (and n1) and must still equal the oracle; the
    # next one carries the new problem's.  6000 points: the two problems' decisions differ for the
    # guard as built (g = 16); should g change so that they agree, pick problems that differ again.
    a, b = _oracle(6000, 0.5, 21, 0, 1024), _oracle(6000, 0.7, 22, 0, 1024)
    fa, fb = _plain_flag(a), _plain_flag(b)
    assert fa != fb, "the two problems must differ in the slab decision for this test to see a stale one"
    c = L.Context(0)
    try:
        c.debug_set(L.DBG_BOUND, 1)
        p2, p3 = _dev(a)
        assert _call(c, p2, p3, a)[0] == 0 and c.debug_get(L.DBG_BOUND_SLAB_RAN) == fa
        for prev, cur, fprev, fcur in ((a, b, fa, fb), (b, a, fb, fa)):
            q2, q3 = _dev(cur)
            p2.copy_(q2)
            p3.copy_(q3)
            stale = _call(c, p2, p3, cur)
            assert stale[0] == 1 and stale[1] == _b0_n1(prev)[1]
            assert c.debug_get(L.DBG_BOUND_SLAB_RAN) == fprev
            fresh = _call(c, p2, p3, cur)
            assert fresh[0] == 1 and c.debug_get(L.DBG_BOUND_SLAB_RAN) == fcur
            _check_counts(c, cur, fresh[1], fresh[2])
    finally:
        c.close()


@pytest.mark.parametrize("other", ["fallback", "out_of_range"])
def test_no_slab_without_a_cut(other):
    # (2000, 0.9, 9): no hypothesis of the first 256 passes delta; (3000, 0.5, 7) x 1e3: outside the
    # f16 operand range.  One whole pass: the slab is reported unused, plain and hinted
    o = _oracle(2000, 0.9, 9, 0, 2048) if other == "fallback" else _oracle(3000, 0.5, 7, 0, 2048, 1e3)
    for mode in (0, 2):
        assert _run(o, mode, whole=other == "out_of_range") == (len(o["mask"]), 0, 0)
