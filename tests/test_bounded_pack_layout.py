"""The index maps of the bounded sequence's packed slab operands and of pass 2's shares (DESIGN.md
§16.3), through rsac_bound_layout: the functions of rsac_math.h that the kernels run.  No device.
"""
import pytest

from rsac import _lib as L


def test_packed_operand_rows_are_a_bijection():
    # the 2 x 32 operand rows hold each (hypothesis, component) of the 32 hypotheses x {xs, z'} once
    rows = {}
    for t in range(2):
        for row in range(32):
            hyp, comp = L.bound_layout(0, t, row, 0, 0, 0)[:2]
            assert 0 <= hyp < 32 and comp in (0, 1)
            assert (hyp, comp) not in rows
            rows[(hyp, comp)] = (t, row)
    assert len(rows) == 64


def test_accumulators_follow_the_rows():
    # accumulator i of the lanes of a half is result row 8 (i >> 2) + 4 half + (i & 3) of a 32x32 MFMA;
    # a lane-half's pair (2k, 2k + 1) is (xs, z') of one hypothesis, found again through its slot
    seen = {}
    for t in range(2):
        for half in range(2):
            for i in range(16):
                row = 8 * (i >> 2) + 4 * half + (i & 3)
                rh, rc = L.bound_layout(0, t, row, 0, 0, 0)[:2]
                ah, ac = L.bound_layout(0, t, 0, half, i, 0)[2:4]
                assert (ah, ac) == (rh, rc)
                assert ac == (i & 1)
                if i & 1:
                    assert ah == seen[(t, half, i - 1)]
                seen[(t, half, i)] = ah
                slot, hf = L.bound_layout(0, 0, 0, 0, 0, ah)[4:6]
                assert hf == half and slot == 8 * t + (i >> 1)
    slots = {tuple(L.bound_layout(0, 0, 0, 0, 0, j)[4:6]) for j in range(32)}
    assert slots == {(s, h) for s in range(16) for h in range(2)}


def _cover(tiles, pts, grid, fill, min_len, max_seg=64):
    """run the kernel's segment loop over every share -> per tile the list of (first, length)"""
    passes, length, n = L.bound_layout(1, tiles, pts, grid, fill, min_len)[:3]
    assert passes == (pts + 255) // 256
    line = tiles * passes
    if line == 0:
        assert n == 0
        return passes, length, n, {}
    assert length >= min_len and (n - 1) * length < line <= n * length
    if length > min_len:  # as near to fill x grid equal shares as whole block passes allow
        assert n <= fill * grid and (length - 1) * fill * grid < line
    segs = {}
    for u in range(n):
        pos, end = u * length, min(line, (u + 1) * length)
        while pos < end:
            tile, first, seg = L.bound_layout(2, tiles, pts, grid, fill, min_len, u, pos)[:3]
            assert tile == pos // passes and first == pos % passes
            assert 1 <= seg <= max_seg and first + seg <= passes and pos + seg <= end
            segs.setdefault(tile, []).append((first, seg))
            pos += seg
    return passes, length, n, segs


# tiles, points, grid, shares per block, shortest share: S = 0; S in 1..31; a line shorter than the
# grid; most shares over two tiles; the workload (408 tiles x 10 000 points on 768 blocks) at 1, 2
# and 4 shares per block; 20 000 points (79 block passes a tile; with 700 tiles a share is longer
# than the window of 64 and its segments end there, with 12 the GPU test's short shares); the slab
# off (pass 2 over the 688 points past n1); more tiles than shares (a share over many tiles)
@pytest.mark.parametrize("tiles,pts,grid,fill,min_len", [
    (0, 1500, 384, 1, 4), (1, 1500, 384, 1, 4), (3, 1500, 384, 1, 4), (60, 1200, 320, 1, 4),
    (408, 10000, 768, 1, 4), (408, 10000, 768, 2, 4), (408, 10000, 768, 4, 4), (408, 10000, 768, 1, 2),
    (408, 10000, 768, 1, 8), (700, 20000, 768, 1, 4), (12, 20000, 768, 1, 4), (60, 688, 320, 1, 4),
    (3125, 10000, 768, 1, 4), (3125, 300, 8, 1, 4), (5, 0, 768, 1, 4)])
def test_shares_cover_the_line_once(tiles, pts, grid, fill, min_len):
    passes, length, n, segs = _cover(tiles, pts, grid, fill, min_len)
    assert sorted(segs) == list(range(tiles if passes else 0))
    for tile, ss in segs.items():
        ss.sort()
        at = 0
        for first, seg in ss:  # no gap, no double cover
            assert first == at
            at += seg
        assert at == passes
    if (tiles, pts) == (60, 1200):
        straddle = sum(1 for u in range(n) if (u * length) // passes != (min(tiles * passes, (u + 1) * length) - 1) // passes)
        assert 2 * straddle > n
    if (tiles, pts) == (700, 20000):  # shares of 73 block passes: cut at the window
        assert passes == 79 and length > 64 and any(seg == 64 for ss in segs.values() for _, seg in ss)


def test_layout_rejects_bad_arguments():
    with pytest.raises(L.RsacError):
        L.bound_layout(0, 2, 0, 0, 0, 0)
    with pytest.raises(L.RsacError):
        L.bound_layout(2, 4, 1500, 384, 1, 4, 0, 99)
    with pytest.raises(L.RsacError):
        L.bound_layout(9)
