"""The homography refit and its local optimisation, the parts that need no GPU: the new entry points
in the header and the ctypes table, the host fit against the oracle on the debug.log blocks, the
argument errors, and the local-optimisation loop restated on the oracle (tests/homfitref.py) -- its
invariants and the pinned table of DESIGN.md "Homography: least-squares and LM refit and local
optimisation on GPU"."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import homfitref as R  # noqa: E402
import pyoracle as O  # noqa: E402
import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rsac_homography_fit_device", "rsac_homography_fit_batched_device", "rsac_homography_local_opt")


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def test_exports():
    header = open(os.path.join(ROOT, "include", "rsac.h")).read()
    names = {row[0] for row in L.SIGNATURES}
    for name in NEW:
        assert re.search(r"RSAC_EXPORT int %s\(" % name, header), name
        assert name in names and hasattr(L.lib(), name)
    for name in ("homography_fit", "homography_fit_batched", "homography_local_opt"):
        assert name in rsac.__all__ and callable(getattr(rsac, name))
    assert re.search(r"#define RSAC_ABI_VERSION\s+2\b", header)
    assert L.lib().rsac_abi_version() == 2


def test_host_fit_equals_oracle_on_the_debuglog_blocks():
    blocks = R.debuglog_blocks()
    assert len(blocks) == 24
    for src, dst, mask in blocks:
        H = rsac.homography_fit(src, dst, mask)
        Ho = R.fit(O.soa_hom(src, dst), mask)
        assert H is not None and Ho is not None and _bits_equal(H, Ho)


def test_host_fit_equals_oracle_on_the_gpu_tests_inputs():
    """the inputs of tests/test_hom_fit_gpu.py through the host twin: what the device is held to"""
    for m in R.SIZES:
        for shape in ("ones", "third") + (("chunk",) if m >= 128 else ()):
            for noise in R.NOISES:
                src, dst, mask = R.case(m, shape, noise)
                H, Ho = rsac.homography_fit(src, dst, mask), R.fit(O.soa_hom(src, dst), mask)
                assert H is not None and Ho is not None and _bits_equal(H, Ho), (m, shape, noise)
    for args in (R.four_ones(130), R.four_ones(4097), R.translation()):
        H, Ho = rsac.homography_fit(*args), R.fit(O.soa_hom(args[0], args[1]), args[2])
        assert H is not None and _bits_equal(H, Ho)
    for args in (R.three_ones(130), R.equal_x(65, "src"), R.equal_x(65, "dst")):
        assert rsac.homography_fit(*args) is None and R.fit(O.soa_hom(args[0], args[1]), args[2]) is None


def test_bad_arguments_raise_before_any_device_work():
    pr = R.problem(40, 0.3, 11)
    src, dst = pr["src"], pr["dst"]
    for bad in ("lm", "LO", 1, None, 2.0):
        with pytest.raises(ValueError, match="refine"):
            rsac.homography_ransac(src, dst, refine=bad)
        with pytest.raises(ValueError, match="refine"):
            rsac.homography_lmeds(src, dst, refine=bad)
    with pytest.raises(ValueError):
        rsac.homography_fit(src, dst[:39], device=0)
    with pytest.raises(ValueError):
        rsac.homography_fit(src, dst, np.ones(39, bool), device=0)
    with pytest.raises(ValueError):
        rsac.homography_fit_batched([src, src], [dst])
    with pytest.raises(ValueError):
        rsac.homography_fit_batched([src], [dst], [np.ones(39, bool)])
    H = np.eye(3)
    for rounds in (0, -1):
        with pytest.raises(ValueError, match="max_rounds"):
            rsac.homography_local_opt(src, dst, H, max_rounds=rounds)
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="reproj_thresh"):
            rsac.homography_local_opt(src, dst, H, thr)
    with pytest.raises(ValueError):
        rsac.homography_local_opt(src, dst, np.eye(4))
    with pytest.raises(ValueError):
        rsac.homography_local_opt(src, dst[:39], H)


@pytest.mark.parametrize("key", R.INPUTS, ids=[str(k[0]) for k in R.INPUTS])
def test_loop_invariants(key):
    r = R.row(key)
    soa = R.soa_of(key)
    for cap in range(1, R.MAX_ROUNDS + 1):
        H, mask, count, steps = r["lo"][cap]
        assert steps <= cap and int(mask.sum()) == count
        # every accepted round raised the count strictly: replay the chain
        Hc, counts = r["H0"], [r["c0"]]
        mk = r["mask0"]
        for _ in range(steps):
            Hc = R.fit(soa, mk)
            c, mk = O.hom_count(Hc, soa, R.THR, mask=True)
            counts.append(c)
        assert all(b > a for a, b in zip(counts, counts[1:])) and counts[-1] == count
        assert _bits_equal(Hc, H) and np.array_equal(mk, mask)
        if steps < cap:  # stopped by the rule, not by the cap: one more fit does not raise the count
            Hn = R.fit(soa, mask)
            assert Hn is None or count < 4 or not O.hom_count(Hn, soa, R.THR) > count
    # the loop with the library's host fit in place of the oracle's: the same chain
    pr = R.problem(*key)
    host = lambda s, m: rsac.homography_fit(pr["src"], pr["dst"], m)  # noqa: E731
    for cap in (1, R.MAX_ROUNDS):
        H, mask, count, steps = R.local_opt(soa, r["H0"], R.THR, cap, host)
        rH, rmask, rcount, rsteps = r["lo"][cap]
        assert (count, steps) == (rcount, rsteps) and np.array_equal(mask, rmask) and _bits_equal(H, rH)


def test_zero_rounds_return_the_input_itself():
    soa = R.soa_of(R.INPUTS[0])
    H = np.array([[1.0, 0, 5000.0], [0, 1.0, 5000.0], [0, 0, 1.0]])  # no point of the problem is near it
    Ho, mask, count, steps = R.local_opt(soa, H, R.THR, 4)
    assert count < 4 and steps == 0 and Ho is not None and _bits_equal(Ho, H) and int(mask.sum()) == count
    # a model at its fixed point: the fit on its own mask does not raise the count
    r = R.row(R.INPUTS[2])
    Hf, _, cf, _ = r["lo"][R.MAX_ROUNDS]
    Ho, _, count, steps = R.local_opt(R.soa_of(R.INPUTS[2]), Hf, R.THR, 4)
    assert steps == 0 and count == cf and _bits_equal(Ho, Hf)


@pytest.mark.parametrize("key", R.INPUTS, ids=[str(k[0]) for k in R.INPUTS])
def test_pinned_table(key):
    want = R.TABLE[key]
    assert R.table_row(key) == want
    assert want[2] >= want[1] >= want[0] or want[3] == 0
    assert want[3] <= R.MAX_ROUNDS
