"""The batched fundamental-matrix calls without a GPU (DESIGN.md "Batched fundamental matrix"): the
header declares the four entry points, the library exports them with the ctypes table's
signatures, and the Python wrappers turn bad arguments away before any device work."""
import os
import re

import numpy as np
import pytest

import rsac
from rsac import _lib as L
from rsac import synth

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rsac.h")
ENTRY_POINTS = {
    # name -> number of arguments
    "rsac_fundamental_ransac_batched": 15,
    "rsac_fundamental_lmeds_batched": 15,
    "rsac_fundamental_fit_batched_device": 10,
    "rsac_fundamental_local_opt_batched": 14,
}


def _declarations():
    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"RSAC_EXPORT\s+int\s+(rsac_\w+)\s*\(([^;]*?)\)\s*;", txt, re.S)}


def test_header_declares_the_batched_entry_points():
    decl = _declarations()
    for name, nargs in ENTRY_POINTS.items():
        assert name in decl, name
        args = [a.strip() for a in decl[name].split(",")]
        assert len(args) == nargs, (name, args)
        assert args[0] == "rsac_ctx *ctx" and args[3] == "const int64_t *offsets" and args[4] == "int32_t n_problems"
        assert args[-1] == "void *stream"


def test_library_exports_them_and_the_table_matches():
    lib = L.lib()
    table = {n: (res, args) for n, res, args in L.SIGNATURES}
    for name, nargs in ENTRY_POINTS.items():
        assert hasattr(lib, name), name
        res, args = table[name]
        assert res is L.C.c_int and len(args) == nargs, name
        assert args[4] is L.C.c_int32  # n_problems


def _pairs(sizes):
    prs = [synth.fundamental_problem(n, 0.3, seed=40 + i) for i, n in enumerate(sizes)]
    return [p["pts1"] for p in prs], [p["pts2"] for p in prs]


def test_wrappers_reject_bad_arguments_without_a_device():
    a, b = _pairs([20, 30])
    F = np.eye(3)
    with pytest.raises(ValueError, match="differ in length"):
        rsac.fundamental_ransac_batched(a, b[:1])
    with pytest.raises(ValueError, match="counts differ"):
        rsac.fundamental_ransac_batched(a, [b[0], b[1][:29]])
    with pytest.raises(ValueError, match=">= 8"):
        rsac.fundamental_ransac_batched([a[0], a[1][:7]], [b[0], b[1][:7]])
    with pytest.raises(ValueError, match="score"):
        rsac.fundamental_ransac_batched(a, b, score="lmeds")
    with pytest.raises(ValueError, match="refine"):
        rsac.fundamental_ransac_batched(a, b, refine="lm")
    with pytest.raises(ValueError, match="differ in length"):
        rsac.fundamental_lmeds_batched(a, b[:1])
    with pytest.raises(ValueError, match="counts differ"):
        rsac.fundamental_lmeds_batched(a, [b[0], b[1][:29]])
    with pytest.raises(ValueError, match=">= 9"):
        rsac.fundamental_lmeds_batched([a[0], a[1][:8]], [b[0], b[1][:8]])
    with pytest.raises(ValueError, match="n_iters"):
        rsac.fundamental_lmeds_batched(a, b, n_iters=0)
    with pytest.raises(ValueError, match="refine"):
        rsac.fundamental_lmeds_batched(a, b, refine="lm")
    with pytest.raises(ValueError, match="differ in length"):
        rsac.fundamental_fit_batched(a, b[:1])
    with pytest.raises(ValueError, match="counts differ"):
        rsac.fundamental_fit_batched(a, [b[0], b[1][:29]])
    with pytest.raises(ValueError, match="mask_list"):
        rsac.fundamental_fit_batched(a, b, [np.ones(20, bool)])
    with pytest.raises(ValueError, match="mask and points"):
        rsac.fundamental_fit_batched(a, b, [np.ones(20, bool), np.ones(29, bool)])
    with pytest.raises(ValueError, match="F_list"):
        rsac.fundamental_local_opt_batched(a, b, [F])
    with pytest.raises(ValueError, match="9 elements"):
        rsac.fundamental_local_opt_batched(a, b, [F, np.zeros(8)])
    with pytest.raises(ValueError, match="max_rounds"):
        rsac.fundamental_local_opt_batched(a, b, [F, F], max_rounds=0)
    with pytest.raises(ValueError, match="reproj_thresh"):
        rsac.fundamental_local_opt_batched(a, b, [F, F], reproj_thresh=0.0)
    with pytest.raises(ValueError, match="differ in length"):
        rsac.fundamental_local_opt_batched(a, b[:1], [F, F])


def test_empty_batches_return_empty_lists():
    assert rsac.fundamental_ransac_batched([], []) == []
    assert rsac.fundamental_lmeds_batched([], []) == []
    assert rsac.fundamental_fit_batched([], []) == []
    assert rsac.fundamental_local_opt_batched([], [], []) == []
