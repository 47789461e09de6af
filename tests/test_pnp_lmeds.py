"""LMedS PnP without a GPU (DESIGN.md "LMedS PnP"): the host median (rsac_pnp_median_host, the source
the kernels run) against the NumPy restatement of tests/pnplmedsref.py bit for bit, the iteration
rule for 4 and 5 model points, the ABI table, the Python argument checks, and the restatement's own
TABLE."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lmedsref as LM  # noqa: E402
import msacref as MS  # noqa: E402
import pnplmedsref as M  # noqa: E402
import pyoracle as O  # noqa: E402
import rsac  # noqa: E402
from rsac import _lib as L  # noqa: E402

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rsac.h")


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


@pytest.mark.parametrize("row", range(len(M.TABLE)))
def test_restatement_reproduces_the_table(row):
    key, (best, median, ones) = M.TABLE[row]
    r = M.lmeds_case(*key, refine=False)
    assert (r["best"], r["median"], r["n_inliers"], r["iters"]) == (best, median, ones, 48)
    assert (r["status"] > 0).any() and int(r["mask"].sum()) == ones


@pytest.mark.parametrize("row", range(len(M.TABLE_REF)))
def test_restatement_reproduces_the_reference_mode_table(row):
    key, (best, median, ones) = M.TABLE_REF[row]
    r = M.lmeds_case(*key, refine=False, reference_mode=True)
    assert (r["best"], r["median"], r["n_inliers"], r["iters"]) == (best, median, ones, 89)


def test_the_bound_recovers_the_true_inliers():
    for key, (_, _, ones) in M.TABLE:
        inl = M.problem(*key)["inlier"]
        mask = M.lmeds_case(*key, refine=False)["mask"]
        assert not (mask & ~inl).any()
        assert int(inl.sum()) - ones == (1 if key == (513, .3, 6) else 0)


def test_no_model_case_has_fewer_than_four_ones():
    r = M.lmeds_case(*M.NO_MODEL, refine=False)
    st, med = r["status"], r["medians"]
    best, bm, _ = LM.scan(st, med, len(st))
    assert r["best"] == -1 and best >= 0 and bm == 0.0 and not r["mask"].any()
    pr = M.problem(*M.NO_MODEL)
    soa, cam = O.soa_pnp(pr["points3d"], pr["points2d"]), O.cam_from_K(pr["K"])
    _, _, models, _, _ = M.hypotheses_case(*M.NO_MODEL, 48)
    e = MS.errors(models[best, :9], models[best, 9:12], soa, cam)
    assert int((e <= M.thr2(bm, 5)).sum()) == 3


@pytest.mark.parametrize("row", range(len(M.TABLE)))
def test_host_median_equals_restatement_on_the_winners(row):
    key, (best, median, _) = M.TABLE[row]
    pr = M.problem(*key)
    st, med, models, _, _ = M.hypotheses_case(*key, 48)
    assert rsac.pnp_median(pr["points2d"], pr["points3d"], pr["K"], models[best, :12]) == median == med[best]
    for h in (0, 1, 47):  # and on a few losers
        if st[h] > 0:
            assert rsac.pnp_median(pr["points2d"], pr["points3d"], pr["K"], models[h, :12]) == med[h]


def _check(p3, p2, K, model12):
    soa, cam = O.soa_pnp(p3, p2), O.cam_from_K(K)
    with np.errstate(all="ignore"):
        ref = M.median_of_pose(np.asarray(model12, np.float64), soa, cam)
    got = rsac.pnp_median(p2, p3, K, model12)
    assert _same(got, ref), (got, ref)
    return got


@pytest.mark.parametrize("n", [1, 2, 3, 12, 13, 64, 65, 1000, 1001])
def test_host_median_odd_even_and_poses_behind_the_camera(n):
    pr = M.problem(max(n, 8), 0.3, 40 + n)
    p3, p2, K = pr["points3d"][:n], pr["points2d"][:n], pr["K"]
    m = np.r_[pr["R"].reshape(9), pr["t"]]
    _check(p3, p2, K, m)
    # the camera turned round (z < 0 for every point), and moved into the cloud (z of both signs)
    flip = np.diag([1.0, -1.0, -1.0])
    _check(p3, p2, K, np.r_[(flip @ pr["R"]).reshape(9), flip @ pr["t"]])
    t_in = pr["t"] - np.array([0.0, 0.0, float(np.median((p3 @ pr["R"].T + pr["t"])[:, 2]))])
    got = _check(p3, p2, K, np.r_[pr["R"].reshape(9), t_in])
    assert got >= 0.0


def test_host_median_z_zero_nan_and_inf():
    pr = M.problem(9, 0.0, 3)
    p3, p2, K = np.array(pr["points3d"]), np.array(pr["points2d"]), pr["K"]
    m = np.r_[pr["R"].reshape(9), pr["t"]]
    # z == 0 exactly for every point: the projection takes 1 / z as 1
    ident = np.r_[np.eye(3).reshape(9), np.zeros(3)]
    flat = p3.copy()
    flat[:, 2] = 0.0
    _check(flat, p2, K, ident)
    # fewer than half NaN: they rank above every finite error and the median stays finite
    bad = p3.copy()
    bad[:4, 0] = np.nan
    assert np.isfinite(_check(bad, p2, K, m))
    # more than half: the median is a NaN; with infinite pixels an infinity
    bad[:5, 0] = np.nan
    assert np.isnan(_check(bad, p2, K, m))
    far = p2.copy()
    far[:5, 1] = np.inf
    assert np.isinf(_check(p3, far, K, m))


def test_iteration_count_rule_for_four_and_five_model_points():
    assert (rsac.lmeds_num_iters(0.99, 2000, 4), rsac.lmeds_num_iters(0.99, 2000, 5)) == (48, 89)
    for k in (4, 5):
        for conf in (0.5, 0.9, 0.99, 0.995, 0.999999):
            for mx in (1, 2, 10, 50, 2000, 100000):
                assert rsac.lmeds_num_iters(conf, mx, k) == M.num_iters(conf, mx, k)


def test_sigma_with_five_model_points():
    for med, n in [(0.0, 6), (1e-9, 50), (3.5, 6), (3.5, 333), (1e6, 12)]:
        assert rsac.lmeds_sigma(med, n, 5) == M.sigma(med, n, 5)
        assert rsac.lmeds_sigma(med, n, 4) == M.sigma(med, n, 4) == LM.sigma(med, n)


def test_signatures_exist_and_match_the_header():
    txt = open(HDR).read()
    sig = {n: (r, a) for n, r, a in L.SIGNATURES}
    for name, nargs in [("rsac_pnp_lmeds", 15), ("rsac_pnp_lmeds_batched", 17), ("rsac_pnp_medians", 14),
                        ("rsac_pnp_median_host", 6)]:
        assert name in sig and hasattr(L.lib(), name)
        decl = re.search(r"RSAC_EXPORT int " + name + r"\(([^;]*)\);", txt).group(1)
        assert len(decl.split(",")) == nargs == len(sig[name][1]), name
    assert L.ABI_VERSION == 2 and L.lib().rsac_abi_version() == 2


def test_python_argument_checks_fire_without_a_device():
    pr = M.problem(12, .25, 5)
    a = (pr["points2d"], pr["points3d"], pr["K"])
    for kw in (dict(confidence=0.0), dict(confidence=1.0), dict(n_iters=0), dict(max_iters=0), dict(refine="lo"),
               dict(sampler="mwc"), dict(minimal="dlt")):
        with pytest.raises(ValueError):
            rsac.pnp_lmeds(*a, **kw)
        with pytest.raises(ValueError):
            rsac.pnp_lmeds_batched([a[0]], [a[1]], [a[2]], **kw)
    with pytest.raises(TypeError):
        rsac.pnp_lmeds(*a, dist=np.zeros(5))
    with pytest.raises(ValueError, match="differ in length"):
        rsac.pnp_lmeds(a[0][:11], a[1], a[2])
    with pytest.raises(ValueError, match="counts differ"):
        rsac.pnp_lmeds_batched([a[0][:11]], [a[1]], [a[2]])
    with pytest.raises(ValueError, match="one K per problem"):
        rsac.pnp_lmeds_batched([a[0]], [a[1]], [a[2], a[2]])
    with pytest.raises(ValueError, match=">= 4"):
        rsac.pnp_lmeds_batched([a[0][:3]], [a[1][:3]], [a[2]])
    with pytest.raises(ValueError):
        rsac.pnp_medians(*a, n_hyps=0)
    with pytest.raises(ValueError):
        rsac.pnp_medians(*a, n_hyps=8, minimal="dlt")
    with pytest.raises(ValueError):
        rsac.pnp_median(a[0][:11], a[1], a[2], np.zeros(12))
    with pytest.raises(rsac.RsacError):
        rsac.pnp_median(a[0][:0], a[1][:0], a[2], np.zeros(12))  # n >= 1
