"""The DEM ray march (k_dem_march, rsac_geo.h, rsac/dem.py) at chunk, binade and grid edges.

Bar: status and hit equal the batched oracle (oracle/dem_oracle.py: ray_intersect_dem_many) bit for
bit on EVERY ray.  What makes that a fair demand is the margin rule of tests/demref.py: every scene
is fixed so that each decision of the oracle's march is more than 1e-6 m (height against elevation)
and 1e-12 deg (position against the grid's bounds) from flipping; the margins are asserted first,
on the CPU (test_case_margins), and again before each GPU comparison.

CPU part: the sanitizer program of the RSAC_HD pieces (tests/sanitize/geo_harness.cpp), the oracle's
no-data semantics, the margins and intended steps of every scene, and the accuracy of the oracle's
projection against a 40-digit evaluation of the same Krueger series (mpmath).  Measured there
(x86-64, numpy 2 / glibc), largest error over the 312 points of `_utm_points`:
    forward  2.900e-9 m    (1.6 ulp of a northing of 9e6 m)       -> ORACLE_FWD_ERR_M   = 2.91e-9
    inverse  3.215e-14 deg (2.3 ulp of a longitude of 120 deg)    -> ORACLE_INV_ERR_DEG = 3.22e-14
The GPU kernels are held to 8 x those figures (another libm, the device's transcendentals):
2.3e-8 m and 2.6e-13 deg, 43 x and 3900 x tighter than the 1e-6 m / 1e-9 deg of test_dem.py.

Infinite direction components are included: a position of +-inf makes the projection NaN in the
oracle (inf - inf in the series) and in utm_inverse_fast (inf / inf in dsinhcosh), a NaN point is
off the grid for scipy and for dem_interp alike, and an infinite height never enters the
interpolation, so no 0 * inf is evaluated on either side.  Infinite DEM values are left out:
scipy's and dem_interp's weights reach an exact 0 at different points.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import dem_oracle as D
import demref as R
from rsac import synth

HERE = os.path.dirname(os.path.abspath(__file__))
LATC, LONC = 26.0936, 119.3906

# measured by test_oracle_utm_accuracy_vs_mpmath (see the module docstring); the GPU bounds are 8 x
ORACLE_FWD_ERR_M = 2.91e-9
ORACLE_INV_ERR_DEG = 3.22e-14


# ------------------------------------------------------------------ CPU: the sanitizer program

def test_geo_harness(tmp_path):
    out = tmp_path / "geo"
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "sanitize"), "-f", "geo.mk", f"OUT={out}"], check=True,
                   timeout=600)
    r = subprocess.run([str(out / "geo_asan")], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    txt = r.stdout + r.stderr
    assert r.returncode == 0, txt[-3000:]
    for bad in ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer"):
        assert bad not in txt, txt[-3000:]
    assert "ok (0 failed checks)" in txt


# ------------------------------------------------------------------ scenes

def _case(g, origins, dirs, expect=None, **kw):
    origins = np.ascontiguousarray(np.asarray(origins, np.float64).reshape(-1, 3))
    dirs = np.ascontiguousarray(np.asarray(dirs, np.float64).reshape(-1, 3))
    if origins.shape[0] == 1:
        origins = np.repeat(origins, dirs.shape[0], axis=0)
    m = R.march(origins, dirs, g, **kw)
    return dict(g=g, origins=origins, dirs=dirs, kw=kw, m=m, expect=expect or {})


def _ground(g, e, n, zone=50, south=False):
    lon, lat = D.utm_to_wgs84(np.float64(e), np.float64(n), zone, south)
    return float(D.make_interpolator(g["z"], g["y0"], g["dy"], g["x0"], g["dx"])((lat, lon)))


def _layout_rays(g, latc, lonc, zone, south):
    """256 rays from 5 distinct origins (so o[3 * r] is read per ray), downward cones and a few
    level / rising rays; hits, exits and exhausted searches all occur."""
    rng = np.random.default_rng(20)
    e0, n0 = R.utm(lonc, latc, zone, south)
    off = np.array([[0.0, 0.0], [-310.5, 122.25], [240.125, -401.0], [95.0, 380.75], [-150.3, -270.9]])
    org = np.empty((5, 3))
    for k in range(5):
        e, n = e0 + off[k, 0], n0 + off[k, 1]
        org[k] = e, n, _ground(g, e, n, zone, south) + 140.0 + 35.0 * k
    which = np.arange(256) % 5
    az = rng.uniform(0, 2 * np.pi, 256)
    tilt = np.radians(np.where(np.arange(256) % 8 == 7, rng.uniform(-4, 2, 256), rng.uniform(6, 55, 256)))
    d = np.c_[np.sin(az) * np.cos(tilt), np.cos(az) * np.cos(tilt), -np.sin(tilt)]
    return org[which], d


LAYOUTS = {"north_up": {}, "south_up": dict(south_up=True), "east_first": dict(east_first=True)}


@functools.lru_cache(maxsize=None)
def case_layout(layout, where="kuliang"):
    latc, lonc, zone, south = {"kuliang": (LATC, LONC, 50, False), "zone40S": (-LATC, LONC - 60.0, 40, True),
                               "zone1N": (LATC, LONC - 294.0, 1, False)}[where]
    g = R.grid(latc, lonc, **LAYOUTS[layout])
    assert g["z"].shape == (37, 53)
    o, d = _layout_rays(R.grid(latc, lonc), latc, lonc, zone, south)  # the same rays for every layout
    return _case(g, o, d, max_search_dist=700, min_steps=150, zone=zone, south=south)


PIN_STEPS = [0, 1, 63, 64, 127, 128, 191, 192, 255, 256, 257, 511, 512, 1000]
PIN_CONFIGS = [(0, 1200, 1), (150, 1200, 1), (256, 1200, 1), (300, 1200, 1),           # min_steps
               (0, 0, 1), (0, 1, 1), (0, 255, 1), (0, 256, 1), (0, 257, 1), (0, 1000, 3),  # n_steps (333 = int(1000 / 3))
               (300, 255, 1), (300, 257, 1), (400, 1000, 3), (257, 257, 1)]          # min_steps >= n_steps


@functools.lru_cache(maxsize=None)
def case_pinned(min_steps, max_search_dist, step):
    """A flat DEM at 300 m and rays (0.3, 0.2, -0.75) -- every coordinate advances -- from heights
    300 + 0.75 (S - 0.5): at unit step the height crosses the surface half a step before step S
    (margin 0.375 m, all sums exact), so the first hit is due at S and lands at max(S, min_steps)."""
    g = R.grid(LATC, LONC, fn=lambda la, lo: 300.0)
    n_steps = int(max_search_dist / step)
    S = sorted(set(PIN_STEPS + [s for s in (n_steps - 1, n_steps, n_steps + 1) if s >= 0]))
    e0, n0 = R.utm(LONC, LATC)
    o = np.array([[e0, n0, 300.0 + 0.75 * (s - 0.5)] for s in S])
    d = np.repeat([[0.3, 0.2, -0.75]], len(S), axis=0)
    due = np.maximum(np.maximum(0, np.ceil((np.array(S) - 0.5) / step)).astype(int), min_steps)
    return _case(g, o, d, expect=dict(steps=np.minimum(due, n_steps), status=np.where(due < n_steps, 0, 1)),
                 max_search_dist=max_search_dist, step=step, min_steps=min_steps)


@functools.lru_cache(maxsize=None)
def case_order(layout):
    """Hit and grid exit inside one 256-step chunk, in either order; exits before min_steps; origins
    outside and (to 1e-9 deg, the exact node being unreachable through a UTM origin; the node
    itself is checked in geo_harness.cpp) on a corner node."""
    g = R.grid(LATC, LONC, fn=lambda la, lo: 300.0, **LAYOUTS[layout])
    ylo, yhi, xlo, xhi = R.bounds(g)
    ee, ne = R.utm(xhi, LATC)     # east edge at the centre's latitude
    ew, nw = R.utm(xlo, LATC)
    en, nn = R.utm(LONC, yhi)     # north edge at the centre's longitude
    ec, nc = R.utm(xlo + 1e-9, yhi - 1e-9)
    es, ns = R.utm(xhi - 1e-9, ylo + 1e-9)
    rays = [  # origin, direction, status, step
        ((ee - 229.5, ne, 300 + 0.5 * 199.5), (1, 0, -0.5), 0, 200),    # hits at 200, would leave at 230
        ((ee - 199.5, ne, 300 + 0.5 * 229.5), (1, 0, -0.5), 2, 200),    # leaves at 200, would hit at 230
        ((ee - 39.5, ne, 250.0), (1, 0, -0.5), 2, 40),                  # underground, gone before min_steps
        ((ee + 50.0, ne, 400.0), (0, 0, -1), 2, 0),                     # origin outside
        ((ew + 229.5, nw, 300 + 0.5 * 199.5), (-1, 0, -0.5), 0, 200),   # westward
        ((ew + 199.5, nw, 300 + 0.5 * 229.5), (-1, 0, -0.5), 2, 200),
        ((en, nn - 229.5, 300 + 0.5 * 199.5), (0, 1, -0.5), 0, 200),    # northward
        ((en, nn - 199.5, 300 + 0.5 * 229.5), (0, 1, -0.5), 2, 200),
        ((en, nn - 255.5, 300 + 0.5 * 299.5), (0, 1, -0.5), 2, 256),    # leaves on the next chunk's first step
        ((en, nn - 256.5, 300 + 0.5 * 255.5), (0, 1, -0.5), 0, 256),    # hits there, would leave at 257
        ((ec, nc, 300 + 200.5), (0.3, -0.3, -1), 0, 201),               # from the north-west corner node inward
        ((es, ns, 300 + 200.5), (-0.3, 0.3, -1), 0, 201),               # from the south-east corner node inward
        ((ec, nc, 300 + 200.5), (-0.3, 0.3, -1), 2, 1),                 # from the corner outward
    ]
    return _case(g, [r[0] for r in rays], [r[1] for r in rays],
                 expect=dict(status=np.array([r[2] for r in rays]), steps=np.array([r[3] for r in rays])),
                 min_steps=150)


@functools.lru_cache(maxsize=None)
def case_stride(name):
    """Coordinates driven through what switches stride_positions between its branches."""
    ex = {}
    if name == "descent":  # heights through 512, 256 and 128 onto a plain at 100 m
        g = R.grid(LATC, LONC, fn=lambda la, lo: 100.0)
        e0, n0 = R.utm(LONC, LATC)
        hs = [700.0, 700.3, 650.123, 520.0, 513.37, 600.5, 512.0, 256.0]
        cs = [-0.7, -0.5, -0.61803, -0.9, -1.0]
        o = [(e0, n0, h + 0.17) for h in hs for _ in cs]
        d = [(0.1 * np.cos(k), 0.1 * np.sin(k), c) for k, h in enumerate(hs) for c in cs]
        kw = dict(max_search_dist=1500, min_steps=0)
        ex["status"] = np.zeros(len(o), int)
    elif name == "easting_2^19":  # a DEM centred on easting 524288, crossed eastward and westward
        lon, lat = D.utm_to_wgs84(524288.0, 2888500.0)
        g = R.grid(float(lat), float(lon), amp=0.2)
        o, d = [], []
        for sgn in (1.0, -1.0):
            for off, dd in [(260.4, (0.9, 0.05, -0.3)), (128.0, (1.0, 0.0, -0.25)), (64.0, (0.5, 0.25, -0.5)),
                            (300.7, (0.83, -0.11, -0.27)), (1.0, (2.0 ** -20, 0.3, -0.4)), (200.0, (0.7, 0.7, -0.2))]:
                o.append((524288.0 - sgn * off, 2888500.0, 440.0))
                d.append((sgn * dd[0], dd[1], dd[2]))
        kw = dict(max_search_dist=2500, min_steps=150)
        ex["cross"] = (0, 524288.0)
    elif name == "northing_2^21":  # a DEM centred on northing 2097152, crossed northward and southward
        lon, lat = D.utm_to_wgs84(600000.0, 2097152.0)
        g = R.grid(float(lat), float(lon), amp=0.2)
        o, d = [], []
        for sgn in (1.0, -1.0):
            for off, dd in [(260.4, (0.05, 0.9, -0.3)), (128.0, (0.0, 1.0, -0.25)), (64.0, (0.25, 0.5, -0.5)),
                            (300.7, (-0.11, 0.83, -0.27)), (1.0, (0.3, 2.0 ** -18, -0.4)), (200.0, (0.7, 0.7, -0.2))]:
                o.append((600000.0, 2097152.0 - sgn * off, 440.0))
                d.append((dd[0], sgn * dd[1], dd[2]))
        kw = dict(max_search_dist=2500, min_steps=150)
        ex["cross"] = (1, 2097152.0)
    elif name == "ties_and_zeros":  # on the central meridian: easting 500000 (ulp 2^-34), northing ~2.9e6 (ulp 2^-31)
        g = R.grid(LATC, 117.0, amp=0.2)
        n0 = float(np.floor(R.utm(117.0, LATC)[1]))
        t = 2.0 ** -35  # half an ulp of the easting: unnormalised directions, as the reference leaves them
        d = [(0.5 + t, 0.25, -0.5), (-(0.5 + t), 0.25, -0.5), (0.5 + 3 * t, -0.25, -0.25), (t, 0.0, -1.0), (-t, 0.0, -1.0),
             (0.25, 0.25 + 2.0 ** -32, -0.5), (0.25, -(0.5 + 3 * 2.0 ** -32), -0.5), (0.5 + t, 0.25 + 2.0 ** -32, -0.3),
             # one and two zero components, and none that moves
             (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.0, 0.5, -0.5), (0.7, 0.0, -0.3), (0.0, -1.0, 0.0), (0.0, 0.0, 0.0),
             (0.0, 0.0, 1.0), (-0.0, 0.3, -0.6)]
        o = [(500000.0, n0, 450.0)] * len(d)
        # A tie rounds to the even neighbour, so from an even starting mantissa (500000.0) every sum
        # lands on an even one and the stride is constant after all.  It is the odd start that makes
        # the first stride differ from the later ones: the case the tie check exists for.
        ue, un = 2.0 ** -34, 2.0 ** -31
        odd = [((500000.0 + ue, n0, 450.0), (0.5 + t, 0.25, -0.5)), ((500000.0 + ue, n0, 450.0), (-(0.5 + t), 0.25, -0.5)),
               ((500000.0 - ue, n0, 450.0), (0.5 + 3 * t, -0.25, -0.25)), ((500000.0 + ue, n0, 450.0), (t, 0.0, -1.0)),
               ((500000.0 + 3 * ue, n0, 450.0), (-t, 0.0, -1.0)), ((500000.0 + ue, n0, 450.0), (0.5 + ue + t, 0.1, -0.4)),
               ((500000.0, n0 + un, 450.0), (0.25, 0.25 + 2.0 ** -32, -0.5)),
               ((500000.0, n0 - un, 450.0), (0.25, -(0.5 + 3 * 2.0 ** -32), -0.5)),
               ((500000.0 + ue, n0 + un, 450.0), (0.5 + t, 0.25 + 2.0 ** -32, -0.3))]
        o, d = o + [r[0] for r in odd], d + [r[1] for r in odd]
        kw = dict(max_search_dist=1500, min_steps=150)
    elif name == "below_sea":  # heights through 0.0 and a change of sign; a start at exactly 0.0
        g = R.grid(LATC, LONC, base=-60.0, amp=0.2)
        e0, n0 = R.utm(LONC, LATC)
        o = [(e0, n0, 30.0), (e0, n0, 30.0), (e0, n0, 30.1), (e0, n0, 0.0), (e0, n0, 0.0), (e0, n0, -0.0),
             (e0, n0, 2.0 ** -30), (e0, n0, 64.0)]
        d = [(0.2, 0.1, -0.5), (0.2, 0.1, -0.7), (-0.2, 0.1, -0.3), (0.3, 0.0, -0.5), (0.0, 0.0, -1.0), (0.1, 0.2, -0.25),
             (0.1, -0.2, -0.5), (0.1, 0.1, -1.0)]
        kw = dict(max_search_dist=1500, min_steps=0)
        ex["status"] = np.zeros(len(o), int)
    else:
        raise KeyError(name)
    return _case(g, o, d, expect=ex, **kw)


def _hole_grid():
    g = R.grid(LATC, LONC)
    g["z"][13:21, 30:39] = np.nan   # east of the centre node (18, 26)
    return g


@functools.lru_cache(maxsize=None)
def case_nodata():
    """A no-data hole: the reference's comparison with NaN is false, so rays march through it."""
    g = _hole_grid()
    rng = np.random.default_rng(31)
    e0, n0 = R.utm(LONC, LATC)
    h0 = _ground(R.grid(LATC, LONC), e0, n0) + 120.0
    az = np.radians(rng.uniform(60, 120, 48))
    sl = rng.uniform(0.15, 0.6, 48)
    d = np.c_[np.sin(az), np.cos(az), -sl]
    return _case(g, [(e0, n0, h0)], d, max_search_dist=1200, min_steps=0)


@functools.lru_cache(maxsize=None)
def case_nonfinite(min_steps):
    g = R.grid(LATC, LONC)
    e0, n0 = R.utm(LONC, LATC)
    gh = _ground(g, e0, n0)
    h = gh + 100.0 if min_steps else gh - 5.0   # min_steps 0: step 0 is already a hit
    nan, inf = np.nan, np.inf
    good = (0.3, 0.2, -0.5)
    rays = [((nan, n0, h), good), ((e0, nan, h), good), ((nan, nan, nan), good), ((e0, n0, nan), good),
            ((e0, n0, h), (nan, 0.2, -0.5)), ((e0, n0, h), (0.3, nan, -0.5)), ((e0, n0, h), (0.3, 0.2, nan)),
            ((e0, n0, h), (inf, 0.2, -0.5)), ((e0, n0, h), (-inf, 0.2, -0.5)), ((e0, n0, h), (0.3, inf, -0.5)),
            ((e0, n0, h), (0.3, -inf, -0.5)), ((e0, n0, h), (0.3, 0.2, inf)), ((e0, n0, h), (0.3, 0.2, -inf)),
            ((e0, n0, h), (nan, nan, nan)), ((inf, n0, h), good), ((e0, n0, h), good)]
    if min_steps:
        st = [2, 2, 2, None, 2, 2, None, 2, 2, 2, 2, None, 0, 2, 2, 0]
        sp = [0, 0, 0, None, 1, 1, None, 1, 1, 1, 1, None, min_steps, 1, 0, None]
    else:
        st = [2, 2, 2, None, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0]
        sp = [0, 0, 0, None, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    return _case(g, [r[0] for r in rays], [r[1] for r in rays], expect=dict(status_opt=st, steps_opt=sp),
                 max_search_dist=900, min_steps=min_steps)


@functools.lru_cache(maxsize=None)
def case_pixels():
    """pixel_to_geo with non-unit z factors: the rescaled, renormalised directions of main_v1.py:661-683."""
    from rsac.dem import pixel_to_ray
    g = R.grid(LATC, LONC)
    rng = np.random.default_rng(41)
    K, Rm = synth.main_v1_K(), synth.camera_rotation(40.0, 25.0)
    px = rng.uniform([0, 0], [synth.IMAGE_W, synth.IMAGE_H], (96, 2))
    zf = rng.uniform(0.6, 1.6, 96)
    e0, n0 = R.utm(LONC, LATC)
    d = pixel_to_ray(px, K, Rm).copy()
    d[:, 2] *= zf
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c = _case(g, [(e0, n0, _ground(g, e0, n0) + 160.0)], d, max_search_dist=900, min_steps=150)
    c.update(pixels=px, K=K, R=Rm, zf=zf)
    return c


CASES = ([("layout", (k,)) for k in LAYOUTS] + [("layout", ("north_up", "zone40S")), ("layout", ("south_up", "zone1N"))] +
         [("pinned", cfg) for cfg in PIN_CONFIGS] + [("order", (k,)) for k in LAYOUTS] +
         [("stride", (k,)) for k in ("descent", "easting_2^19", "northing_2^21", "ties_and_zeros", "below_sea")] +
         [("nodata", ()), ("nonfinite", (150,)), ("nonfinite", (0,)), ("pixels", ())])
CASE_IDS = ["-".join([k] + [str(a) for a in args]) for k, args in CASES]


def _get(kind, args):
    return globals()["case_" + kind](*args)


def _check_intent(kind, args, c):
    """Oracle-only: the scene does what it was built for (the margins are asserted by the caller)."""
    m, ex = c["m"], c["expect"]
    if "status" in ex:
        np.testing.assert_array_equal(m["status"], ex["status"])
    if "steps" in ex:
        np.testing.assert_array_equal(m["steps"], ex["steps"])
    for key, opt in (("status", ex.get("status_opt")), ("steps", ex.get("steps_opt"))):
        if opt is not None:
            for i, v in enumerate(opt):
                assert v is None or m[key][i] == v, (key, i, m[key][i], v)
    if "cross" in ex:  # the hit lies on the other side of the binade boundary from the origin
        axis, edge = ex["cross"]
        hit = m["status"] == 0
        crossed = hit & ((c["origins"][:, axis] - edge) * (m["hits"][:, axis] - edge) < 0)
        assert crossed.sum() >= 8 and (c["origins"][crossed, axis] < edge).any() and (c["origins"][crossed, axis] > edge).any()
    if kind == "layout":
        assert set(m["status"].tolist()) == {0, 1, 2}
        assert len(np.unique(c["origins"], axis=0)) == 5
        # the three layouts hold the same ground: with every margin cleared, the same steps
        ref = case_layout("north_up", *args[1:])["m"]
        np.testing.assert_array_equal(m["steps"], ref["steps"])
        np.testing.assert_array_equal(m["status"], ref["status"])
    if kind == "pinned" and args == (0, 1200, 1):
        assert set(PIN_STEPS + [1199]) <= set(m["steps"][m["status"] == 0].tolist()) and m["status"][-1] == 1
    if kind == "stride" and args[0] == "descent":
        assert (m["hits"][:, 2] < 128.0).all() and (c["origins"][:, 2] > 256.0).all()
    if kind == "stride" and args[0] == "below_sea":
        assert (m["hits"][:, 2] < 0.0).all() and (c["origins"][:, 2] >= 0.0).all()
    if kind == "nodata":
        through = (m["nan_cells"] > 0) & (m["status"] == 0)
        assert through.sum() >= 8, through.sum()


@pytest.mark.parametrize("kind,args", CASES, ids=CASE_IDS)
def test_case_margins(kind, args):
    c = _get(kind, args)
    R.assert_margins(c["m"])
    _check_intent(kind, args, c)
    # the issue's limits on shapes
    assert max(c["g"]["z"].shape) <= 64 and min(c["g"]["z"].shape) <= 48
    assert len(c["dirs"]) <= 512 and c["kw"].get("max_search_dist", 10000) / c["kw"].get("step", 1) <= 10000


def _through_hole(c, k):
    m = c["m"]
    return np.flatnonzero((m["nan_cells"] > 0) & (m["status"] == 0))[:k]


def test_oracle_marches_through_nodata_like_the_literal_loop():
    """ray_intersect_dem_many against the literal loop over a NaN hole: 8 rays, 600 steps.  Only a
    point outside the axes (or a NaN point) is off the DEM; before the oracle's explicit bounds test
    a no-data cell ended the ray with status 2."""
    c = case_nodata()
    g = c["g"]
    idx = _through_hole(c, 6).tolist()
    idx += [i for i in range(len(c["dirs"])) if i not in idx][:2]
    d = c["dirs"][idx]
    hits, st = D.ray_intersect_dem_many(c["origins"][0], d, g["z"], g["y0"], g["dy"], g["x0"], g["dx"],
                                        max_search_dist=600, min_steps=0)
    interp = D.make_interpolator(g["z"], g["y0"], g["dy"], g["x0"], g["dx"])
    assert (st == 0).sum() >= 4
    for i in range(len(idx)):
        h, s = D.ray_intersect_dem(c["origins"][0], d[i], interp, max_search_dist=600, min_steps=0)
        assert s == st[i], (i, s, st[i])
        if s == 0:
            np.testing.assert_array_equal(h, hits[i])


# ------------------------------------------------------------------ CPU: projection accuracy against mpmath

def _utm_points():
    """3 x 104 points: +-3.5 deg of longitude about the central meridian, latitudes 0 .. 84 deg, in
    zone 50 north, zone 40 south and zone 1 north."""
    rng = np.random.default_rng(51)
    dl = np.r_[rng.uniform(-3.5, 3.5, 96), 0.0, 0.0, 3.5, -3.5, 3.0, -3.0, 0.0, 1e-9]
    la = np.r_[rng.uniform(0.0, 84.0, 96), 0.0, 84.0, 0.0, 84.0, 45.0, 1e-7, 26.0936, 60.0]
    return [(50, False, 117.0 + dl, la), (40, True, 57.0 + dl, -la), (1, False, -177.0 + dl, la)]


def _mp_krueger():
    """Krueger's series to n^6 at 40 digits, from the published formulas (Karney 2011, eqs. 35-36 and
    the rectifying radius of eq. 14), in exact rationals of n."""
    import mpmath as mp
    mp.mp.dps = 40
    q = lambda a, b=1: mp.mpf(a) / mp.mpf(b)
    f = 1 / mp.mpf("298.257223563")
    a = mp.mpf(6378137)
    n = f / (2 - f)
    A = a / (1 + n) * (1 + n ** 2 / 4 + n ** 4 / 64 + n ** 6 / 256)
    poly = lambda first, cs: sum(c * n ** (first + i) for i, c in enumerate(cs))
    alpha = [poly(1, [q(1, 2), q(-2, 3), q(5, 16), q(41, 180), q(-127, 288), q(7891, 37800)]),
             poly(2, [q(13, 48), q(-3, 5), q(557, 1440), q(281, 630), q(-1983433, 1935360)]),
             poly(3, [q(61, 240), q(-103, 140), q(15061, 26880), q(167603, 181440)]),
             poly(4, [q(49561, 161280), q(-179, 168), q(6601661, 7257600)]),
             poly(5, [q(34729, 80640), q(-3418889, 1995840)]),
             poly(6, [q(212378941, 319334400)])]
    beta = [poly(1, [q(1, 2), q(-2, 3), q(37, 96), q(-1, 360), q(-81, 512), q(96199, 604800)]),
            poly(2, [q(1, 48), q(1, 15), q(-437, 1440), q(46, 105), q(-1118711, 3870720)]),
            poly(3, [q(17, 480), q(-37, 840), q(-209, 4480), q(5569, 90720)]),
            poly(4, [q(4397, 161280), q(-11, 504), q(-830251, 7257600)]),
            poly(5, [q(4583, 161280), q(-108847, 3991680)]),
            poly(6, [q(20648693, 638668800)])]
    e = mp.sqrt(f * (2 - f))
    k0A = q(9996, 10000) * A

    def taup_of(tau):
        sig = mp.sinh(e * mp.atanh(e * tau / mp.sqrt(1 + tau ** 2)))
        return tau * mp.sqrt(1 + sig ** 2) - sig * mp.sqrt(1 + tau ** 2)

    def forward(lon, lat, zone, south):
        lon0 = mp.radians(-183 + 6 * zone)
        phi, dl = mp.radians(mp.mpf(float(lat))), mp.radians(mp.mpf(float(lon))) - lon0
        tp = taup_of(mp.tan(phi))
        xip, etap = mp.atan2(tp, mp.cos(dl)), mp.asinh(mp.sin(dl) / mp.hypot(tp, mp.cos(dl)))
        xi = xip + sum(alpha[j - 1] * mp.sin(2 * j * xip) * mp.cosh(2 * j * etap) for j in range(1, 7))
        eta = etap + sum(alpha[j - 1] * mp.cos(2 * j * xip) * mp.sinh(2 * j * etap) for j in range(1, 7))
        return 500000 + k0A * eta, (10000000 if south else 0) + k0A * xi

    def inverse(E, N, zone, south):
        lon0 = mp.radians(-183 + 6 * zone)
        xi, eta = (mp.mpf(float(N)) - (10000000 if south else 0)) / k0A, (mp.mpf(float(E)) - 500000) / k0A
        xip = xi - sum(beta[j - 1] * mp.sin(2 * j * xi) * mp.cosh(2 * j * eta) for j in range(1, 7))
        etap = eta - sum(beta[j - 1] * mp.cos(2 * j * xi) * mp.sinh(2 * j * eta) for j in range(1, 7))
        tp = mp.sin(xip) / mp.hypot(mp.sinh(etap), mp.cos(xip))
        tau = tp / (1 - e ** 2)
        for _ in range(10):  # Newton on tau'(tau) = tp (eqs. 19-21), quadratic: 1e-2 -> below 1e-40
            t = taup_of(tau)
            tau += (tp - t) * (1 + (1 - e ** 2) * tau ** 2) / ((1 - e ** 2) * mp.sqrt(1 + t ** 2) * mp.sqrt(1 + tau ** 2))
        return mp.degrees(lon0 + mp.atan2(mp.sinh(etap), mp.cos(xip))), mp.degrees(mp.atan(tau))

    return forward, inverse


@functools.lru_cache(maxsize=None)
def utm_truth():
    """Per variant: (zone, south, lon, lat, EN f64 (the forward truth rounded: the inverse's input),
    forward truth (mp), inverse truth of EN (mp))."""
    fwd, inv = _mp_krueger()
    out = []
    for zone, south, lon, lat in _utm_points():
        F = [fwd(lo, la, zone, south) for lo, la in zip(lon, lat)]
        EN = np.array([[float(e), float(n)] for e, n in F])
        I = [inv(e, n, zone, south) for e, n in EN]
        out.append((zone, south, lon, lat, EN, F, I))
    return out


def _utm_errors(forward_fn, inverse_fn):
    """Largest |computed - truth| of forward (m) and inverse (deg) over every variant."""
    import mpmath as mp
    fe = ie = 0.0
    for zone, south, lon, lat, EN, F, I in utm_truth():
        e, n = forward_fn(lon, lat, zone, south)
        lo, la = inverse_fn(EN[:, 0], EN[:, 1], zone, south)
        for k in range(len(lon)):
            fe = max(fe, float(abs(mp.mpf(float(e[k])) - F[k][0])), float(abs(mp.mpf(float(n[k])) - F[k][1])))
            ie = max(ie, float(abs(mp.mpf(float(lo[k])) - I[k][0])), float(abs(mp.mpf(float(la[k])) - I[k][1])))
    return fe, ie


def test_oracle_utm_accuracy_vs_mpmath():
    fe, ie = _utm_errors(D.wgs84_to_utm, D.utm_to_wgs84)
    print(f"oracle vs 40-digit series: forward {fe:.3e} m, inverse {ie:.3e} deg")
    assert sum(len(v[2]) for v in utm_truth()) == 312
    # the recorded figures are this measurement, rounded up in the third digit
    assert fe <= ORACLE_FWD_ERR_M and ie <= ORACLE_INV_ERR_DEG
    # and the GPU bounds made of them are no looser than test_dem.py's
    assert 8 * ORACLE_FWD_ERR_M <= 1e-6 and 8 * ORACLE_INV_ERR_DEG <= 1e-9


# ------------------------------------------------------------------ GPU

def _dem_grid(g):
    from rsac import dem
    return dem.DemGrid(g["z"], g["y0"], g["dy"], g["x0"], g["dx"])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,args", CASES, ids=CASE_IDS)
def test_gpu_march_equals_oracle(kind, args):
    from rsac import dem
    c = _get(kind, args)
    R.assert_margins(c["m"])
    hits, st = dem.ray_intersect_dem(c["origins"], c["dirs"], _dem_grid(c["g"]), **c["kw"])
    R.assert_equal(c["m"], hits, st)
    if kind == "layout" and args[0] != "north_up":
        # the layouts agree with each other, not only each with its oracle
        ref = case_layout("north_up", *args[1:])
        h0, s0 = dem.ray_intersect_dem(ref["origins"], ref["dirs"], _dem_grid(ref["g"]), **ref["kw"])
        np.testing.assert_array_equal(st, s0)
        np.testing.assert_array_equal(hits, h0)


@pytest.mark.gpu
def test_gpu_nodata_equals_literal_loop():
    from rsac import dem
    c = case_nodata()
    g = c["g"]
    idx = _through_hole(c, 4)
    assert len(idx) == 4
    hits, st = dem.ray_intersect_dem(c["origins"][idx], c["dirs"][idx], _dem_grid(g), **c["kw"])
    interp = D.make_interpolator(g["z"], g["y0"], g["dy"], g["x0"], g["dx"])
    for k, i in enumerate(idx):
        h, s = D.ray_intersect_dem(c["origins"][i], c["dirs"][i], interp, **c["kw"])
        assert s == 0 and st[k] == 0
        np.testing.assert_array_equal(hits[k], h)


@pytest.mark.gpu
def test_gpu_python_device_path():
    """rsac.dem.ray_intersect_dem with CUDA-tensor directions (_ray_intersect_dem_device)."""
    import torch
    from rsac import dem
    c = case_layout("south_up")
    R.assert_margins(c["m"])
    g = _dem_grid(c["g"])
    dev = torch.device("cuda:0")
    h_ref, s_ref = dem.ray_intersect_dem(c["origins"], c["dirs"], g, **c["kw"])
    R.assert_equal(c["m"], h_ref, s_ref)

    def same(h, s, href=h_ref, sref=s_ref):
        assert isinstance(h, torch.Tensor) and h.is_cuda and h.dtype == torch.float64 and tuple(h.shape) == href.shape
        assert isinstance(s, torch.Tensor) and s.is_cuda and s.dtype == torch.int8
        np.testing.assert_array_equal(s.cpu().numpy(), sref)
        np.testing.assert_array_equal(h.cpu().numpy(), href)

    d_t = torch.tensor(c["dirs"], dtype=torch.float64, device=dev)
    assert "_device_z" not in g.__dict__
    same(*dem.ray_intersect_dem(c["origins"], d_t, g, **c["kw"]))             # per-ray origins (host array)
    z_cached = g.__dict__["_device_z"][0]
    o_t = torch.tensor(c["origins"], dtype=torch.float64, device=dev)
    same(*dem.ray_intersect_dem(o_t, d_t, g, **c["kw"]))                      # device origins, cached DEM
    assert g.__dict__["_device_z"][0] is z_cached
    # non-contiguous directions: every other column of a (N, 6) tensor
    wide = torch.zeros((len(c["dirs"]), 6), dtype=torch.float64, device=dev)
    wide[:, ::2] = d_t
    view = wide[:, ::2]
    assert not view.is_contiguous()
    same(*dem.ray_intersect_dem(c["origins"], view, g, **c["kw"]))
    # a single origin, float32 directions: the march of those directions widened to f64
    d32 = c["dirs"][:64].astype(np.float32)
    one = c["origins"][0]
    m32 = R.march(one, d32.astype(np.float64), c["g"], **c["kw"])
    R.assert_margins(m32)
    h32, s32 = dem.ray_intersect_dem(one, d32.astype(np.float64), g, **c["kw"])
    R.assert_equal(m32, h32, s32)
    same(*dem.ray_intersect_dem(one, torch.tensor(d32, device=dev), g, **c["kw"]), href=h32, sref=s32)
    same(*dem.ray_intersect_dem(torch.tensor(one, device=dev), torch.tensor(d32, device=dev), g, **c["kw"]),
         href=h32, sref=s32)
    with pytest.raises(ValueError):
        dem.ray_intersect_dem(c["origins"][:3], d_t, g)


@pytest.mark.gpu
def test_gpu_pixel_to_geo_z_factors():
    from rsac import dem
    c = case_pixels()
    R.assert_margins(c["m"])
    assert np.abs(c["zf"] - 1.0).min() > 1e-3
    hits, st = dem.pixel_to_geo(c["pixels"], c["K"], c["R"], c["origins"][0], _dem_grid(c["g"]), z_factors=c["zf"],
                                **c["kw"])
    R.assert_equal(c["m"], hits, st)
    assert set(c["m"]["status"].tolist()) >= {0}


def _abi_march(**over):
    """rsac_dem_ray_intersect on a valid 4-ray problem with some arguments replaced."""
    import rsac._lib as L
    c = case_order("north_up")
    g = c["g"]
    a = dict(o=c["origins"][:4].copy(), d=c["dirs"][:4].copy(), n=4, z=g["z"], ny=37, nx=53, y0=g["y0"], dy=g["dy"],
             x0=g["x0"], dx=g["dx"], zone=50, south=0, dist=1000.0, step=1.0, min_steps=150,
             hits=np.full((4, 3), 7.0), st=np.full(4, 7, np.int8))
    a.update(over)
    p = lambda v: None if v is None else v.ctypes.data
    ctx = L.context(0)
    with ctx.lock:
        rc = L.lib().rsac_dem_ray_intersect(ctx.handle, p(a["o"]), p(a["d"]), a["n"], p(a["z"]), a["ny"], a["nx"],
                                            a["y0"], a["dy"], a["x0"], a["dx"], a["zone"], a["south"], a["dist"],
                                            a["step"], a["min_steps"], 0, p(a["hits"]), p(a["st"]), None)
    return rc, a["hits"], a["st"]


@pytest.mark.gpu
def test_gpu_abi_argument_checks():
    import rsac._lib as L
    rc, hits, st = _abi_march()
    assert rc == 0
    np.testing.assert_array_equal(st, case_order("north_up")["m"]["status"][:4])
    bad = [dict(ny=1), dict(nx=1), dict(ny=0), dict(nx=-3), dict(dy=0.0), dict(dx=0.0), dict(dy=-0.0), dict(step=0.0),
           dict(step=-1.0), dict(step=float("nan")), dict(zone=0), dict(zone=61), dict(zone=-1), dict(n=-1),
           dict(o=None), dict(d=None), dict(z=None), dict(hits=None), dict(st=None)]
    for over in bad:
        rc, hits, st = _abi_march(**over)
        assert rc == L.EINVAL, over
        if hits is not None and st is not None:
            assert (hits == 7.0).all() and (st == 7).all(), over   # nothing written
    rc, hits, st = _abi_march(n=0)
    assert rc == 0 and (hits == 7.0).all() and (st == 7).all()
    # rsac_utm_convert
    ctx = L.context(0)
    src = np.array([[117.5, 26.0], [118.0, 27.0]])

    def conv(inp=src, n=2, zone=50, out="new"):
        o = np.full((2, 2), 7.0) if isinstance(out, str) else out
        with ctx.lock:
            rc = L.lib().rsac_utm_convert(ctx.handle, 0, None if inp is None else inp.ctypes.data, n, zone, 0, 0,
                                          None if o is None else o.ctypes.data, None)
        return rc, o

    rc, o = conv()
    e, n = D.wgs84_to_utm(src[:, 0], src[:, 1])
    assert rc == 0 and np.abs(o - np.c_[e, n]).max() < 1e-6
    for kw in (dict(inp=None), dict(out=None), dict(n=-1), dict(zone=0), dict(zone=61)):
        rc, o = conv(**kw)
        assert rc == L.EINVAL, kw
        assert o is None or (o == 7.0).all()
    rc, o = conv(n=0)
    assert rc == 0 and (o == 7.0).all()


@pytest.mark.gpu
def test_gpu_utm_grid_stride_second_trip():
    """n = 4096 * 256 + 257: the launch is capped at 4096 blocks of 256 threads, so 257 threads
    take a second trip of the grid-stride loop.  Bit for bit the same points converted in two
    halves (each below the cap: one trip); an oversized output's tail stays untouched."""
    import torch
    import rsac._lib as L
    from rsac import dem
    n = 4096 * 256 + 257
    rng = np.random.default_rng(61)
    ll = np.c_[117.0 + rng.uniform(-3.5, 3.5, n), rng.uniform(0.0, 84.0, n)]
    h = n // 2
    en = dem.wgs84_to_utm(ll)
    np.testing.assert_array_equal(en, np.r_[dem.wgs84_to_utm(ll[:h]), dem.wgs84_to_utm(ll[h:])])
    back = dem.utm_to_wgs84(en)
    np.testing.assert_array_equal(back, np.r_[dem.utm_to_wgs84(en[:h]), dem.utm_to_wgs84(en[h:])])
    assert np.abs(back - ll).max() < 1e-11   # every point was converted, none left at the zero fill
    # device buffers, output longer than n
    dev = torch.device("cuda:0")
    ctx = L.context(0)
    for inverse, src, want in ((0, ll, en), (1, en, back)):
        t_in = torch.tensor(src, dtype=torch.float64, device=dev)
        t_out = torch.full((n + 300, 2), -7.0, dtype=torch.float64, device=dev)
        with ctx.lock:
            L.check(L.lib().rsac_utm_convert(ctx.handle, inverse, t_in.data_ptr(), n, 50, 0, L.F_DEVICE_IN,
                                             t_out.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        got = t_out.cpu().numpy()
        np.testing.assert_array_equal(got[:n], want)
        assert (got[n:] == -7.0).all()


@pytest.mark.gpu
def test_gpu_utm_accuracy_vs_mpmath():
    """k_utm_forward / k_utm_inverse against the 40-digit series: within 8 x the oracle's own error."""
    from rsac import dem

    def fwd(lon, lat, zone, south):
        en = dem.wgs84_to_utm(np.c_[lon, lat], zone=zone, south=south)
        return en[:, 0], en[:, 1]

    def inv(e, n, zone, south):
        ll = dem.utm_to_wgs84(np.c_[e, n], zone=zone, south=south)
        return ll[:, 0], ll[:, 1]

    fe, ie = _utm_errors(fwd, inv)
    print(f"kernels vs 40-digit series: forward {fe:.3e} m, inverse {ie:.3e} deg")
    assert fe <= 8 * ORACLE_FWD_ERR_M, fe
    assert ie <= 8 * ORACLE_INV_ERR_DEG, ie
