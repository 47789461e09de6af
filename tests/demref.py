"""TEST INFRASTRUCTURE for tests/test_dem_edges.py: scenes for the DEM ray march and the oracle's
march with its decision margins.

The bar of test_dem_edges.py is "status and hit equal the batched oracle bit for bit on every ray".
The kernel and the oracle evaluate the same projection series in different forms (Clenshaw +
delta series against direct sums + Newton), so their (lat, lon) differ in the last places and a
decision that hangs on those places may legitimately flip.  `march` therefore reports, per ray,
how far every decision of the oracle's own march was from flipping:

  * hmargin: the smallest |height - elevation| over the steps from min_steps to the deciding one
    (every "not yet a hit" and the final "hit" is a comparison of those two numbers);
  * bmargin: the smallest distance, in degrees, of (lat, lon) to the grid's bounds over the steps
    up to and including the deciding one (this includes the step before a grid exit and the exit).

`assert_margins` requires hmargin > 1e-6 m and bmargin > 1e-12 deg of every ray: 1e-12 deg (0.1 um)
is above the kernel's and the oracle's projection difference (tests/sanitize/geo_harness.cpp holds
utm_inverse_fast to 5.2e-13 deg of utm_inverse (4 x the measured 1.279e-13); test_dem_edges holds both inverses to the series'
value), and a coordinate change of 1e-12 deg moves an interpolated height of these scenes by
less than 1e-8 m.  Scenes are fixed by seed so that every ray clears both; a borderline ray means
another seed, never a tolerance.
"""
import numpy as np

import dem_oracle as D

H_MARGIN = 1e-6     # metres
B_MARGIN = 1e-12    # degrees


def terrain(lat, lon, latc, lonc, base=300.0, amp=1.0):
    """A smooth surface with no symmetry, as a function of the geographic position (so the same
    ground can be laid out with either sign of dy / dx).  ~+-150 m * amp about `base` over 0.015 deg."""
    u, v = (np.asarray(lat) - latc) * 400.0, (np.asarray(lon) - lonc) * 400.0
    return base + amp * (70.0 * np.sin(1.3 * u + 0.4) + 50.0 * np.cos(0.9 * v - 1.1) +
                         30.0 * np.sin(0.7 * u - 1.7 * v + 0.2) + 12.0 * u - 7.0 * v)


def grid(latc, lonc, ny=37, nx=53, ady=1.0 / 2400, adx=1.0 / 3600, south_up=False, east_first=False, fn=None,
         base=300.0, amp=1.0):
    """A DEM of ny x nx nodes centred on (latc, lonc): dict(z, y0, dy, x0, dx).  Default layout is
    GDAL's north-up (dy < 0, dx > 0); south_up gives dy > 0, east_first gives dx < 0, the array
    laid out to match (z[i, j] is the ground at lat_i, lon_j of that layout)."""
    hy, hx = 0.5 * (ny - 1) * ady, 0.5 * (nx - 1) * adx
    y0, dy = (latc - hy, ady) if south_up else (latc + hy, -ady)
    x0, dx = (lonc + hx, -adx) if east_first else (lonc - hx, adx)
    lat = np.arange(ny) * dy + y0
    lon = np.arange(nx) * dx + x0
    LA, LO = np.meshgrid(lat, lon, indexing="ij")
    z = terrain(LA, LO, latc, lonc, base, amp) if fn is None else np.asarray(fn(LA, LO), np.float64) + np.zeros_like(LA)
    return dict(z=np.ascontiguousarray(z), y0=float(y0), dy=float(dy), x0=float(x0), dx=float(dx))


def bounds(g):
    ny, nx = g["z"].shape
    ya, yb = g["y0"], (ny - 1) * g["dy"] + g["y0"]
    xa, xb = g["x0"], (nx - 1) * g["dx"] + g["x0"]
    return min(ya, yb), max(ya, yb), min(xa, xb), max(xa, xb)


def utm(lon, lat, zone=50, south=False):
    e, n = D.wgs84_to_utm(lon, lat, zone, south)
    return float(e), float(n)


def march(origins, dirs, g, max_search_dist=10000, step=1, min_steps=150, zone=50, south=False):
    """D.ray_intersect_dem_many with the margins: dict(hits, status, steps (the deciding step index,
    n_steps for status 1), hmargin, bmargin, nan_cells (steps that read a no-data cell)).  The hits
    and statuses are asserted equal to the oracle's own, so this is its march and no second one."""
    from scipy.interpolate import RegularGridInterpolator
    z = np.asarray(g["z"], np.float64)
    dem_x = np.arange(z.shape[1]) * g["dx"] + g["x0"]
    dem_y = np.arange(z.shape[0]) * g["dy"] + g["y0"]
    interp = RegularGridInterpolator((dem_y, dem_x), z)
    ylo, yhi, xlo, xhi = bounds(g)
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    pos = np.array(origins, np.float64).reshape(-1, 3).copy()
    if pos.shape[0] == 1:
        pos = np.repeat(pos, d.shape[0], axis=0)
    n = d.shape[0]
    n_steps = int(max_search_dist / step)
    hits = np.full((n, 3), np.nan)
    status = np.ones(n, np.int8)
    steps = np.full(n, n_steps, np.int64)
    hmargin = np.full(n, np.inf)
    bmargin = np.full(n, np.inf)
    nan_cells = np.zeros(n, np.int64)
    live = np.arange(n)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(n_steps):
            if live.size == 0:
                break
            lon, lat = D.utm_to_wgs84(pos[live, 0], pos[live, 1], zone, south)
            bm = np.minimum(np.minimum(np.abs(lat - ylo), np.abs(yhi - lat)),
                            np.minimum(np.abs(lon - xlo), np.abs(xhi - lon)))
            bm[np.isnan(bm)] = np.inf      # a NaN point is off the DEM whatever its last places
            bmargin[live] = np.minimum(bmargin[live], bm)
            off = ~((lat >= ylo) & (lat <= yhi) & (lon >= xlo) & (lon <= xhi))
            elev = np.full(live.size, np.nan)
            if not off.all():
                elev[~off] = interp(np.c_[lat[~off], lon[~off]])
            nan_cells[live] += ~off & np.isnan(elev)
            if s >= min_steps:
                hm = np.abs(pos[live, 2] - elev)
                hm[np.isnan(hm) | off] = np.inf  # height <= NaN is false in every implementation
                hmargin[live] = np.minimum(hmargin[live], hm)
            hit = ~off & (s >= min_steps) & (pos[live, 2] <= elev)
            status[live[off]] = 2
            steps[live[off]] = s
            hits[live[hit]] = pos[live[hit]]
            status[live[hit]] = 0
            steps[live[hit]] = s
            live = live[~off & ~hit]
            pos[live, 0] += step * d[live, 0]
            pos[live, 1] += step * d[live, 1]
            pos[live, 2] += step * d[live, 2]
        oh, ost = D.ray_intersect_dem_many(origins, d, z, g["y0"], g["dy"], g["x0"], g["dx"], max_search_dist, step,
                                           min_steps, zone, south)
    np.testing.assert_array_equal(ost, status)
    np.testing.assert_array_equal(oh, hits)
    return dict(hits=hits, status=status, steps=steps, hmargin=hmargin, bmargin=bmargin, nan_cells=nan_cells)


def assert_margins(m):
    bad = np.flatnonzero(~(m["hmargin"] > H_MARGIN) | ~(m["bmargin"] > B_MARGIN))
    assert bad.size == 0, [(int(i), int(m["status"][i]), int(m["steps"][i]), m["hmargin"][i], m["bmargin"][i])
                           for i in bad[:8]]


def assert_equal(m, hits, status):
    """The bar: status and hit bit for bit, every ray."""
    hits, status = np.asarray(hits), np.asarray(status)
    bad = np.flatnonzero((status != m["status"]) | ~np.all((hits == m["hits"]) | (np.isnan(hits) & np.isnan(m["hits"])),
                                                           axis=1))
    assert bad.size == 0, (f"{bad.size} of {len(status)} rays differ", [
        (int(i), int(status[i]), int(m["status"][i]), int(m["steps"][i]), hits[i].tolist(), m["hits"][i].tolist())
        for i in bad[:6]])
    # -0.0 == 0.0 above: compare the hit coordinates' signs as well
    h = m["status"] == 0
    assert np.array_equal(np.signbit(hits[h]), np.signbit(m["hits"][h]))
