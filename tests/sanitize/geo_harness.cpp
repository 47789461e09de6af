// TEST INFRASTRUCTURE (tests/sanitize): the host+device pieces of the pixel -> ground path
// (rsac_geo.h: stride_closed_form, dem_interp, utm_inverse_fast / utm_inverse, dem_march -- the
// source k_dem_march runs) under ASan + UBSan + float-cast-overflow on the CPU.  A stand-alone
// program with no HIP runtime call, built by geo.mk (make -f geo.mk run) and by
// tests/test_dem_edges.py::test_geo_harness; never loaded into Python, never run on a GPU machine.
// Exit status 0 = every check passed (the sanitizers abort on a finding).
// Checks:
//   1. stride_closed_form: the kernel's chunking (W = 256: x + t * delta where the function says
//      so, additions one by one otherwise, the next chunk from the value at base + W) against
//      plain x = x + c, every step bit for bit, 2048 steps per (x, c) pair; starting values mid
//      binade, at binade edges, descending through binades, near and at zero; steps random, +-1,
//      +-0.5, 0, dyadic, larger than |x|, half-ulp ties, below ulp / 2, NaN / inf.  Both branches
//      must be taken in every family.
//   2. dem_interp: 3 x 4 and 2 x 2 grids, the four sign combinations of dy and dx: nodes, cell
//      centres, edges, one ulp outside, NaN coordinates, a NaN cell, the row stride.
//   3. utm_inverse_fast against utm_inverse over a lattice of eastings / northings, both
//      hemispheres, zones 1 / 40 / 50 / 60.
//   4. dem_march (the sequential host form) against the literal three-line loop, statuses 0 / 1 / 2.
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <limits>
#include <random>
#include <vector>

#include "rsac_geo.h"

using namespace rsac;

static int g_fail = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) {                                                              \
            fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                                            \
        }                                                                        \
    } while (0)

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0 || (a != a && b != b); }

static double ulp_of(double x) {
    int ex;
    frexp(x, &ex);
    return ldexp(1.0, ex - 53);
}

// ---------------------------------------------------------------- 1. stride_closed_form
constexpr int kW = 256;
constexpr int kChunks = 8;  // 2048 steps per pair

struct Tally {
    long closed = 0, stepped = 0, pairs = 0, mismatches = 0;
};

// stride_positions of rsac_kernels.hip for every t of a chunk at once
static void run_pair(double x0, double c, Tally &ty) {
    double ref = x0;  // the reference's sequential position at step base + t
    double x = x0;    // the chunked position at step base
    ++ty.pairs;
    for (int chunk = 0; chunk < kChunks; ++chunk) {
        double delta = 0.0;
        const bool closed = stride_closed_form(x, c, kW, delta);
        closed ? ++ty.closed : ++ty.stepped;
        double seq = x;
        for (int t = 0; t < kW; ++t) {
            const double xt = closed ? x + (double)t * delta : seq;
            if (!same_bits(xt, ref)) ++ty.mismatches;
            ref = ref + c;
            seq = seq + c;
        }
        x = closed ? x + (double)kW * delta : seq;
        if (!same_bits(x, ref)) ++ty.mismatches;
    }
}

static void stride_family(const char *name, const std::vector<double> &xs, unsigned seed, Tally &total) {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> uc(-2.0, 2.0);
    Tally ty;
    for (double x : xs) {
        std::vector<double> cs;
        for (int i = 0; i < 160; ++i) cs.push_back(uc(rng));
        for (double v : {1.0, 0.5, 0.0}) {
            cs.push_back(v);
            cs.push_back(-v);
        }
        for (int k = 1; k <= 44; k += 3) {  // dyadic, one and two bits
            cs.push_back(ldexp(1.0, -k));
            cs.push_back(-ldexp(3.0, -k));
            cs.push_back(0.5 + ldexp(1.0, -k));
            cs.push_back(-(0.25 + ldexp(1.0, -k)));
        }
        const double ax = fabs(x), u = ulp_of(x == 0.0 ? 1.0 : x);
        for (double m : {1.5, 2.0, 3.0, 40.0}) {  // |c| > |x|
            cs.push_back(m * (ax + 1e-3));
            cs.push_back(-m * (ax + 1e-3));
        }
        for (int k = 0; k < 6; ++k) {  // half-ulp ties of the rounding of c onto x's grid
            cs.push_back((k + 0.5) * u);
            cs.push_back(-(k + 0.5) * u);
            cs.push_back(0.5 + (k + 0.5) * u);
            cs.push_back(-(1.0 + (k + 0.5) * u));
            cs.push_back(ldexp(1.0, -7) + (k + 0.5) * u);
        }
        for (double f : {0.25, 0.49, 1e-3}) {  // below ulp / 2: the position never moves
            cs.push_back(f * u);
            cs.push_back(-f * u);
        }
        cs.push_back(std::numeric_limits<double>::denorm_min());
        cs.push_back(-std::numeric_limits<double>::min());
        for (double ccur : cs) run_pair(x, ccur, ty);
        // non-finite step: additions one by one, every chunk
        for (double bad : {nan, inf, -inf}) {
            Tally tb;
            run_pair(x, bad, tb);
            CHECK(tb.mismatches == 0 && tb.closed == 0);
            ty.stepped += tb.stepped;
            ty.pairs += tb.pairs;
        }
    }
    if (ty.mismatches || !ty.closed || !ty.stepped)
        fprintf(stderr, "stride family %s: %ld pairs, %ld closed-form chunks, %ld step-by-step chunks, %ld mismatches\n",
                name, ty.pairs, ty.closed, ty.stepped, ty.mismatches);
    CHECK(ty.mismatches == 0);
    CHECK(ty.closed > 0);   // both branches in every family
    CHECK(ty.stepped > 0);
    total.closed += ty.closed;
    total.stepped += ty.stepped;
    total.pairs += ty.pairs;
    total.mismatches += ty.mismatches;
}

static void check_stride() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    Tally total;
    stride_family("mid-binade", {500000.0, 2887000.0, 739000.25, 2888500.0 + 1.0 / 3.0}, 11, total);
    stride_family("binade edges", {524288.0 - 40.0, 524288.0 + 3.0, 4194304.0 - 100.0, 524288.0, 2097152.0 - 0.125}, 12,
                  total);
    stride_family("binade descent", {700.0, 520.0, 300.0, 130.0, 65.0, 512.0 + 1e-9, 256.0}, 13, total);
    stride_family("near zero", {1.0, 1e-3, -5.0, 0.0, -0.0, 5e-324}, 14, total);
    // non-finite position: never the closed form, no cast or shift of a non-finite value
    for (double bad : {nan, inf, -inf})
        for (double c : {0.0, 1.0, -0.5, nan, inf}) {
            Tally tb;
            run_pair(bad, c, tb);
            CHECK(tb.mismatches == 0 && tb.closed == 0);
        }
    printf("stride_closed_form: %ld pairs, %ld closed-form chunks, %ld step-by-step chunks, %ld mismatches\n",
           total.pairs, total.closed, total.stepped, total.mismatches);
}

// ---------------------------------------------------------------- 2. dem_interp
static void check_interp_grid(int ny, int nx, double y0, double dy, double x0, double dx, bool exact_centres) {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    std::vector<double> z((size_t)ny * nx);
    for (int i = 0; i < ny; ++i)
        for (int j = 0; j < nx; ++j) z[(size_t)i * nx + j] = 100.0 * i + j;  // pins the row stride
    const DemGrid g{z.data(), ny, nx, y0, dy, x0, dx};
    auto lat_of = [&](int i) { return (double)i * dy + y0; };
    auto lon_of = [&](int j) { return (double)j * dx + x0; };
    double out;
    // every node returns its own value exactly (the four corners among them)
    for (int i = 0; i < ny; ++i)
        for (int j = 0; j < nx; ++j) {
            out = -1.0;
            CHECK(dem_interp(g, lat_of(i), lon_of(j), out));
            CHECK(out == 100.0 * i + j);
        }
    // cell centres: the mean of the four corners
    for (int i = 0; i + 1 < ny; ++i)
        for (int j = 0; j + 1 < nx; ++j) {
            const double lat = 0.5 * (lat_of(i) + lat_of(i + 1)), lon = 0.5 * (lon_of(j) + lon_of(j + 1));
            const double mean = 0.25 * (z[(size_t)i * nx + j] + z[(size_t)i * nx + j + 1] + z[(size_t)(i + 1) * nx + j] +
                                        z[(size_t)(i + 1) * nx + j + 1]);
            CHECK(dem_interp(g, lat, lon, out));
            // a coordinate of ~120 deg carries 1.4e-14 deg, 5e-11 of a cell; the rows differ by 100
            if (exact_centres)
                CHECK(out == mean);
            else
                CHECK(fabs(out - mean) < 1e-7);
        }
    // the four outer edges are inside, one ulp beyond each is outside
    const double ya = lat_of(0), yb = lat_of(ny - 1), xa = lon_of(0), xb = lon_of(nx - 1);
    const double ylo = ya < yb ? ya : yb, yhi = ya < yb ? yb : ya, xlo = xa < xb ? xa : xb, xhi = xa < xb ? xb : xa;
    const double ym = 0.5 * (ylo + yhi) + 0.1 * fabs(dy), xm = 0.5 * (xlo + xhi) + 0.1 * fabs(dx);
    CHECK(dem_interp(g, ylo, xm, out) && dem_interp(g, yhi, xm, out));
    CHECK(dem_interp(g, ym, xlo, out) && dem_interp(g, ym, xhi, out));
    CHECK(dem_interp(g, ylo, xlo, out) && dem_interp(g, ylo, xhi, out) && dem_interp(g, yhi, xlo, out) &&
          dem_interp(g, yhi, xhi, out));
    CHECK(!dem_interp(g, nextafter(ylo, -inf), xm, out));
    CHECK(!dem_interp(g, nextafter(yhi, inf), xm, out));
    CHECK(!dem_interp(g, ym, nextafter(xlo, -inf), out));
    CHECK(!dem_interp(g, ym, nextafter(xhi, inf), out));
    CHECK(!dem_interp(g, nextafter(yhi, inf), nextafter(xhi, inf), out));
    // NaN / infinite coordinates are outside
    CHECK(!dem_interp(g, nan, xm, out) && !dem_interp(g, ym, nan, out) && !dem_interp(g, nan, nan, out));
    CHECK(!dem_interp(g, inf, xm, out) && !dem_interp(g, ym, -inf, out));
    // along an edge the value interpolates that edge's row / column only
    CHECK(dem_interp(g, lat_of(0), 0.5 * (lon_of(0) + lon_of(1)), out) && fabs(out - 0.5) < 1e-7);
    CHECK(dem_interp(g, 0.5 * (lat_of(ny - 2) + lat_of(ny - 1)), lon_of(nx - 1), out) &&
          fabs(out - (100.0 * (ny - 1.5) + (nx - 1))) < 1e-7);
    // a no-data cell: inside, value NaN (the march goes on: height <= NaN is false)
    std::vector<double> zn = z;
    zn[0] = nan;
    const DemGrid gn{zn.data(), ny, nx, y0, dy, x0, dx};
    out = 0.0;
    CHECK(dem_interp(gn, 0.5 * (lat_of(0) + lat_of(1)), 0.5 * (lon_of(0) + lon_of(1)), out));
    CHECK(out != out);
    out = 0.0;
    CHECK(dem_interp(gn, lat_of(0), lon_of(0), out) && out != out);
    if (nx > 2) {  // a cell that does not touch the hole is unaffected
        CHECK(dem_interp(gn, lat_of(ny - 1), lon_of(nx - 1), out) && out == 100.0 * (ny - 1) + (nx - 1));
    }
}

static void check_interp() {
    for (int sy : {-1, 1})
        for (int sx : {-1, 1}) {
            // GDAL-like spacings (1.5" x 1") and dyadic ones, where every quotient is exact
            check_interp_grid(3, 4, 26.0936, sy / 2400.0, 119.3906, sx / 3600.0, false);
            check_interp_grid(2, 2, 26.0936, sy / 2400.0, 119.3906, sx / 3600.0, false);
            check_interp_grid(3, 4, 26.0, sy * ldexp(1.0, -11), 119.0, sx * ldexp(1.0, -12), true);
            check_interp_grid(2, 2, 26.0, sy * ldexp(1.0, -11), 119.0, sx * ldexp(1.0, -12), true);
            check_interp_grid(3, 4, -0.0005, sy / 2400.0, -0.0004, sx / 3600.0, false);  // axes through zero
        }
}

// ---------------------------------------------------------------- 3. utm_inverse_fast
static void check_inverse_fast() {
    const TmConst k = tm_const();
    double worst = 0.0;
    for (int zone : {1, 40, 50, 60})
        for (int south = 0; south < 2; ++south) {
            const UtmZone z = utm_zone(zone, south != 0);
            for (int ie = 0; ie <= 40; ++ie)
                for (int in = 0; in <= 93; ++in) {
                    const double E = 166000.0 + 16700.0 * ie;  // ie = 20: the zone centre, eta = 0
                    const double N = south ? 1e7 - 1e5 * in : 1e5 * in;
                    double lon, lat, lonf, latf;
                    utm_inverse(k, z, E, N, lon, lat);
                    utm_inverse_fast(k, z, E, N, lonf, latf);
                    CHECK(dfinite(lonf) && dfinite(latf));
                    const double dl = fabs(lonf - lon), db = fabs(latf - lat);
                    if (dl > worst) worst = dl;
                    if (db > worst) worst = db;
                    if (ie == 20) CHECK(lon == -183.0 + 6.0 * zone || fabs(lon - (-183.0 + 6.0 * zone)) < 1e-13);
                }
        }
    printf("utm_inverse_fast vs utm_inverse: largest difference %.3e deg\n", worst);
    // measured 1.279e-13 deg (x86-64, glibc; a few ulps of a longitude near 180 deg, whose ulp is
    // 2.8e-14 deg: the two forms round the same series differently -- not the 1e-15 deg of one ulp of
    // the radian value); 4x for another libm.  It must stay below 1e-12 deg (0.1 um on the ground):
    // a march decision with a 1e-6 m margin then cannot flip.
    constexpr double kMeasured = 1.279e-13;
    constexpr double kBound = 4 * kMeasured;
    static_assert(kBound < 1e-12, "utm_inverse_fast must agree with utm_inverse to 1e-12 deg");
    CHECK(worst <= kBound);
}

// ---------------------------------------------------------------- 4. dem_march
static int literal_march(const TmConst &k, const UtmZone &z, const DemGrid &g, const double *o, const double *d,
                         int n_steps, double step, int min_steps, double *pos) {
    double p[3] = {o[0], o[1], o[2]};
    for (int s = 0; s < n_steps; ++s) {
        double lon, lat, elev;
        utm_inverse(k, z, p[0], p[1], lon, lat);
        if (!dem_interp(g, lat, lon, elev)) return 2;
        if (s >= min_steps && p[2] <= elev) return memcpy(pos, p, sizeof p), 0;
        for (int a = 0; a < 3; ++a) p[a] += step * d[a];
    }
    return 1;
}

static void check_march() {
    const TmConst k = tm_const();
    const UtmZone z = utm_zone(50, false);
    const int ny = 3, nx = 4;
    std::vector<double> zz((size_t)ny * nx);
    for (int i = 0; i < ny; ++i)
        for (int j = 0; j < nx; ++j) zz[(size_t)i * nx + j] = 100.0 * i + j;
    const double y0 = 26.0936, dy = -1.0 / 2400, x0 = 119.3906, dx = 1.0 / 3600;
    const DemGrid g{zz.data(), ny, nx, y0, dy, x0, dx};
    double E, N;
    utm_forward(k, z, x0 + 1.5 * dx, y0 + 1.0 * dy, E, N);  // the grid's centre (~83 m x 92 m)
    struct Ray {
        double o[3], d[3];
        int n_steps;
        double step;
        int min_steps, want;
    };
    const Ray rays[] = {
        {{E, N, 250.0}, {0.05, 0.03, -1.0}, 10000, 1.0, 0, 0},     // down: hit
        {{E, N, 250.0}, {0.05, -0.03, -1.0}, 10000, 0.5, 150, 0},  // half-metre steps
        {{E, N, 50.0}, {0.0, 0.0, -1.0}, 10000, 1.0, 7, 0},        // underground: hit exactly at min_steps
        {{E, N, 250.0}, {0.05, 0.03, -1.0}, 20, 1.0, 0, 1},        // search too short
        {{E, N, 50.0}, {0.0, 0.0, -1.0}, 7, 1.0, 7, 1},            // min_steps == n_steps
        {{E, N, 250.0}, {0.1, 0.1, -1.0}, 0, 1.0, 0, 1},           // no step at all
        {{E, N, 250.0}, {1.0, 0.0, 0.0}, 10000, 1.0, 0, 2},        // level: leaves the grid eastward
        {{E, N, 250.0}, {0.0, -1.0, -0.01}, 10000, 1.0, 150, 2},   // leaves southward
        {{E + 500.0, N, 250.0}, {0.0, 0.0, -1.0}, 10000, 1.0, 0, 2},  // origin outside
        {{E, N, 50.0}, {1.0, 0.0, 0.0}, 10000, 1.0, 150, 2},       // underground but gone before min_steps
    };
    int seen[3] = {0, 0, 0};
    for (const Ray &r : rays) {
        double a[3] = {-1, -1, -1}, b[3] = {-1, -1, -1};
        const int sa = dem_march(k, z, g, r.o, r.d, r.n_steps, r.step, r.min_steps, a);
        const int sb = literal_march(k, z, g, r.o, r.d, r.n_steps, r.step, r.min_steps, b);
        CHECK(sa == sb && sa == r.want);
        CHECK(same_bits(a[0], b[0]) && same_bits(a[1], b[1]) && same_bits(a[2], b[2]));
        if (sa == 0) CHECK(a[2] <= 203.0 && a[2] < r.o[2] + 1e-9);
        if (sa >= 0 && sa < 3) ++seen[sa];
    }
    CHECK(seen[0] && seen[1] && seen[2]);
    // the hit of the third ray is min_steps additions below the origin
    double a[3];
    CHECK(dem_march(k, z, g, rays[2].o, rays[2].d, 10000, 1.0, 7, a) == 0 && a[2] == 43.0);
}

int main() {
    check_stride();
    check_interp();
    check_inverse_fast();
    check_march();
    printf("%s (%d failed checks)\n", g_fail ? "FAILED" : "ok", g_fail);
    return g_fail ? 1 : 0;
}
