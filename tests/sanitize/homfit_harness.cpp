// TEST INFRASTRUCTURE (tests/sanitize): the host side of the homography refit (csrc/rsac_host.hip's
// hom_refine and the pieces of rsac_math.h it shares with the k_hom_fit kernel: hom_fit_lrows,
// hom_fit_point, hom_fit_denorm, hom_jacobi_*, hom_eig8_*, hom_lm_*) under ASan + UBSan on the CPU.
// A stand-alone program, built by homfit.mk and run by hand (make -f homfit.mk run); not a pytest
// test, never loaded into Python, never run on a GPU machine.  Exit status 0 = every check passed
// (the sanitizers abort on a finding).
// Checks:
//   1. noise-free correspondences of a known H at m = 4 .. 4097 masked points (around the 64-point
//      chunks of the kernel), with masks of all ones and of every third point: the refit maps every
//      masked point onto its partner;
//   2. noisy points with gross errors under the mask: a finite model, H[8] = 1;
//   3. fewer than 4 masked points and points equal in one coordinate: no model;
//   4. NaN / infinite / huge coordinates under the mask: nothing traps, whatever comes out;
//   5. the shared pieces on degenerate operands (zero and NaN matrices, a zero step).
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <limits>
#include <random>
#include <vector>

#include "rsac_host.h"
#include "rsac_math.h"

using namespace rsac;

static int g_fail = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) {                                                              \
            fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                                            \
        }                                                                        \
    } while (0)

struct Pts {
    std::vector<float> sx, sy, dx, dy;
    int n() const { return (int)sx.size(); }
};

static const double kH[9] = {1500.0, 40.0, 1000.0, 30.0, -1400.0, 700.0, 0.05, 0.3, 1.0};

static Pts scene(int n, unsigned seed, double noise) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> ux(-0.6, 0.6), uy(-0.2, 0.2);
    std::normal_distribution<double> g(0.0, 1.0);
    Pts p;
    for (int i = 0; i < n; ++i) {
        const float x = (float)ux(rng), y = (float)uy(rng);
        const double w = kH[6] * x + kH[7] * y + 1.0;
        p.sx.push_back(x);
        p.sy.push_back(y);
        p.dx.push_back((float)((kH[0] * x + kH[1] * y + kH[2]) / w + noise * g(rng)));
        p.dy.push_back((float)((kH[3] * x + kH[4] * y + kH[5]) / w + noise * g(rng)));
    }
    return p;
}

static bool fit(const Pts &p, const std::vector<uint8_t> &m, double *H) {
    return hom_refine(p.sx.data(), p.sy.data(), p.dx.data(), p.dy.data(), m.data(), p.n(), H);
}

static void check_maps(const Pts &p, const std::vector<uint8_t> &m, const double *H, double tol) {
    CHECK(H[8] == 1.0);
    for (int i = 0; i < p.n(); ++i) {
        if (!m[i]) continue;
        const double w = H[6] * p.sx[i] + H[7] * p.sy[i] + 1.0;
        CHECK(fabs((H[0] * p.sx[i] + H[1] * p.sy[i] + H[2]) / w - p.dx[i]) < tol);
        CHECK(fabs((H[3] * p.sx[i] + H[4] * p.sy[i] + H[5]) / w - p.dy[i]) < tol);
    }
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    double H[9];
    // 1. exact correspondences (up to the f32 rounding of the pixels: ~1e-4 px)
    for (int m : {4, 5, 8, 12, 63, 64, 65, 127, 128, 129, 1000, 4097}) {
        const Pts p = scene(m, 7u + (unsigned)m, 0.0);
        std::vector<uint8_t> ones(m, 1);
        CHECK(fit(p, ones, H));
        check_maps(p, ones, H, 5e-3);
        const int n = m + (m + 1) / 2 + 1;
        const Pts q = scene(n, 70u + (unsigned)m, 0.0);
        std::vector<uint8_t> third(n);
        int cnt = 0;
        for (int i = 0; i < n; ++i) cnt += third[i] = i % 3 != 0;
        CHECK(fit(q, third, H) == (cnt >= 4));
        if (cnt >= 4) check_maps(q, third, H, 5e-3);
    }
    // 2. noise and gross errors under the mask (the LM's rejected steps, restarts and iteration cap)
    for (double noise : {0.01, 0.5, 3.0}) {
        for (int n : {12, 65, 300, 4097}) {
            Pts p = scene(n, 300u + (unsigned)n, noise);
            for (int i = 3; i < n; i += 7) { p.dx[i] += 250.f; p.dy[i] -= 180.f; }
            std::vector<uint8_t> ones(n, 1);
            CHECK(fit(p, ones, H));
            for (int k = 0; k < 9; ++k) CHECK(std::isfinite(H[k]));
            CHECK(H[8] == 1.0);
        }
    }
    // 3. no model
    {
        const Pts p = scene(130, 5, 0.5);
        std::vector<uint8_t> m(130, 0);
        CHECK(!fit(p, m, H));
        m[0] = m[1] = m[129] = 1;
        CHECK(!fit(p, m, H));
        m[128] = 1;
        CHECK(fit(p, m, H));
        std::vector<uint8_t> ones(130, 1);
        for (int col = 0; col < 4; ++col) {
            Pts q = p;
            std::vector<float> &v = col == 0 ? q.sx : col == 1 ? q.sy : col == 2 ? q.dx : q.dy;
            for (float &e : v) e = v[0];
            CHECK(!fit(q, ones, H));
        }
    }
    // 4. non-finite and huge operands: the loops are bounded, nothing may trap
    {
        const Pts base = scene(200, 9, 0.5);
        std::vector<uint8_t> ones(200, 1);
        for (float bad : {nan, inf, -inf, 3e38f, 1e-38f}) {
            for (int col = 0; col < 4; ++col) {
                Pts q = base;
                std::vector<float> &v = col == 0 ? q.sx : col == 1 ? q.sy : col == 2 ? q.dx : q.dy;
                v[77] = bad;
                (void)fit(q, ones, H);
            }
        }
        Pts q = base;
        for (int i = 0; i < 200; ++i) { q.sx[i] *= 1e30f; q.dy[i] *= 1e30f; }
        (void)fit(q, ones, H);
        // collinear points: a rank-deficient system through the clipped pseudo-inverse
        q = base;
        for (int i = 0; i < 200; ++i) { q.sy[i] = 2.f * q.sx[i]; q.dy[i] = 2.f * q.dx[i]; }
        (void)fit(q, ones, H);
    }
    // 5. the shared pieces on degenerate operands
    {
        double W[64] = {0}, V[64] = {0}, b[8] = {1, 2, 3, 4, 5, 6, 7, 8}, x[8], A[64] = {0}, d[8] = {0};
        hom_eig8_clip(W);
        hom_eig8_solve(W, V, b, x);
        for (int k = 0; k < 8; ++k) CHECK(x[k] == 0.0);
        CHECK(hom_eig8_maxdiag(W, V) == kHomDblEps);
        CHECK(hom_lm_gain(A, b, d, 2.0, 1.0) == 1.0);  // a zero step: the denominator falls back to 1
        CHECK(hom_lm_nu(b, d, 2.0, 1.0) == 2.0);
        CHECK(hom_lm_dinf(d) == 0.0 && !hom_lm_go_on(1, 10, 0.0, 1.0) && !hom_lm_go_on(10, 10, 1.0, 1.0));
        for (int i = 0; i < 64; ++i) W[i] = std::numeric_limits<double>::quiet_NaN();
        hom_eig8_clip(W);
        hom_eig8_solve(W, V, b, x);
        (void)hom_eig8_maxdiag(W, V);
        CHECK(hom_jacobi_done(0.0, 0.0) && hom_jacobi_skip(0.0) && !hom_jacobi_skip(1.0));
        double c, s;
        hom_jacobi_rot(1.0, 1.0, 0.5, c, s);
        CHECK(fabs(c * c + s * s - 1.0) < 1e-15);
        double rx, ry, jx[8], jy[8];
        const double h[8] = {1, 0, 0, 0, 1, 0, 0, -1};
        hom_fit_point(h, 3.0, 1.0, 0.0, 0.0, rx, ry, jx, jy);  // w = 0: the projection is defined as 0
        CHECK(rx == 0.0 && ry == 0.0 && jx[2] == 0.0);
        hom_fit_point(h, 3.0, 2.0, 1.0, 1.0, rx, ry, nullptr, nullptr);
        CHECK(rx == -4.0 && ry == -3.0);
    }
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("homfit harness ok\n");
    return 0;
}
