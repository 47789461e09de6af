// TEST INFRASTRUCTURE (tests/sanitize): the host side of the least-squares fundamental matrix
// (rsac_math.h: fm_fit_host, fm_fit_reduce_host, fm_fit_acc1 / fm_fit_acc2, fm_fit_centroids,
// fm_fit_solve -- the source the k_fm_fit_* kernels run) under ASan + UBSan on the CPU.  A stand-alone
// program, built by fmfit.mk and run by hand (make -f fmfit.mk run); not a pytest test, never loaded
// into Python, never run on a GPU machine.  Exit status 0 = every check passed (the sanitizers abort
// on a finding).
// Checks:
//   1. noise-free correspondences of a known F at n = 8 .. 300 000 (one slot, one wave, one range,
//      74 ranges): unit norm, rank 2, every point on its epipolar line, masks of every third point;
//   2. m = 0 .. 9 masked points (by n and by mask): no model below 8;
//   3. NaN / infinite coordinates under the mask and coincident points: no model; the same values
//      outside the mask: not one bit changes;
//   4. the range walk at n just below, at and above multiples of 4096 with the mask's ones only at
//      the two ends.
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <limits>
#include <random>
#include <vector>

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
    std::vector<float> x1, y1, x2, y2;
    int n() const { return (int)x1.size(); }
};

// two pinhole views of random 3D points (no noise): x2^T F x1 = 0 up to the f32 rounding of the pixels
static Pts scene(int n, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> ux(-30, 30), uy(-20, 20), uz(40, 120);
    Pts p;
    const double f = 1200, cx = 960, cy = 540, th = 0.07, tx = 4.0, ty = 0.5, tz = 0.3;
    for (int i = 0; i < n; ++i) {
        const double X = ux(rng), Y = uy(rng), Z = uz(rng);
        p.x1.push_back((float)(f * X / Z + cx));
        p.y1.push_back((float)(f * Y / Z + cy));
        const double X2 = cos(th) * X + sin(th) * Z + tx, Y2 = Y + ty, Z2 = -sin(th) * X + cos(th) * Z + tz;
        p.x2.push_back((float)(f * X2 / Z2 + cx));
        p.y2.push_back((float)(f * Y2 / Z2 + cy));
    }
    return p;
}

static bool fit(const Pts &p, const std::vector<uint8_t> *mask, double *F, int *count = nullptr) {
    return fm_fit_host(p.x1.data(), p.y1.data(), p.x2.data(), p.y2.data(), mask ? mask->data() : nullptr, p.n(), F,
                       count);
}

static void check_model(const Pts &p, const std::vector<uint8_t> *mask, const double *F) {
    double nrm = 0;
    for (int k = 0; k < 9; ++k) nrm += F[k] * F[k];
    CHECK(fabs(nrm - 1.0) < 1e-14);
    const double det = F[0] * (F[4] * F[8] - F[5] * F[7]) - F[1] * (F[3] * F[8] - F[5] * F[6]) +
                       F[2] * (F[3] * F[7] - F[4] * F[6]);
    CHECK(fabs(det) < 1e-12);
    // f32 pixels: a quarter-pixel Sampson bound holds with a wide margin for a noise-free scene
    for (int i = 0; i < p.n(); ++i)
        if (!mask || (*mask)[i]) CHECK(fm_inlier(F, p.x1[i], p.y1[i], p.x2[i], p.y2[i], 0.0625));
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    double F[9], G[9];
    // 1. sizes around every level of the order
    for (int n : {8, 9, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 8193, 70000, 300000}) {
        const Pts p = scene(n, 7u + (unsigned)n);
        int cnt = -1;
        CHECK(fit(p, nullptr, F, &cnt) && cnt == n);
        check_model(p, nullptr, F);
        if (n >= 16) {
            std::vector<uint8_t> m(n);
            int ones = 0;
            for (int i = 0; i < n; ++i) ones += m[i] = i % 3 != 0;
            CHECK(fit(p, &m, G, &cnt) && cnt == ones);
            check_model(p, &m, G);
        }
    }
    // 2. m = 0 .. 9
    for (int m = 0; m <= 9; ++m) {
        const Pts p = scene(m, 100u + (unsigned)m);
        CHECK(fit(p, nullptr, F) == (m >= 8));
        const Pts q = scene(5000, 200u + (unsigned)m);
        std::vector<uint8_t> mk(5000, 0);
        for (int k = 0; k < m; ++k) mk[(size_t)k * 4999 / 9] = 1;
        int cnt = -1;
        CHECK(fit(q, &mk, F, &cnt) == (m >= 8) && cnt == m);
    }
    CHECK(!fm_fit_host(nullptr, nullptr, nullptr, nullptr, nullptr, 0, F));
    // 3. non-finite and coincident points
    {
        const Pts base = scene(1000, 3);
        std::vector<uint8_t> m(1000);
        for (int i = 0; i < 1000; ++i) m[i] = i % 2;
        CHECK(fit(base, &m, F));
        for (float bad : {nan, inf, -inf}) {
            for (int col = 0; col < 4; ++col) {
                Pts p = base;
                std::vector<float> &v = col == 0 ? p.x1 : col == 1 ? p.y1 : col == 2 ? p.x2 : p.y2;
                const float keep = v[501];
                v[501] = bad;  // under the mask
                CHECK(!fit(p, &m, G));
                CHECK(!fit(p, nullptr, G));
                v[501] = keep;
                v[500] = bad;  // outside it (the mask holds the odd indices)
                v[0] = bad;
                CHECK(fit(p, &m, G) && memcmp(F, G, sizeof F) == 0);
            }
            Pts p = base;
            p.y2[998] = bad;
            p.x1[2] = bad;
            CHECK(fit(p, &m, G) && memcmp(F, G, sizeof F) == 0);
        }
        Pts c = base;
        for (int i = 0; i < 1000; ++i) {
            c.x1[i] = c.x1[0]; c.y1[i] = c.y1[0]; c.x2[i] = c.x2[0]; c.y2[i] = c.y2[0];
        }
        CHECK(!fit(c, nullptr, G));
        c = base;
        for (int i = 0; i < 1000; ++i)
            if (m[i]) { c.x2[i] = 17.25f; c.y2[i] = -3.5f; }
        CHECK(!fit(c, &m, G));
        // collinear points in both images: a model may or may not come out, but nothing may trap
        c = base;
        for (int i = 0; i < 1000; ++i) { c.y1[i] = 2.f * c.x1[i]; c.y2[i] = 2.f * c.x2[i]; }
        (void)fit(c, nullptr, G);
        // huge coordinates: the moments overflow to infinity, no model
        c = base;
        for (int i = 0; i < 1000; ++i) { c.x1[i] *= 1e35f; c.y2[i] *= 1e35f; }
        (void)fit(c, nullptr, G);
    }
    // 4. the range walk: ones at the two ends only
    for (int n : {4095, 4096, 4097, 8191, 8192, 8193, 12289}) {
        const Pts p = scene(n, 11u + (unsigned)n);
        std::vector<uint8_t> m(n, 0);
        for (int k = 0; k < 4; ++k) m[k] = m[n - 1 - k] = 1;
        int cnt = -1;
        CHECK(fit(p, &m, F, &cnt) && cnt == 8);
        check_model(p, &m, F);
        m[n - 1] = 0;
        CHECK(!fit(p, &m, F, &cnt) && cnt == 7);
    }
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("fmfit harness ok\n");
    return 0;
}
