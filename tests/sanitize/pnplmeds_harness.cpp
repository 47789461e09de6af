// TEST INFRASTRUCTURE (tests/sanitize): the host-only LMedS PnP pieces of librsac (csrc/rsac_host.hip:
// pnp_median_host -- the source the k_pnp_median* kernels run --, and the host side of the driver's
// round: scan_step_lmeds over (status, median), lmeds_sigma, lmeds_num_iters for 4 and 5 model points)
// under ASan + UBSan on the CPU.  A stand-alone program, built by pnplmeds.mk and run by hand
// (make -f pnplmeds.mk run); not a pytest test, never loaded into Python, never run on a GPU machine.
// Exit status 0 = every check passed (the sanitizers abort on a finding).  Checks:
//   1. medians over 100 000 and 99 999 points against a sort of the same keys: the true pose, the
//      camera turned round (every point behind it), the camera inside the cloud (z of both signs and
//      z == 0 exactly), with 0 %, 1 %, 30 % and 70 % of the points carrying a NaN / inf coordinate;
//   2. n = 1 .. 9 against a sorted copy, with duplicates and NaN;
//   3. the driver's scan of a round and its bound: the best median's sigma and thr2 are finite and
//      positive for every n > model_points, 4 and 5 model points.
#include <stdio.h>

#include <algorithm>
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

static bool same(double a, double b) { return (a != a && b != b) || a == b; }

static const double kCam[4] = {1200.0, 1150.0, 640.0, 360.0};

static double median_by_sort(const std::vector<float> &soa, int n, const double *R, const double *t) {
    const float *b = soa.data();
    const Cam k{kCam[0], kCam[1], kCam[2], kCam[3]};
    std::vector<uint32_t> key((size_t)n);
    for (int i = 0; i < n; ++i)
        key[i] = lmeds_key(pnp_err(R, t, k, (double)b[i], (double)b[n + i], (double)b[2 * (size_t)n + i],
                                   b[3 * (size_t)n + i], b[4 * (size_t)n + i]));
    std::sort(key.begin(), key.end());
    return lmeds_median(n > 1 ? key[n / 2 - 1] : 0, key[n / 2], n);
}

// points in front of the identity camera at depth 5 .. 15, their noisy projections
static void fill(std::mt19937_64 &rng, int n, std::vector<float> &soa, double bad_fraction) {
    std::uniform_real_distribution<double> U(-1.0, 1.0), B(0.0, 1.0);
    soa.assign((size_t)5 * n, 0.f);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int i = 0; i < n; ++i) {
        const double z = 10.0 + 5.0 * U(rng), x = 3.0 * U(rng), y = 2.0 * U(rng);
        soa[i] = (float)x;
        soa[(size_t)n + i] = (float)y;
        soa[(size_t)2 * n + i] = (float)z;
        soa[(size_t)3 * n + i] = (float)(kCam[0] * x / z + kCam[2] + U(rng));
        soa[(size_t)4 * n + i] = (float)(kCam[1] * y / z + kCam[3] + U(rng));
        if (B(rng) < bad_fraction) {
            const float v[4] = {inf, -inf, nan, -nan};
            soa[(size_t)(rng() % 5) * n + i] = v[rng() % 4];
        }
    }
}

static double host_median(const std::vector<float> &soa, int n, const double *R, const double *t) {
    const float *b = soa.data();
    return pnp_median_host(b, b + n, b + 2 * (size_t)n, b + 3 * (size_t)n, b + 4 * (size_t)n, n, kCam, R, t);
}

static void check_medians(std::mt19937_64 &rng) {
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, flip[9] = {1, 0, 0, 0, -1, 0, 0, 0, -1};
    const double t0[3] = {0, 0, 0}, t_in[3] = {0, 0, -10.0};  // z - 10: both signs, and exactly 0 below
    for (double bad : {0.0, 0.01, 0.3, 0.7}) {
        for (int n : {100000, 99999}) {
            std::vector<float> soa;
            fill(rng, n, soa, bad);
            for (int i = 0; i < 64; ++i) soa[(size_t)2 * n + (size_t)i * 1000] = 10.f;  // z == 0 under t_in
            const double a = host_median(soa, n, I, t0);
            CHECK(same(a, median_by_sort(soa, n, I, t0)));
            if (bad == 0.0) CHECK(a > 0.0 && a < 4.0);  // the noise: uniform +-1 px in u and v
            if (bad == 0.7) CHECK(!(a < 1.7976931348623157e308));  // inf or NaN: never wins the scan
            CHECK(same(host_median(soa, n, flip, t0), median_by_sort(soa, n, flip, t0)));
            CHECK(same(host_median(soa, n, I, t_in), median_by_sort(soa, n, I, t_in)));
        }
    }
}

static void check_small() {
    std::mt19937_64 rng(5);
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t0[3] = {0, 0, 0};
    for (int n = 1; n <= 9; ++n) {
        for (int trial = 0; trial < 50; ++trial) {
            std::vector<float> soa((size_t)5 * n, 0.f);
            for (int i = 0; i < n; ++i) {
                soa[(size_t)2 * n + i] = 1.f;
                soa[(size_t)3 * n + i] = (float)(rng() % 4);  // many duplicates
            }
            if (trial % 7 == 0) soa[(size_t)3 * n] = std::numeric_limits<float>::quiet_NaN();
            if (trial % 11 == 0) soa[(size_t)2 * n + n - 1] = 0.f;  // z == 0
            CHECK(same(host_median(soa, n, I, t0), median_by_sort(soa, n, I, t0)));
        }
    }
    CHECK(lmeds_num_iters(0.99, 4, 2000) == 48);
    CHECK(lmeds_num_iters(0.99, 5, 2000) == 89);
    CHECK(lmeds_num_iters(0.99, 5, 1) == 3);
}

// the host side of the driver's round: the scan over a round's rows, then the winner's bound
static void check_round(std::mt19937_64 &rng) {
    for (int trial = 0; trial < 400; ++trial) {
        const int64_t H = 1 + rng() % 200;
        const int sk = 4 + (int)(trial & 1);
        const int n = sk + 1 + (int)(rng() % 100000);
        std::vector<int8_t> st(H);
        std::vector<double> med(H);
        for (int64_t i = 0; i < H; ++i) {
            st[i] = rng() % 9 == 0 ? 0 : 1;
            med[i] = (double)(float)((double)(rng() % 4096) / 16);
            if (rng() % 11 == 0) med[i] = std::numeric_limits<double>::quiet_NaN();
            if (rng() % 13 == 0) med[i] = std::numeric_limits<double>::infinity();
            if (st[i] == 0) med[i] = -1.0;
        }
        if (trial % 5 == 0) st[rng() % H] = -1;
        LmedsScan sc;
        sc.reset(H);
        scan_step_lmeds(sc, st.data(), med.data(), H);
        int64_t best = -1, i = 0;
        double bm = 1.7976931348623157e308;
        for (; i < H; ++i) {
            if (st[i] < 0) break;
            if (st[i] > 0 && med[i] < bm) {
                best = i;
                bm = med[i];
            }
        }
        CHECK(sc.best == best && sc.iter == i && sc.best_median == bm);
        if (sc.best >= 0) {
            const double sigma = lmeds_sigma(sc.best_median, n, sk);
            const float thr2 = (float)(sigma * sigma);
            CHECK(sigma >= 0.001 && std::isfinite(sigma) && thr2 > 0.f && std::isfinite(thr2));
        }
    }
}

int main() {
    std::mt19937_64 rng(20261020);
    check_medians(rng);
    check_small();
    check_round(rng);
    printf("pnp lmeds harness: %s (%d failed checks)\n", g_fail ? "FAILED" : "ok", g_fail);
    return g_fail ? 1 : 0;
}
