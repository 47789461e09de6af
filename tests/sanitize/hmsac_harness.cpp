// TEST INFRASTRUCTURE (tests/sanitize): the host-only pieces of MSAC scoring for homographies
// (csrc/rsac_host.hip: hom_cost_host -- the source k_hom_cost / k_hom_cost_lane run --, scan_step_msac;
// rsac_math.h msac_shift / msac_q / msac_term) under ASan + UBSan on the CPU.  A stand-alone program,
// built by hmsac.mk and run by hand (make -f hmsac.mk run); not a pytest test, never loaded into
// Python, never run on a GPU machine.  Exit status 0 = every check passed (the sanitizers abort on a
// finding).  Checks:
//   1. counts and costs over 20 000 points, some with inf / NaN coordinates, some exactly on a model's
//      pole (denominator 0), against a literal loop in double arithmetic, for thresholds from a
//      subnormal thr2 to 3e38;
//   2. n = 0 .. 9 and an all-outlier sum above 2^32;
//   3. the scan with model_points = 4 fed in chunks == fed at once == the literal loop.
#include <stdio.h>
#include <string.h>

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

// the definition: k = 19 - floor(log2 thr2), an inlier costs floor(e 2^k), any other point floor(thr2 2^k)
static int64_t cost_literal(const float *sx, const float *sy, const float *dx, const float *dy, int n, const double *H,
                            float thr2, int32_t *count) {
    float hf[8];
    for (int q = 0; q < 8; ++q) hf[q] = (float)H[q];
    int ex = 0;
    frexp((double)thr2, &ex);  // thr2 = m 2^ex, m in [0.5, 1): floor(log2 thr2) = ex - 1
    const int k = 19 - (ex - 1);
    const int64_t Q = (int64_t)floor(ldexp((double)thr2, k));
    int64_t cost = 0;
    *count = 0;
    for (int i = 0; i < n; ++i) {
        const float e = hom_err(hf, sx[i], sy[i], dx[i], dy[i]);
        if (e <= thr2) {
            cost += (int64_t)floor(ldexp((double)e, k));
            ++*count;
        } else {
            cost += Q;
        }
    }
    return cost;
}

static void fill(std::mt19937_64 &rng, int n, std::vector<float> &soa, double bad_fraction) {
    std::uniform_real_distribution<float> U(0.f, 1000.f);
    std::uniform_real_distribution<double> B(0.0, 1.0);
    soa.assign((size_t)4 * std::max(n, 1), 0.f);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int i = 0; i < n; ++i) {
        const float x = U(rng), y = U(rng);
        soa[i] = x;
        soa[(size_t)n + i] = y;
        soa[(size_t)2 * n + i] = 1.1f * x + 3.f + 0.01f * U(rng);
        soa[(size_t)3 * n + i] = 0.9f * y - 2.f + 0.01f * U(rng);
        if (B(rng) < bad_fraction) {
            const int k = (int)(rng() % 4);
            const float v[4] = {inf, -inf, nan, -nan};
            soa[(size_t)(rng() % 4) * n + i] = v[k];
        }
    }
}

static void check_costs(std::mt19937_64 &rng) {
    const double models[4][9] = {{1.1, 0, 3, 0, 0.9, -2, 0, 0, 1},
                                 {1.1, 0.001, 3, -0.002, 0.9, -2, 1e-6, -2e-6, 1},
                                 {1, 0, 0, 0, 1, 0, -1.0 / 512, 0, 1},  // a pole at x = 512
                                 {0, 0, 0, 0, 0, 0, -1.0 / 512, 0, 1}}; // ... with a zero numerator: 0 * inf
    // thr2: subnormal, the smallest normal, ordinary bounds (3, 8 and 75 px), huge, FLT_MAX
    const float thr2s[] = {1e-45f, 3e-39f, 1.17549435e-38f, 1e-6f, 9.f, 64.f, 5625.f, 1e30f, 3e38f, 3.402823466e38f};
    for (double bad : {0.0, 0.01, 0.5}) {
        const int n = 20000;
        std::vector<float> soa;
        fill(rng, n, soa, bad);
        for (int i = 0; i < 64; ++i) soa[(size_t)i * 300] = 512.f;  // exactly on the pole
        const float *b = soa.data();
        for (const auto &H : models)
            for (float t2 : thr2s) {
                int32_t c0 = -1, c1 = -1;
                const int64_t got = hom_cost_host(b, b + n, b + 2 * n, b + 3 * n, n, H, t2, &c0);
                const int64_t want = cost_literal(b, b + n, b + 2 * n, b + 3 * n, n, H, t2, &c1);
                CHECK(got == want && c0 == c1);
                CHECK(got >= 0 && got <= (int64_t)n * (1 << 20));
                CHECK(msac_q(t2, msac_shift(t2)) >= (1u << 19) && msac_q(t2, msac_shift(t2)) < (1u << 20));
            }
    }
}

static void check_small_and_large() {
    const double H[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int n = 0; n <= 9; ++n) {
        std::vector<float> soa((size_t)4 * std::max(n, 1), 0.f);
        for (int i = 0; i < n; ++i) soa[(size_t)2 * n + i] = (float)i;  // e = i^2
        const float *b = soa.data();
        int32_t c0 = -1, c1 = -1;
        CHECK(hom_cost_host(b, b + n, b + 2 * n, b + 3 * n, n, H, 9.f, &c0) ==
              cost_literal(b, b + n, b + 2 * n, b + 3 * n, n, H, 9.f, &c1));
        CHECK(c0 == c1 && c0 == std::min(n, 4));
        CHECK(hom_cost_host(b, b + n, b + 2 * n, b + 3 * n, n, H, 9.f, nullptr) >= 0);  // count_out is optional
    }
    const int n = 8200;  // every point an outlier at Q = 2^19: the sum passes 2^32
    std::vector<float> soa((size_t)4 * n, 0.f);
    for (int i = 0; i < n; ++i) soa[(size_t)2 * n + i] = 1000.f;
    const float *b = soa.data();
    int32_t c = -1;
    CHECK(hom_cost_host(b, b + n, b + 2 * n, b + 3 * n, n, H, 64.f, &c) == (int64_t)n << 19 && c == 0);
    CHECK(((int64_t)n << 19) > (1ll << 32));
}

static void check_scan(std::mt19937_64 &rng) {
    for (int trial = 0; trial < 400; ++trial) {
        const int64_t H = 1 + rng() % 3000;
        const int n = 4 + (int)(rng() % 300);
        std::vector<int8_t> st(H);
        std::vector<int32_t> cnt(H);
        std::vector<int64_t> cost(H);
        for (int64_t i = 0; i < H; ++i) {
            st[i] = rng() % 9 == 0 ? 0 : 1;
            cnt[i] = st[i] ? (int32_t)(rng() % (n + 1)) : 0;
            cost[i] = st[i] ? (int64_t)(rng() % 64) + ((int64_t)(rng() % 3) << 32) : -1;  // many ties
        }
        if (trial % 5 == 0) st[rng() % H] = -1;
        const int max_iters = 1 + (int)(rng() % 3500);
        const double conf = trial % 2 ? 0.995 : 0.5;
        ScanState a, b;
        int64_t ca = -1, cb = -1;
        a.reset(max_iters);
        b.reset(max_iters);
        scan_step_msac(a, ca, cnt.data(), cost.data(), st.data(), H, n, 4, conf);
        for (int64_t i = 0; i < H;) {
            const int64_t c = std::min<int64_t>(H - i, 1 + rng() % 700);
            scan_step_msac(b, cb, cnt.data() + i, cost.data() + i, st.data() + i, c, n, 4, conf);
            i += c;
        }
        CHECK(a.best == b.best && a.iter == b.iter && a.done == b.done && a.max_good == b.max_good && ca == cb &&
              a.niters == b.niters);
        // the literal loop
        int64_t best = -1, bc = -1, i = 0, niters = std::max(max_iters, 1);
        int32_t good = 0;
        for (; i < H && i < niters; ++i) {
            if (st[i] < 0) break;
            if (st[i] > 0 && cnt[i] > 3 && (best < 0 || cost[i] < bc)) {
                best = i;
                bc = cost[i];
                good = cnt[i];
                niters = update_num_iters(conf, (double)(n - good) / n, 4, (int)niters);
            }
        }
        CHECK(a.best == best && a.iter == i && ca == bc && a.max_good == good && a.niters == niters);
    }
}

int main() {
    std::mt19937_64 rng(20240611);
    check_costs(rng);
    check_small_and_large();
    check_scan(rng);
    printf("hmsac harness: %s (%d failed checks)\n", g_fail ? "FAILED" : "ok", g_fail);
    return g_fail ? 1 : 0;
}
