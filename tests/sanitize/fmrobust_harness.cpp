// TEST INFRASTRUCTURE (tests/sanitize): the host-only pieces of MSAC and LMedS for the fundamental
// matrix (csrc/rsac_host.hip: fm_err_host / fm_cost_host / fm_median_host -- the source the k_fm_cost*
// and k_fm_median* kernels run --, scan_step_msac with 8 model points, scan_step_lmeds; rsac_math.h
// fm_err / fm_err_inl / fm_msac_term) under ASan + UBSan on the CPU.  A stand-alone program, built by
// fmrobust.mk and run by hand (make -f fmrobust.mk run); not a pytest test, never loaded into Python,
// never run on a GPU machine.  Exit status 0 = every check passed (the sanitizers abort on a finding).
// Checks:
//   1. errors, counts, costs and medians over 20 000 points, some with inf / NaN coordinates, under
//      ordinary models, models with a zero denominator (F = e3 e3^T, F = 0) and a model with huge
//      entries, against literal loops, for thresholds from a subnormal thr2 to FLT_MAX;
//   2. n = 0 .. 9 and an all-outlier sum above 2^32;
//   3. both scans fed in chunks == fed at once == the literal loops.
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

static uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// the definition: the error from fm_inlier's own chain, then k = 19 - floor(log2 thr2), an inlier
// below the bound costs floor(e 2^k), any other point floor(thr2 2^k)
static float err_literal(const double *F, double x1, double y1, double x2, double y2, double T, bool *inl) {
    const double a = fma(F[0], x1, fma(F[1], y1, F[2]));
    const double b = fma(F[3], x1, fma(F[4], y1, F[5]));
    const double c = fma(F[6], x1, fma(F[7], y1, F[8]));
    const double a2 = fma(F[0], x2, fma(F[3], y2, F[6]));
    const double b2 = fma(F[1], x2, fma(F[4], y2, F[7]));
    const double r = fma(x2, a, fma(y2, b, c));
    const double den = fma(a, a, fma(b, b, fma(a2, a2, b2 * b2)));
    const double r2 = r * r;
    *inl = r2 <= T * den;
    if (r2 == 0.0) return 0.f;
    return (float)(r2 / den);
}

static int64_t cost_literal(const float *x1, const float *y1, const float *x2, const float *y2, int n, const double *F,
                            float thr2, int32_t *count) {
    int ex = 0;
    frexp((double)thr2, &ex);  // thr2 = m 2^ex, m in [0.5, 1): floor(log2 thr2) = ex - 1
    const int k = 19 - (ex - 1);
    const int64_t Q = (int64_t)floor(ldexp((double)thr2, k));
    int64_t cost = 0;
    *count = 0;
    for (int i = 0; i < n; ++i) {
        bool inl;
        const float e = err_literal(F, x1[i], y1[i], x2[i], y2[i], (double)thr2, &inl);
        CHECK(inl == fm_inlier(F, x1[i], y1[i], x2[i], y2[i], (double)thr2));
        *count += inl;
        cost += (inl && e <= thr2) ? (int64_t)floor(ldexp((double)e, k)) : Q;
    }
    return cost;
}

static double median_literal(const std::vector<float> &e) {
    std::vector<uint32_t> key(e.size());
    for (size_t i = 0; i < e.size(); ++i) key[i] = std::isnan(e[i]) ? 0x7FC00000u : bits(e[i]);
    std::sort(key.begin(), key.end());
    const size_t n = key.size();
    float hi, lo;
    memcpy(&hi, &key[n / 2], 4);
    if (n & 1) return (double)hi;
    memcpy(&lo, &key[n / 2 - 1], 4);
    const float s = lo + hi;
    return (double)s * 0.5;
}

static bool same(double a, double b) { return memcmp(&a, &b, 8) == 0 || (std::isnan(a) && std::isnan(b)); }

static void fill(std::mt19937_64 &rng, int n, std::vector<float> &soa, double bad_fraction) {
    std::uniform_real_distribution<float> U(0.f, 1000.f);
    std::uniform_real_distribution<double> B(0.0, 1.0);
    soa.assign((size_t)4 * std::max(n, 1), 0.f);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int i = 0; i < n; ++i) {
        const float x = U(rng), y = U(rng);
        soa[i] = x;
        soa[(size_t)n + i] = y;
        soa[(size_t)2 * n + i] = x + 40.f + 0.01f * U(rng);
        soa[(size_t)3 * n + i] = (i % 3 == 0) ? y : y + 0.002f * U(rng);  // every third point exactly on its line
        if (B(rng) < bad_fraction) {
            const int k = (int)(rng() % 4);
            const float v[4] = {inf, -inf, nan, -nan};
            soa[(size_t)(rng() % 4) * n + i] = v[k];
        }
    }
}

static void check_scores(std::mt19937_64 &rng) {
    const double s = 0.7071067811865476;
    const double models[6][9] = {{0, 0, 0, 0, 0, -s, 0, s, 0},                       // x translation: lines y2 = y1
                                 {1e-7, 2e-6, -1e-3, -2e-6, 1e-7, -0.7, 1e-3, 0.7, 0.01},
                                 {0, 0, 0, 0, 0, 0, 0, 0, 1},                        // den == 0 < r^2: +inf
                                 {0, 0, 0, 0, 0, 0, 0, 0, 0},                        // r^2 == den == 0: error 0
                                 {1e150, 0, 0, 0, 1e150, 0, 0, 0, 1e150},            // r^2 and den overflow
                                 {0, 0, 0, 0, 0, -1e-170, 0, 1e-170, 0}};            // r^2 and den underflow
    // thr2: subnormal, the smallest normal, ordinary bounds (1.5 and 3 px), huge, FLT_MAX
    const float thr2s[] = {1e-45f, 3e-39f, 1.17549435e-38f, 1e-6f, 2.25f, 9.f, 1e30f, 3e38f, 3.402823466e38f};
    for (double bad : {0.0, 0.01, 0.5}) {
        const int n = 20000;
        std::vector<float> soa;
        fill(rng, n, soa, bad);
        const float *b = soa.data();
        std::vector<float> e(n), el(n);
        for (const auto &F : models) {
            fm_err_host(b, b + n, b + 2 * n, b + 3 * n, n, F, e.data());
            for (int i = 0; i < n; ++i) {
                bool inl;
                el[i] = err_literal(F, b[i], b[n + i], b[2 * n + i], b[3 * n + i], 1.0, &inl);
                CHECK(bits(e[i]) == bits(el[i]) || (std::isnan(e[i]) && std::isnan(el[i])));
                CHECK(std::isnan(e[i]) || e[i] >= 0.f);
            }
            CHECK(same(fm_median_host(b, b + n, b + 2 * n, b + 3 * n, n, F), median_literal(el)));
            CHECK(same(fm_median_host(b, b + n, b + 2 * n, b + 3 * n, n - 1, F),
                       median_literal(std::vector<float>(el.begin(), el.end() - 1))));
            for (float t2 : thr2s) {
                int32_t c0 = -1, c1 = -1;
                const int64_t got = fm_cost_host(b, b + n, b + 2 * n, b + 3 * n, n, F, t2, &c0);
                const int64_t want = cost_literal(b, b + n, b + 2 * n, b + 3 * n, n, F, t2, &c1);
                CHECK(got == want && c0 == c1);
                CHECK(got >= 0 && got <= (int64_t)n * (1 << 20));
            }
        }
    }
}

static void check_small_and_large() {
    const double s = 0.7071067811865476;
    const double F[9] = {0, 0, 0, 0, 0, -s, 0, s, 0};  // r = s (y1 - y2), den = 1: e = (y1 - y2)^2 / 2
    for (int n = 0; n <= 9; ++n) {
        std::vector<float> soa((size_t)4 * std::max(n, 1), 0.f), e(std::max(n, 1), -1.f);
        for (int i = 0; i < n; ++i) soa[(size_t)3 * n + i] = (float)i;
        const float *b = soa.data();
        int32_t c0 = -1, c1 = -1;
        CHECK(fm_cost_host(b, b + n, b + 2 * n, b + 3 * n, n, F, 5.f, &c0) ==
              cost_literal(b, b + n, b + 2 * n, b + 3 * n, n, F, 5.f, &c1));
        CHECK(c0 == c1 && c0 == std::min(n, 4));                                      // e = 0, .5, 2, 4.5 pass 5
        CHECK(fm_cost_host(b, b + n, b + 2 * n, b + 3 * n, n, F, 5.f, nullptr) >= 0);  // count_out is optional
        fm_err_host(b, b + n, b + 2 * n, b + 3 * n, n, F, e.data());
        if (n >= 1) {
            std::vector<float> el(e.begin(), e.begin() + n);
            CHECK(same(fm_median_host(b, b + n, b + 2 * n, b + 3 * n, n, F), median_literal(el)));
        }
    }
    const int n = 8200;  // every point an outlier at Q = 2^19: the sum passes 2^32
    std::vector<float> soa((size_t)4 * n, 0.f);
    for (int i = 0; i < n; ++i) soa[(size_t)3 * n + i] = 1000.f;
    const float *b = soa.data();
    int32_t c = -1;
    CHECK(fm_cost_host(b, b + n, b + 2 * n, b + 3 * n, n, F, 64.f, &c) == (int64_t)n << 19 && c == 0);
    CHECK(((int64_t)n << 19) > (1ll << 32));
}

static void check_scans(std::mt19937_64 &rng) {
    for (int trial = 0; trial < 400; ++trial) {
        const int64_t H = 1 + rng() % 3000;
        const int n = 8 + (int)(rng() % 300);
        std::vector<int8_t> st(H);
        std::vector<int32_t> cnt(H);
        std::vector<int64_t> cost(H);
        std::vector<double> med(H);
        for (int64_t i = 0; i < H; ++i) {
            st[i] = rng() % 9 == 0 ? 0 : 1;
            cnt[i] = st[i] ? (int32_t)(rng() % (n + 1)) : 0;
            cost[i] = st[i] ? (int64_t)(rng() % 64) + ((int64_t)(rng() % 3) << 32) : -1;  // many ties
            med[i] = st[i] ? (double)(rng() % 64) * 0.25 : -1.0;
            if (st[i] && rng() % 50 == 0) med[i] = std::numeric_limits<double>::quiet_NaN();
            if (st[i] && rng() % 50 == 0) med[i] = std::numeric_limits<double>::infinity();
        }
        if (trial % 5 == 0) st[rng() % H] = -1;
        const int max_iters = 1 + (int)(rng() % 3500);
        const double conf = trial % 2 ? 0.99 : 0.5;
        ScanState a, b;
        int64_t ca = -1, cb = -1;
        a.reset(max_iters);
        b.reset(max_iters);
        LmedsScan la, lb;
        la.reset(max_iters);
        lb.reset(max_iters);
        scan_step_msac(a, ca, cnt.data(), cost.data(), st.data(), H, n, 8, conf);
        scan_step_lmeds(la, st.data(), med.data(), H);
        for (int64_t i = 0; i < H;) {
            const int64_t c = std::min<int64_t>(H - i, 1 + rng() % 700);
            scan_step_msac(b, cb, cnt.data() + i, cost.data() + i, st.data() + i, c, n, 8, conf);
            scan_step_lmeds(lb, st.data() + i, med.data() + i, c);
            i += c;
        }
        CHECK(a.best == b.best && a.iter == b.iter && a.done == b.done && a.max_good == b.max_good && ca == cb &&
              a.niters == b.niters);
        CHECK(la.best == lb.best && la.done == lb.done && same(la.best_median, lb.best_median));
        // the literal loops
        int64_t best = -1, bc = -1, i = 0, niters = std::max(max_iters, 1);
        int32_t good = 0;
        for (; i < H && i < niters; ++i) {
            if (st[i] < 0) break;
            if (st[i] > 0 && cnt[i] > 7 && (best < 0 || cost[i] < bc)) {
                best = i;
                bc = cost[i];
                good = cnt[i];
                niters = update_num_iters(conf, (double)(n - good) / n, 8, (int)niters);
            }
        }
        CHECK(a.best == best && a.iter == i && ca == bc && a.max_good == good && a.niters == niters);
        int64_t lbest = -1;
        double bm = std::numeric_limits<double>::max();
        for (i = 0; i < H && i < std::max(max_iters, 1); ++i) {
            if (st[i] < 0) break;
            if (st[i] > 0 && med[i] < bm) {
                lbest = i;
                bm = med[i];
            }
        }
        CHECK(la.best == lbest && same(la.best_median, bm));
    }
    CHECK(lmeds_num_iters(0.99, 8, 2000) == 548);
    CHECK(lmeds_sigma(0.0, 9, 8) == 0.001 && lmeds_sigma(1.0, 9, 8) == 2.5 * 1.4826 * 6.0);
}

int main() {
    std::mt19937_64 rng(20240702);
    check_scores(rng);
    check_small_and_large();
    check_scans(rng);
    printf("fmrobust harness: %s (%d failed checks)\n", g_fail ? "FAILED" : "ok", g_fail);
    return g_fail ? 1 : 0;
}
