// TEST INFRASTRUCTURE (tests/sanitize): the host-only LMedS pieces of librsac (csrc/rsac_host.hip:
// hom_median_host -- the source k_hom_median runs --, scan_step_lmeds, lmeds_num_iters; rsac_math.h
// lmeds_*) under ASan + UBSan on the CPU.  A stand-alone program, built by lmeds.mk and run by hand
// (make -f lmeds.mk run); not a pytest test, never loaded into Python, never run on a GPU machine.
// Exit status 0 = every check passed (the sanitizers abort on a finding).  Checks:
//   1. medians over 100 000 points, some with inf / NaN coordinates, against std::nth_element on the
//      same keys, for several models (one with a pole through the data);
//   2. n = 1 .. 9, 4 and 5 among them, against a sorted copy;
//   3. the scan fed in chunks == fed at once, with status 0 / -1 and NaN medians.
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

static bool same(double a, double b) { return (a != a && b != b) || a == b; }

// the definition, by sorting: keys ascending, read back as f32
static double median_by_sort(const float *sx, const float *sy, const float *dx, const float *dy, int n,
                             const double *H) {
    float hf[8];
    for (int q = 0; q < 8; ++q) hf[q] = (float)H[q];
    std::vector<uint32_t> key((size_t)n);
    for (int i = 0; i < n; ++i) key[i] = lmeds_key(hom_err(hf, sx[i], sy[i], dx[i], dy[i]));
    std::sort(key.begin(), key.end());
    return lmeds_median(n > 1 ? key[n / 2 - 1] : 0, key[n / 2], n);
}

static void fill(std::mt19937_64 &rng, int n, std::vector<float> &soa, double bad_fraction) {
    std::uniform_real_distribution<float> U(0.f, 1000.f);
    std::uniform_real_distribution<double> B(0.0, 1.0);
    soa.assign((size_t)4 * n, 0.f);
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

static void check_medians(std::mt19937_64 &rng) {
    const double models[3][9] = {{1.1, 0, 3, 0, 0.9, -2, 0, 0, 1},
                                 {1.1, 0.001, 3, -0.002, 0.9, -2, 1e-6, -2e-6, 1},
                                 {1, 0, 0, 0, 1, 0, -1.0 / 512, 0, 1}};  // a pole at x = 512
    for (double bad : {0.0, 0.01, 0.3, 0.7}) {
        for (int n : {100000, 99999}) {
            std::vector<float> soa;
            fill(rng, n, soa, bad);
            if (bad == 0.0)
                for (int i = 0; i < 64; ++i) soa[(size_t)i * 1000] = 512.f;  // exactly on the pole
            const float *b = soa.data();
            for (const auto &H : models) {
                const double got = hom_median_host(b, b + n, b + 2 * n, b + 3 * n, n, H);
                CHECK(same(got, median_by_sort(b, b + n, b + 2 * n, b + 3 * n, n, H)));
                if (bad == 0.7) CHECK(!(got < 1.7976931348623157e308));  // inf or NaN: never wins
            }
        }
    }
}

static void check_small() {
    std::mt19937_64 rng(5);
    const double H[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int n = 1; n <= 9; ++n) {
        for (int trial = 0; trial < 50; ++trial) {
            std::vector<float> soa((size_t)4 * n, 0.f);
            for (int i = 0; i < n; ++i) soa[(size_t)2 * n + i] = (float)(rng() % 4);  // many duplicates
            if (trial % 7 == 0) soa[(size_t)2 * n] = std::numeric_limits<float>::quiet_NaN();
            const float *b = soa.data();
            CHECK(same(hom_median_host(b, b + n, b + 2 * n, b + 3 * n, n, H),
                       median_by_sort(b, b + n, b + 2 * n, b + 3 * n, n, H)));
        }
    }
    CHECK(lmeds_sigma(0.0, 5, 4) == 0.001);
    CHECK(lmeds_sigma(1.0, 5, 4) == 2.5 * 1.4826 * 6.0);
    CHECK(lmeds_num_iters(0.995, 4, 2000) == 55);
    CHECK(lmeds_num_iters(0.01, 4, 2000) == 3);
}

static void check_scan(std::mt19937_64 &rng) {
    for (int trial = 0; trial < 400; ++trial) {
        const int64_t H = 1 + rng() % 3000;
        std::vector<int8_t> st(H);
        std::vector<double> med(H);
        for (int64_t i = 0; i < H; ++i) {
            st[i] = rng() % 9 == 0 ? 0 : 1;
            med[i] = (double)(rng() % 64) / 4;
            if (rng() % 11 == 0) med[i] = std::numeric_limits<double>::quiet_NaN();
            if (st[i] == 0) med[i] = -1.0;
        }
        if (trial % 5 == 0) st[rng() % H] = -1;
        const int64_t niters = 1 + rng() % 3500;
        LmedsScan a, b;
        a.reset(niters);
        b.reset(niters);
        scan_step_lmeds(a, st.data(), med.data(), H);
        for (int64_t i = 0; i < H;) {
            const int64_t c = std::min<int64_t>(H - i, 1 + rng() % 700);
            scan_step_lmeds(b, st.data() + i, med.data() + i, c);
            i += c;
        }
        CHECK(a.best == b.best && a.iter == b.iter && a.done == b.done && a.best_median == b.best_median);
        // the literal loop
        int64_t best = -1, i = 0;
        double bm = 1.7976931348623157e308;
        for (; i < H && i < niters; ++i) {
            if (st[i] < 0) break;
            if (st[i] > 0 && med[i] < bm) {
                best = i;
                bm = med[i];
            }
        }
        CHECK(a.best == best && a.iter == i && a.best_median == bm);
    }
}

int main() {
    std::mt19937_64 rng(20240607);
    check_medians(rng);
    check_small();
    check_scan(rng);
    printf("lmeds harness: %s (%d failed checks)\n", g_fail ? "FAILED" : "ok", g_fail);
    return g_fail ? 1 : 0;
}
