// rsac_host.h -- host-side pieces of the RANSAC driver: the OpenCV MWC
// sampler (for sampler="opencv"), RANSACUpdateNumIters, the resumable
// sequential best-model scan, Rodrigues and the non-minimal refits.
//
// These run on the CPU because they are sequential by definition (the MWC
// stream, the "first strictly greater" scan) or tiny (refits on the inliers
// of one model).  Reference semantics: RANSACPointSetRegistrator::run /
// getSubset (OpenCV ptsetreg.cpp) behind cv2.solvePnPRansac
// (main_v1.py:497) and cv2.findHomography (main_v1.py:312); the refits play
// the role of cv2.solvePnPRefineLM (main_v1.py:508) and findHomography's
// LS + LM polish.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

namespace rsac {

// Run f(p) for p in [0, P) on up to 16 host threads (the per-problem MWC subset draws and refits
// of a batch are independent; each writes only its own outputs).  The workers are a persistent
// pool (rsac_host.hip: host_pool_run), created on first use, so a call costs a wake-up instead of
// 16 thread creations and joins (r06); a call made while the pool is busy (another thread's
// batch) runs on its own thread.  Sanitizer-checked by tests/sanitize (ThreadSanitizer).
void host_pool_run(int P, int nt, void (*fn)(void *, int), void *arg);
int host_pool_threads();

template <class F>
void parallel_for(int P, F f) {
    const int nt = std::min({host_pool_threads(), 16, (P + 7) / 8});
    if (nt <= 1) {
        for (int p = 0; p < P; ++p) f(p);
        return;
    }
    host_pool_run(P, nt, [](void *a, int p) { (*static_cast<F *>(a))(p); }, &f);
}

struct Mwc {
    uint64_t state = ~(uint64_t)0;
    uint32_t next() {
        state = (uint64_t)(uint32_t)state * 4164903690u + (state >> 32);
        return (uint32_t)state;
    }
    int uniform(int a, int b) { return a == b ? a : (int)(next() % (uint32_t)(b - a) + (uint32_t)a); }
};

// OpenCV getSubset sequence for H consecutive iterations of k-point samples (out: H x k);
// hom != nullptr applies HomographyEstimatorCallback::checkSubset (sx, sy, dx, dy SoA; k = 4).
void mwc_subsets(Mwc &rng, int n, int64_t H, const float *const *hom, int32_t *out, int8_t *status, int k = 4);

int update_num_iters(double p, double ep, int model_points, int max_iters);
// update_num_iters(p, (n - c) / n, ...) through a per-thread table of its pow and logs (the scan replays)
int update_num_iters_count(double p, int n, int c, int model_points, int max_iters);

struct ScanState {
    int64_t niters = 1;
    int64_t best = -1;
    int32_t max_good = 0;
    int64_t iter = 0;
    bool done = false;
    bool improved = false;  // set by scan_step(stop_on_improve) when it stopped at a new best
    void reset(int max_iters) {
        niters = max_iters > 1 ? max_iters : 1;
        best = -1; max_good = 0; iter = 0; done = false; improved = false;
    }
};

// consume hypotheses [s.iter, s.iter + count) (counts/status indexed from 0)
// stop_on_improve: return right after a new best (s.improved set, s.iter = its index + 1)
// rps: the records a sample owns (rsac_host.hip, above scan_step); 1 but for the 7-point fundamental matrix
void scan_step(ScanState &s, const int32_t *counts, const int8_t *status, int64_t count, int n, int model_points,
               double confidence, bool stop_on_improve = false, int rps = 1);

// The MSAC scan (RSAC_F_MSAC; DESIGN.md "MSAC scoring") beside scan_step, over (status, count,
// cost): status < 0 ends the scan; a hypothesis is eligible iff status > 0 and count >
// model_points - 1; an eligible one replaces the best iff its cost is strictly lower (the first
// eligible one always replaces "none"), and then max_good = its count and niters =
// RANSACUpdateNumIters(conf, (n - count) / n, model_points, niters).  best_cost travels beside s.
void scan_step_msac(ScanState &s, int64_t &best_cost, const int32_t *counts, const int64_t *costs,
                    const int8_t *status, int64_t count, int n, int model_points, double confidence, int rps = 1);

// count and MSAC cost of one pose over f32 SoA points: the source k_pnp_cost runs (rsac_math.h)
int64_t pnp_cost_host(const float *X, const float *Y, const float *Z, const float *U, const float *V, int n,
                      const double cam[4], const double *R, const double *t, float thr2, int32_t *count_out);
// count and MSAC cost of one homography (hf[q] = (float)H[q], q < 8) over f32 SoA points: the source
// k_hom_cost / k_hom_cost_lane run
int64_t hom_cost_host(const float *sx, const float *sy, const float *dx, const float *dy, int n, const double *H,
                      float thr2, int32_t *count_out);
int msac_shift_host(float thr2);

// LMedS (DESIGN.md "LMedS homography"): the scan over (status, median) in hypothesis order.
// status < 0 ends the scan, status == 0 is skipped, a hypothesis replaces the best iff its median
// is strictly below the best's in f64 (the best starts at DBL_MAX; ties keep the earlier index, a
// NaN never wins).  The iteration budget is fixed (no update while scanning).
struct LmedsScan {
    int64_t niters = 1;
    int64_t best = -1;
    int64_t iter = 0;
    bool done = false;
    double best_median = 1.7976931348623157e308;  // DBL_MAX
    void reset(int64_t n_iters) { *this = LmedsScan(); niters = n_iters > 1 ? n_iters : 1; }
};
void scan_step_lmeds(LmedsScan &s, const int8_t *status, const double *medians, int64_t count, int rps = 1);
// OpenCV's fixed LMedS iteration count, max(RANSACUpdateNumIters(conf, 0.45, model_points, max_iters), 3)
int lmeds_num_iters(double confidence, int model_points, int max_iters);
// the median of hom_err over f32 SoA points under H (hf[q] = (float)H[q], q < 8): the source
// k_hom_median runs (rsac_math.h lmeds_*); n >= 1
double hom_median_host(const float *sx, const float *sy, const float *dx, const float *dy, int n, const double *H);
// the median of pnp_err over f32 SoA points under (R, t) and cam (fx fy cx cy): the source the
// k_pnp_median* kernels run; n >= 1
double pnp_median_host(const float *X, const float *Y, const float *Z, const float *U, const float *V, int n,
                       const double cam[4], const double *R, const double *t);

// The fundamental matrix's robust scores over f32 SoA points under F (9 doubles): the source the
// k_fm_cost* / k_fm_median* kernels run (rsac_math.h fm_err, fm_msac_term, lmeds_*).
void fm_err_host(const float *x1, const float *y1, const float *x2, const float *y2, int n, const double *F,
                 float *err_out);
int64_t fm_cost_host(const float *x1, const float *y1, const float *x2, const float *y2, int n, const double *F,
                     float thr2, int32_t *count_out);
double fm_median_host(const float *x1, const float *y1, const float *x2, const float *y2, int n, const double *F);  // n >= 1

// the round [s.iter, s.iter + H) from its improvement records (rsac_internal.h ScanRecords:
// the strict prefix maxima above the scan's floor, idx / first_neg relative to the round's
// start): identical to scan_step over the full rows
void scan_records(ScanState &s, const int32_t *idx, const int32_t *cnt, int nrec, int32_t first_neg, int64_t H, int n,
                  int model_points, double confidence, bool stop_on_improve = false, int rps = 1);

void rodrigues_v2m(const double r[3], double R[9]);
void rodrigues_m2v(const double R[9], double r[3]);

// EPnP on the masked points (the final solve of solvePnPRansac with SOLVEPNP_P3P),
// bit-identical to k_pnp_epnp; false for < 4 inliers or a degenerate cloud.
bool pnp_epnp_host(const float *X, const float *Y, const float *Z, const float *U, const float *V, const uint8_t *mask,
                   int n, const double cam[4], double R[9], double t[3]);

// LM over (R, t) on masked correspondences (f32 SoA); returns iterations
int pnp_refine_lm(const float *X, const float *Y, const float *Z, const float *U, const float *V, const uint8_t *mask,
                  int n, const double cam[4], double R[9], double t[3], int max_iter);

// least-squares normalised DLT on the inliers + 10 LM iterations
bool hom_refine(const float *sx, const float *sy, const float *dx, const float *dy, const uint8_t *mask, int n,
                double H[9]);

}  // namespace rsac
