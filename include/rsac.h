/*
 * rsac.h -- C ABI of the MI355X RANSAC engine (librsac.so).
 *
 * Drop-in boundary for the reference's RANSAC hot path.  The reference calls
 * OpenCV through the cv2 Python binding:
 *
 *   cv2.solvePnPRansac(objectPoints, imagePoints, K, dist, iterationsCount,
 *                      reprojectionError, confidence) -> retval, rvec, tvec, inliers
 *        main_v1.py:497-502, testpro-K.py:72-75, testpro.py:536-541, test_pro.py:515-520
 *   cv2.findHomography(src, dst, cv2.RANSAC, ransacReprojThreshold) -> H, mask
 *        main_v1.py:312, process.py:200, test02.py:263, testpro.py:350, test_pro.py:351
 *   Python loop of findHomography over candidate locations
 *        main_v1.py:274-284 (find_homographies), process.py:147-185
 *   K sweep of solvePnPRansac over 27 intrinsics
 *        testpro-K.py:58-75 (estimate_camera_orientation)
 *
 * Each entry point below replaces one of those.  Plain pointers and sizes
 * only; the Python layer (rsac/, ctypes) mirrors the cv2 signatures on top.
 *
 * Conventions
 *   - returns RSAC_OK (model found), RSAC_NO_MODEL (retval=False in cv2
 *     terms), or a negative RSAC_E* code; rsac_last_error() gives the text
 *     (thread-local).
 *   - host inputs: float64, array-of-structs exactly as numpy holds them
 *     (points3d N x 3, points2d N x 2), converted to float32 like OpenCV does.
 *     With RSAC_F_DEVICE_IN the same layout lives in device memory.
 *     With RSAC_F_DEVICE_SOA the inputs are already device float32
 *     structure-of-arrays: pts3d = X[N] Y[N] Z[N], pts2d = U[N] V[N].
 *   - inlier masks are RANSAC-phase masks (uint8, one per point), as OpenCV
 *     returns them; host memory unless RSAC_F_DEVICE_OUT.
 *   - work is enqueued on `stream` (hipStream_t; NULL = the context stream, a blocking stream
 *     ordered with the device null stream, i.e. with torch's default stream);
 *     calls on one context are serialised; contexts are independent.
 */
#ifndef RSAC_H
#define RSAC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSAC_ABI_VERSION 2  /* 2: rsac_set_score_variant removed; rsac_pnp_hypotheses subset width follows RSAC_F_MINIMAL_EPNP5 */

#if defined(__GNUC__)
#define RSAC_EXPORT __attribute__((visibility("default")))
#else
#define RSAC_EXPORT
#endif

/* status codes */
#define RSAC_OK 0
#define RSAC_NO_MODEL 1
#define RSAC_MORE 2 /* rsac_pnp_ransac_first_round: the first round did not end the scan */
#define RSAC_EINVAL (-1)
#define RSAC_ETOOFEW (-2) /* fewer than 4 correspondences (cv2 raises) */
#define RSAC_EHIP (-3)
#define RSAC_ENOMEM (-4)
#define RSAC_ENODEV (-5)

/* flags */
#define RSAC_F_SAMPLER_OPENCV (1u << 0) /* OpenCV MWC getSubset sequence (host-generated) instead of Philox */
#define RSAC_F_ADAPTIVE (1u << 1)       /* RANSACUpdateNumIters early termination, evaluated in rounds */
#define RSAC_F_REFINE (1u << 2)         /* non-minimal refit on the inliers (LM) -> R,t / H */
#define RSAC_F_DEVICE_IN (1u << 3)      /* inputs are device pointers (float64 AoS) */
#define RSAC_F_DEVICE_SOA (1u << 4)     /* inputs are device float32 SoA (implies device) */
#define RSAC_F_DEVICE_OUT (1u << 5)     /* inlier mask output is a device pointer */
#define RSAC_F_EXACT_ONLY (1u << 6)     /* disable the float32 pre-filter in scoring (A/B and tests) */
#define RSAC_F_ASYNC (1u << 8)          /* rsac_pnp_evaluate_range: device outputs, no host wait (see there) */
#define RSAC_F_EPNP (1u << 9)           /* PnP: EPnP on the inliers as the final solve (what solvePnPRansac
                                           runs after a SOLVEPNP_P3P minimal kernel); with RSAC_F_REFINE,
                                           LM from the EPnP pose */
#define RSAC_F_MINIMAL_EPNP5 (1u << 10) /* PnP: 5-point samples solved by EPnP -- solvePnPRansac's default
                                           SOLVEPNP_ITERATIVE kernel, the one every reference call runs
                                           (main_v1.py:497, testpro-K.py:72 pass no flags;
                                           model_points = 5, also in
                                           RANSACUpdateNumIters); explicit subsets are then n x 5 */
#define RSAC_F_LO (1u << 7)             /* LO-RANSAC (PnP, one problem): local optimisation at every new best,
                                           BASELINE.json configs[4]; see DESIGN.md "LO-RANSAC" */
#define RSAC_F_RVEC_ROUNDTRIP (1u << 11) /* PnP: every minimal model's rotation goes through
                                           R' = Rodrigues(Rodrigues(R)) before it is scored, as
                                           OpenCV's PnPRansacCallback keeps (rvec, tvec) and
                                           computeError projects through Rodrigues(rvec)
                                           (main_v1.py:497, testpro-K.py:72); the deterministic
                                           Rodrigues of rsac_rodrigues_* */
#define RSAC_F_MSAC (1u << 12)          /* MSAC model selection -- the hypothesis with the lowest truncated
                                           cost wins instead of the highest inlier count (see "MSAC scoring"
                                           below; DESIGN.md "MSAC scoring", "MSAC scoring for homographies").
                                           Honoured by rsac_pnp_ransac and rsac_pnp_ransac_batched (there it
                                           implies RSAC_F_EXACT_ONLY; RSAC_EINVAL with active lens distortion)
                                           and by rsac_homography_ransac, rsac_homography_ransac_batched and
                                           rsac_location_search, and by rsac_fundamental_ransac (there it
                                           implies RSAC_F_EXACT_ONLY; DESIGN.md "MSAC and LMedS for the
                                           fundamental matrix"); RSAC_EINVAL with RSAC_F_LO or RSAC_F_ASYNC */
#define RSAC_F_POINTS_UNCHANGED (1u << 13) /* rsac_pnp_evaluate_range with RSAC_F_DEVICE_IN: the caller promises
                                           that the arrays at pts3d and pts2d hold the values they held at
                                           this context's previous call.  When that call was an
                                           rsac_pnp_evaluate_range with the same pointers, n, K, threshold,
                                           stream and input flags, and no other entry point of the context
                                           ran in between (rsac_pnp_winner excepted), the per-problem set-up
                                           (f32 conversion, MFMA point operands, bounds, frame) is not
                                           launched again.  Otherwise the flag is ignored; it is never an
                                           error.  The results are the same bits either way. */
#define RSAC_F_FM_7POINT (1u << 14)     /* fundamental matrix: 7-point samples, up to three models each (see
                                           "Seven-point fundamental matrix" below).  Accepted by
                                           rsac_fundamental_ransac (also with RSAC_F_MSAC, RSAC_F_REFINE,
                                           RSAC_F_EXACT_ONLY), rsac_fundamental_lmeds, their _batched forms and
                                           rsac_fundamental_hypotheses / _hypotheses_msac / _medians;
                                           RSAC_EINVAL everywhere else.  Without it every call is unchanged. */

typedef struct rsac_ctx rsac_ctx;

/* per-call diagnostics (all optional; without them no HIP timing events are recorded) */
typedef struct rsac_stats {
    int64_t best_hyp;      /* index of the winning hypothesis (-1 none) */
    int64_t iters;         /* RANSAC iterations consumed (OpenCV `iter` at exit) */
    int64_t hyps_scored;   /* hypotheses evaluated on the GPU (>= iters) */
    int32_t n_inliers;     /* RANSAC-phase inlier count of the winner */
    int32_t rounds;        /* launches of the solve+score pair */
    double gpu_ms;         /* device time of solve+score (events), summed over rounds */
    double solve_ms;       /* ... of which the sample+minimal-solve kernel */
    double score_ms;       /* ... of which the scoring kernel */
    int32_t lo_improvements; /* LO-RANSAC: refits that raised the best count */
    int32_t reserved;
} rsac_stats;

/* Timing of any PnP call on the context (batched ones included, which take no stats argument):
 * with rsac_set_timing(ctx, 1) every call records HIP events around its solve and scoring
 * launches on the call's stream, and rsac_last_stats returns the last call's rsac_stats
 * (gpu_ms / solve_ms / score_ms summed over its rounds).  Off by default (no events).
 * The homography calls (RANSAC and LMedS, batched ones included) leave their figures there too. */
RSAC_EXPORT int rsac_set_timing(rsac_ctx *ctx, int32_t on);
RSAC_EXPORT int rsac_last_stats(rsac_ctx *ctx, rsac_stats *out);

RSAC_EXPORT int rsac_create(int device, rsac_ctx **out);
RSAC_EXPORT void rsac_destroy(rsac_ctx *ctx);
RSAC_EXPORT const char *rsac_last_error(void);
RSAC_EXPORT int rsac_abi_version(void);
RSAC_EXPORT int rsac_device_count(void);
RSAC_EXPORT int rsac_set_round_size(rsac_ctx *ctx, int64_t hyps_per_round); /* adaptive round length (default 4096) */

/* The pose refit (solvePnPRefineLM, main_v1.py:508-509) of a problem above 4096 points runs
 * on several cooperating blocks that must be resident at once.  rsac_refit_blocks reports, for
 * an n-point problem, the ranges of its summation order (lm_blocks) and the blocks that share
 * them on this device (the co-resident limit; fewer blocks walk more ranges each, same order,
 * same bits).  The blocks wait on each other's sums (about 1 s at most): when other work keeps
 * some of them from being resident that long, the call is redone with one block per refit (no
 * co-residency needed, the same bits), so the caller always gets the refined pose. */
RSAC_EXPORT int rsac_refit_blocks(rsac_ctx *ctx, int32_t n, int32_t *ranges, int32_t *blocks);
/* Test hooks, not for production use.  RSAC_DBG_REFIT_MAX_BLOCKS: cap the refit's
 * cooperating blocks (0 = the device limit).  RSAC_DBG_REFIT_DROP_BLOCK (nonzero): launch one
 * block fewer than the ranges' stride, so one range's sums never arrive. */
#define RSAC_DBG_REFIT_MAX_BLOCKS 1
#define RSAC_DBG_REFIT_DROP_BLOCK 2
#define RSAC_DBG_MF_CELL_PTS 5 /* > 0: the MFMA scorer runs every tile by cells of this many points */
/* RSAC_DBG_SPEC_OVERFLOW (nonzero): the host's replay of a speculative first round treats it as
 * having more improvements than the device records (the restart-from-hypothesis-0 branch) */
#define RSAC_DBG_SPEC_OVERFLOW 6
/* RSAC_DBG_F64_SELFTEST: rsac_debug_set(ctx, RSAC_DBG_F64_SELFTEST, n) runs the fast f64 root /
 * division cores (rsac_math.h dsqrt_fast / ddiv_fast) and the Jacobi rotation's fast form against
 * the IEEE operators on the device, over n random operand sets inside their stated ranges plus the
 * range ends; rsac_debug_get(ctx, RSAC_DBG_F64_SELFTEST, &m) then gives the number of results that
 * differ in any bit (0 expected). */
#define RSAC_DBG_F64_SELFTEST 7
RSAC_EXPORT int rsac_debug_set(rsac_ctx *ctx, int32_t key, int64_t value);
/* RSAC_DBG_SPEC_FINISHES / RSAC_DBG_SPEC_REDOS (read only): rsac_pnp_ransac(_batched) calls whose
 * finish was enqueued behind the device's own pick of the winners, and those of them the host's
 * replay rejected (the finish then ran again on the host's winners). */
#define RSAC_DBG_SPEC_FINISHES 3
#define RSAC_DBG_SPEC_REDOS 4
/* RSAC_DBG_BOUND (set): rsac_pnp_evaluate_range's bounded scoring: 0 = by size (the default), 1 =
 * always where the problem allows it, 2 = never.  RSAC_DBG_BOUND_N1 / RSAC_DBG_BOUND_SURVIVORS
 * (read only): the points of pass 1 and the hypotheses pass 2 completed in the context's last
 * rsac_pnp_evaluate_range, read after its stream was synchronised (n and 0 for an unbounded call). */
#define RSAC_DBG_BOUND 8
#define RSAC_DBG_BOUND_N1 9
#define RSAC_DBG_BOUND_SURVIVORS 10
/* RSAC_DBG_LMEDS_KEYS (set): where LMedS PnP keeps the keys of problems past the block kernel's
 * register capacity (65536 points): 0 = device key rows within the default budget of 256 MiB,
 * hypotheses in chunks; > 0 = the same within this many bytes; < 0 = no rows, every counting pass
 * recomputes the keys.  The medians are the same bits either way. */
#define RSAC_DBG_LMEDS_KEYS 11
/* RSAC_DBG_HOM_FIT (set): where RSAC_F_REFINE of the homography drivers and of rsac_location_search
 * fits: 0 = by the measured policy (DESIGN.md "Homography: least-squares and LM refit and local
 * optimisation on GPU"), 1 = always the host tail, 2 = always the device fit.  The same bits
 * either way. */
#define RSAC_DBG_HOM_FIT 12
/* RSAC_DBG_SETUP_REUSED (read only): 1 when the context's last rsac_pnp_evaluate_range launched no
 * set-up (RSAC_F_POINTS_UNCHANGED on the same problem as the call before it), else 0. */
#define RSAC_DBG_SETUP_REUSED 13
/* RSAC_DBG_BOUND_HINTED (read only): 1 when the context's last rsac_pnp_evaluate_range ran the
 * hinted bounded sequence (pass 1 over the n1 that the previous call on the same problem left on
 * the device, the first hypotheses' whole pass inside its launch), else 0. */
#define RSAC_DBG_BOUND_HINTED 14
/* RSAC_DBG_BOUND_SLAB (set): pass 1 of the bounded sequence: 0 = the default (the one-coordinate
 * slab body where the pass is cut short: upper bounds of the counts, survivors recounted over every
 * point; not where the guard for low inlier ratios turns it down), 1 = the exact body (survivors
 * completed over the remaining points), 2 = the slab body wherever the pass is cut short, whatever
 * the guard decides.  The same key, model and mask in every mode.
 * RSAC_DBG_SLAB_SELFTEST: rsac_debug_set(ctx, RSAC_DBG_SLAB_SELFTEST, n) runs the slab body's
 * certain-outlier test against the scorer's decided-outlier test on n operand sets (random over the
 * record and point ranges, and the edges: zero and denormal depths, infinite bands, NaN, |q1| within
 * a few ulp of the bound); rsac_debug_get then gives the number of sets the slab calls a certain
 * outlier and the scorer's test does not call a decided outlier.  It must be 0. */
#define RSAC_DBG_BOUND_SLAB 15
#define RSAC_DBG_SLAB_SELFTEST 16
/* RSAC_DBG_BOUND_SLAB_RAN (read only): 1 when pass 1 of the context's last rsac_pnp_evaluate_range
 * ran the slab body (a bounded call whose pass 1 was cut short, with the slab built, not switched
 * off by RSAC_DBG_BOUND_SLAB and not turned down by the guard for low inlier ratios), else 0.
 * RSAC_DBG_BOUND_COUNT: rsac_debug_set(ctx, RSAC_DBG_BOUND_COUNT, j) selects a hypothesis of the
 * range; rsac_debug_get then copies the count word the last bounded call left for it from the device
 * (the exact count of a hypothesis of the first 256 or of a listed one, pass 1's figure otherwise).
 * Both read after the call's stream was synchronised. */
#define RSAC_DBG_BOUND_SLAB_RAN 17
#define RSAC_DBG_BOUND_COUNT 18
/* RSAC_DBG_BOUND_P2_MIN (set): the shortest share of the bounded sequence's pass 2 in block passes
 * of 256 points (0 = as built).  A value above the block passes of a tile makes every share run over
 * several tiles, and above 64 makes its segments end at the recount window.  The same results for
 * every value. */
#define RSAC_DBG_BOUND_P2_MIN 19
RSAC_EXPORT int rsac_debug_get(rsac_ctx *ctx, int32_t key, int64_t *value);
/* The index maps the bounded sequence's kernels run (no device needed).  what = 0, the packed slab
 * operand: in = {group, row, lane half, accumulator, hypothesis of the tile}, out = {the row's
 * hypothesis, its component (0 xs, 1 z'), the accumulator's hypothesis, its component, the
 * hypothesis's counter slot, its lane half}.  what = 1, pass 2's shares: in = {tiles, points,
 * grid, shares per block, shortest share} (the last two: 0 = as built), out = {block passes per
 * tile, per share, shares}.  what = 2: in = the same + {share, position in the line}, out = {tile,
 * first block pass in the tile, length} of the segment that starts there.  what = 3: out = {shares
 * per block as built (0: the cell rule), shortest share, longest segment, slab operands packed}. */
RSAC_EXPORT int rsac_bound_layout(int32_t what, const int32_t *in, int32_t *out);

/* cv2.solvePnPRansac (main_v1.py:497).  K: 3x3 row-major f64.  Minimal
 * solver: P3P (Lambda Twist) on 4 points.  n_iters = iterationsCount cap,
 * reproj_thresh in px, confidence as in OpenCV.  Outputs R (3x3 row-major),
 * t (3), mask (n). */
RSAC_EXPORT int rsac_pnp_ransac(rsac_ctx *ctx, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                    int32_t n_iters, double reproj_thresh, double confidence, uint64_t seed, uint32_t flags,
                    double R_out[9], double t_out[3], uint8_t *inlier_mask_out, rsac_stats *stats, void *stream);

/* Batched PnP: P independent problems, problem p owns points
 * [offsets[p], offsets[p+1]) and intrinsics K[9p..9p+8] (the K sweep of
 * testpro-K.py:58 is P problems sharing points; pass repeated rows).
 * Outputs per problem: R (9), t (3), status (RSAC_OK/RSAC_NO_MODEL),
 * n_inliers, mask (total points). */
RSAC_EXPORT int rsac_pnp_ransac_batched(rsac_ctx *ctx, const void *pts3d, const void *pts2d, const int64_t *offsets,
                            int32_t n_problems, const double *K, int32_t n_iters, double reproj_thresh,
                            double confidence, uint64_t seed, uint32_t flags, double *R_out, double *t_out,
                            int32_t *status_out, int32_t *n_inliers_out, uint8_t *inlier_mask_out, void *stream);

/* rsac_pnp_ransac_batched with the per-problem results written as f64 rows (ok 0/1, n_inliers,
 * R 9 row-major, t 3) into rows_out, a DEVICE buffer of n_problems x 14 doubles, by a kernel
 * reading the winners' records where they already are: the rows of a rank's problem chunk go to
 * the multi-GPU all-gather without passing through host arrays (rsac/parallel.py
 * pnp_batched_rows).  Returns with the stream synchronised. */
RSAC_EXPORT int rsac_pnp_ransac_batched_rows(rsac_ctx *ctx, const void *pts3d, const void *pts2d,
                                             const int64_t *offsets, int32_t n_problems, const double *K,
                                             int32_t n_iters, double reproj_thresh, double confidence, uint64_t seed,
                                             uint32_t flags, double *rows_out, uint8_t *inlier_mask_out,
                                             void *stream);

/* cv2.findHomography(src, dst, cv2.RANSAC, thr) (main_v1.py:312):
 * src, dst N x 2.  Defaults of OpenCV: max_iters 2000, confidence 0.995. */
RSAC_EXPORT int rsac_homography_ransac(rsac_ctx *ctx, const void *src, const void *dst, int32_t n, int32_t max_iters,
                           double thresh, double confidence, uint64_t seed, uint32_t flags, double H_out[9],
                           uint8_t *mask_out, rsac_stats *stats, void *stream);

/* The location-search loop of find_homographies (main_v1.py:274-284) as one
 * call: P problems with point ranges given by offsets. */
RSAC_EXPORT int rsac_homography_ransac_batched(rsac_ctx *ctx, const void *src, const void *dst, const int64_t *offsets,
                                   int32_t n_problems, int32_t max_iters, double thresh, double confidence,
                                   uint64_t seed, uint32_t flags, double *H_out, int32_t *status_out,
                                   int32_t *n_inliers_out, uint8_t *mask_out, void *stream);

/* The camera-location search of find_homographies / find_homography
 * (main_v1.py:254-348, 419; driver main_v1.py:862-866) as one call.
 * For every candidate location l (locations: L x 3 f64) and every feature i
 * noted on the image (pixels[i] != (0,0), main_v1.py:304):
 *   pos2 = (dz/dx, dy/dx) of pos3d[i] - loc[l]              (main_v1.py:305-308)
 *   H, mask = findHomography(pos2, pixels, RANSAC, thr)     (main_v1.py:312)
 *   err1 = sum_{mask} |pixel - H pos2|,  err2 = sum_{mask} |pos2 - H^-1 pixel|
 *          + (#outliers) * thr                              (main_v1.py:332-348, 419)
 * Host f64 arrays (pos3d n x 3, pixels n x 2).  Outputs: err_out L x 2
 * (err1, err2; (0, 0) where no model, which the driver maps to 1e6), and
 * optionally H_out L x 9 (findHomography's H = inv(M) of main_v1.py:314),
 * status_out L, n_inliers_out L, mask_out L x n_good (RANSAC-phase),
 * n_good_out.  flags: as rsac_homography_ransac (OpenCV sampler + adaptive +
 * refine reproduce cv2.findHomography). */
RSAC_EXPORT int rsac_location_search(rsac_ctx *ctx, const double *pos3d, const double *pixels, int32_t n,
                                     const double *locations, int32_t n_locations, double thresh, int32_t max_iters,
                                     double confidence, uint32_t flags, double *H_out, double *err_out,
                                     int32_t *status_out, int32_t *n_inliers_out, uint8_t *mask_out,
                                     int32_t *n_good_out, void *stream);

/* Fundamental-matrix RANSAC (BASELINE.json configs[3]; the reference has no
 * implementation -- SURVEY.md §8d -- so DESIGN.md "Fundamental matrix" defines it):
 * 8-point samples (Philox), normalised 8-point DLT + rank 2, Sampson test
 * r^2 <= thr^2 (a^2 + b^2 + a'^2 + b'^2) in f64, adaptive RANSACUpdateNumIters with
 * 8 model points.  pts1, pts2: N x 2 (x2^T F x1 = 0).  Flags: ADAPTIVE, DEVICE_IN,
 * DEVICE_SOA, DEVICE_OUT, EXACT_ONLY. */
RSAC_EXPORT int rsac_fundamental_ransac(rsac_ctx *ctx, const void *pts1, const void *pts2, int32_t n, int32_t max_iters,
                                        double thresh, double confidence, uint64_t seed, uint32_t flags,
                                        double F_out[9], uint8_t *mask_out, rsac_stats *stats, void *stream);
/* per-hypothesis probe (status, counts, models) of the fundamental-matrix path */
RSAC_EXPORT int rsac_fundamental_hypotheses(rsac_ctx *ctx, const void *pts1, const void *pts2, int32_t n,
                                            int64_t hyp_begin, int32_t n_hyps, double thresh, uint64_t seed,
                                            uint32_t flags, int32_t *counts_out, int8_t *status_out,
                                            double *models_out, void *stream);

/* The winner of a sharded run, re-derived on every rank without a host round trip
 * ("the winning model is re-derivable from hyp_idx on every rank"):
 * key = device pointer to the all-reduced packed key (count << 32 | ~index; 0 = none);
 * pts3d / pts2d = device f64 AoS; writes the hypothesis' R 9, t 3 to model_out
 * (device, 12 doubles; zeros for key 0) and its RANSAC-test mask to mask_out (device,
 * n bytes, optional).  Asynchronous on `stream`. */
RSAC_EXPORT int rsac_pnp_winner(rsac_ctx *ctx, const double *pts3d, const double *pts2d, int32_t n, const double K[9],
                                double thresh, uint64_t seed, const int64_t *key, double *model_out,
                                uint8_t *mask_out, void *stream);

/* GeoCoordTransformer (main_v1.py:36-57, pyproj EPSG:4326 <-> EPSG:326zz/327zz):
 * inverse != 0: (easting, northing) -> (lon, lat) degrees; inverse == 0: the reverse.
 * in, out: n x 2 f64 (host, or device with RSAC_F_DEVICE_IN: enqueued on `stream`, no wait).
 * Krueger's series to 6th order (DESIGN.md "DEM ray march"). */
RSAC_EXPORT int rsac_utm_convert(rsac_ctx *ctx, int inverse, const double *in, int64_t n, int32_t zone, int32_t south,
                                 uint32_t flags, double *out, void *stream);

/* ray_intersect_dem (main_v1.py:635-656) for n_rays rays at once: from origins[i] (UTM
 * easting, northing, height) march along dirs[i] in `step` m steps, int(max_search_dist /
 * step) times; a ray hits at the first position, from step index min_steps (150 in the
 * reference) on, not above the DEM.  The DEM is the reference's RegularGridInterpolator over
 * (lat, lon): dem ny x nx f64 row-major, lat_i = i * dy + y0, lon_j = j * dx + x0 (GDAL
 * geotransform: y0 = gt[3], dy = gt[5], x0 = gt[0], dx = gt[1]); each step's UTM position is
 * converted with the zone's inverse projection.  Outputs: hits_out n x 3 (NaN without a hit), status_out n:
 * 0 hit, 1 no hit within the distance (None), 2 left the DEM (the reference's caught
 * interpolation error, None).  Host arrays, or device with RSAC_F_DEVICE_IN (all of them; the
 * call then only enqueues on `stream` and returns without waiting). */
RSAC_EXPORT int rsac_dem_ray_intersect(rsac_ctx *ctx, const double *origins, const double *dirs, int32_t n_rays,
                                       const double *dem, int32_t ny, int32_t nx, double y0, double dy, double x0,
                                       double dx, int32_t zone, int32_t south, double max_search_dist, double step,
                                       int32_t min_steps, uint32_t flags, double *hits_out, int8_t *status_out,
                                       void *stream);

/* Minimal slice: inlier counts of given poses (H x [R 9, t 3] f64, host)
 * under the reprojection test of PnPRansacCallback::computeError. */
RSAC_EXPORT int rsac_score_poses(rsac_ctx *ctx, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                     const double *poses, int32_t n_poses, double reproj_thresh, uint32_t flags, int32_t *counts_out,
                     void *stream);

/* Hypothesis-range evaluation for sharding one problem over ranks
 * (SURVEY.md §8e): evaluates hypotheses [hyp_begin, hyp_begin + n_hyps) of
 * the Philox stream and returns the packed key
 * (count << 32) | (0xFFFFFFFF - low32(global index)) of the best one (lowest
 * index among ties), that hypothesis' model (R, t) and, if mask_out is
 * given, its RANSAC-phase mask (device pointer with RSAC_F_DEVICE_OUT).
 * Ranks all-reduce(MAX) the key.
 * Only the best key leaves the call, so on large ranges the scoring is bounded: hypotheses that
 * can no longer reach the best count found so far are not counted to the end (same key, model
 * and mask; DESIGN.md "Bounded scoring").
 * RSAC_F_ASYNC: key_out (one int64, the raw packed key, 0 = no model) and model_out
 * (12 doubles) are DEVICE pointers, mask_out must be a device pointer too; the call only
 * enqueues work on `stream` and returns RSAC_OK without waiting (no stats). */
RSAC_EXPORT int rsac_pnp_evaluate_range(rsac_ctx *ctx, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                            int64_t hyp_begin, int64_t n_hyps, double reproj_thresh, uint64_t seed, uint32_t flags,
                            int64_t *key_out, double model_out[12], uint8_t *mask_out, rsac_stats *stats,
                            void *stream);

/* Raw hot-path outputs for hypotheses [hyp_begin, hyp_begin + n_hyps) of
 * one problem: per-hypothesis status (1 model, 0 solver failed, -1 no
 * subset), inlier count and model (16 f64: R 9, t 3 | H 9; then valid.  PnP
 * records leave valid to the status byte on the device: host outputs get it
 * filled in, RSAC_F_DEVICE_OUT outputs carry an unspecified slot 12).
 * subsets (host int32 n_hyps x 4, or x 5 with RSAC_F_MINIMAL_EPNP5; optional) replaces the Philox draw, e.g.
 * with OpenCV's MWC sequence.  This is what the parity tests compare with
 * the CPU restatement hypothesis by hypothesis. */
RSAC_EXPORT int rsac_pnp_hypotheses(rsac_ctx *ctx, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                                    int64_t hyp_begin, int32_t n_hyps, double reproj_thresh, uint64_t seed,
                                    uint32_t flags, const int32_t *subsets, int32_t *counts_out, int8_t *status_out,
                                    double *models_out, void *stream);
RSAC_EXPORT int rsac_homography_hypotheses(rsac_ctx *ctx, const void *src, const void *dst, int32_t n,
                                           int64_t hyp_begin, int32_t n_hyps, double thresh, uint64_t seed,
                                           uint32_t flags, const int32_t *subsets, int32_t *counts_out,
                                           int8_t *status_out, double *models_out, void *stream);

/* Mask of a given pose under the RANSAC test (used after a sharded run). */
RSAC_EXPORT int rsac_pnp_mask(rsac_ctx *ctx, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                  const double model[12], double reproj_thresh, uint32_t flags, uint8_t *mask_out,
                  int32_t *count_out, void *stream);

/* cv2.solvePnP(..., flags=SOLVEPNP_EPNP) on the masked points (mask NULL = all), the
 * final solve cv2.solvePnPRansac runs on its inliers when the minimal solver is P3P
 * (flags=SOLVEPNP_P3P).  Host arrays; the same computation as the device
 * pass of RSAC_F_EPNP, bit for bit.  Returns RSAC_NO_MODEL for < 4 points or a degenerate
 * (planar) cloud.  The frame's centre follows the refit's rule (rsac_pnp_refine, below). */
RSAC_EXPORT int rsac_pnp_epnp(const double *pts3d, const double *pts2d, int32_t n, const double K[9],
                              const uint8_t *mask, double R_out[9], double t_out[3]);

/* The minimal solver of cv2.solvePnPRansac's default flags on one 5-point sample, on the host
 * (no GPU needed): solvePnP(..., SOLVEPNP_EPNP) in OpenCV's operation sequence (undistortPoints
 * to f32 normalised points, epnp.cpp with lapack.cpp's JacobiSVD; rsac_cvepnp.h, the source the
 * k_cvepnp5_* kernels run, the 12 x 12 JacobiSVD there on six lanes).  pts3d 5 x 3 and pts2d
 * 5 x 2 f64 AoS, rounded to f32 like solvePnPRansac's CV_32F copies (main_v1.py:497,
 * testpro-K.py:72).  Always RSAC_OK (OpenCV's EPnP reports a pose for any sample; a degenerate
 * one gives NaN). */
RSAC_EXPORT int rsac_pnp_epnp_minimal(const double *pts3d, const double *pts2d, const double K[9], double R_out[9],
                                      double t_out[3]);

/* Host-side non-minimal fits (no GPU needed), f64 AoS host inputs rounded
 * to f32 like the RANSAC path.  mask may be NULL (= all points).
 * rsac_pnp_refine: LM on (R, t) in place, cv2.solvePnPRefineLM
 *   (main_v1.py:508, testpro-K.py:122); returns iterations used.
 *   The pose is refined in a frame centred on point 0 when its three f32 coordinates are
 *   finite (masked or not), else on the lowest masked index (point 0 again when the mask is
 *   empty): a NaN / inf first point that the mask leaves out does not reach the pose.  The
 *   same rule holds for rsac_pnp_epnp, rsac_pnp_refine_lm and every final solve of the
 *   RANSAC, LO-RANSAC and LMedS entries (RSAC_F_REFINE, RSAC_F_EPNP).
 * rsac_homography_fit: normalised least-squares DLT + 10 LM iterations,
 *   findHomography's method-0 / final polish (main_v1.py:312). */
RSAC_EXPORT int rsac_pnp_refine(const double *pts3d, const double *pts2d, int32_t n, const double K[9],
                                const uint8_t *mask, double R[9], double t[3], int32_t max_iter);
RSAC_EXPORT int rsac_homography_fit(const double *src, const double *dst, int32_t n, const uint8_t *mask,
                                    double H_out[9]);

/* cv2.solvePnPRefineLM (main_v1.py:508-509, testpro-K.py:122-125) on the device: LM on (R, t)
 * in place from the given start over the masked points (mask NULL = all); host f64 AoS inputs,
 * rounded to f32 like the RANSAC path.  The same bits as rsac_pnp_refine (host). */
RSAC_EXPORT int rsac_pnp_refine_lm(rsac_ctx *ctx, const double *pts3d, const double *pts2d, int32_t n,
                                   const double K[9], const uint8_t *mask, double R[9], double t[3], void *stream);

/* compute_reprojection_error (testpro-K.py:32-36) = cv2.projectPoints (testpro-K.py:33, zero
 * distortion) + the per-point L2 norm of the pixel residual, in f64 on the f64 inputs:
 * proj_out n x 2 (optional), err_out n (optional).  Host arrays, or (RSAC_F_DEVICE_IN) device
 * arrays for inputs and outputs alike, then only enqueued on `stream`. */
RSAC_EXPORT int rsac_pnp_reprojection_errors(rsac_ctx *ctx, const double *pts3d, const double *pts2d, int32_t n,
                                             const double K[9], const double R[9], const double t[3],
                                             uint32_t flags, double *proj_out, double *err_out, void *stream);

/* estimate_camera_orientation (testpro-K.py:39-125) in one call: solvePnPRansac of the points
 * under each of the n_k intrinsics Ks (n_k x 9, the loop of :58-75, one batched launch
 * sequence; flags as rsac_pnp_ransac_batched: the final solve is RSAC_F_REFINE / RSAC_F_EPNP),
 * the gate "success and >= min_inliers inliers" (:77, 6 in the reference), the mean inlier
 * reprojection error of every K on the device (:80-82, through the pose's rvec as projectPoints
 * sees it), the first K with the strictly smallest mean (:90-97), then solvePnPRefineLM of that
 * K's pose on its inliers (:122-125).  Host f64 arrays.  Outputs: *best_out (-1: every K failed,
 * RSAC_NO_MODEL), and optionally per K mean_err_out (NaN where gated), models_out (R 9, t 3 of
 * solvePnPRansac), status_out (RSAC_OK = passed the gate), n_inliers_out, masks_out (n_k x n);
 * R_out / t_out the refined pose of the winner. */
RSAC_EXPORT int rsac_pnp_orientation_sweep(rsac_ctx *ctx, const double *pts3d, const double *pts2d, int32_t n,
                                           const double *Ks, int32_t n_k, int32_t n_iters, double reproj_thresh,
                                           double confidence, uint64_t seed, uint32_t flags, int32_t min_inliers,
                                           int32_t *best_out, double *mean_err_out, double *models_out,
                                           int32_t *status_out, int32_t *n_inliers_out, uint8_t *masks_out,
                                           double R_out[9], double t_out[3], void *stream);

/* Rodrigues (cv2.Rodrigues, main_v1.py:895): vector <-> matrix in cvRodrigues2's operation
 * sequence (range check, R = U V^T through lapack.cpp's JacobiSVD, the theta ~ pi branch;
 * c I + c1 r r^T + s [r]x element by element); acos / sin / cos are series polynomials (~1 ulp),
 * so the bits are the device's and the oracle's, not libm's. */
RSAC_EXPORT void rsac_rodrigues_v2m(const double r[3], double R[9]);
RSAC_EXPORT void rsac_rodrigues_m2v(const double R[9], double r[3]);

/* RANSACUpdateNumIters (OpenCV ptsetreg.cpp) */
RSAC_EXPORT int rsac_update_num_iters(double p, double ep, int model_points, int max_iters);

/* The sequential best-model scan of OpenCV's RANSAC loop (ptsetreg.cpp run(): "count >
 * max(maxGoodCount, modelPoints - 1)" replaces the best, then RANSACUpdateNumIters), over
 * per-hypothesis (status, count) in hypothesis order.  rsac_pnp_ransac runs it internally;
 * it is exported for drivers that produce the counts elsewhere, e.g. the multi-GPU loop of
 * rsac/parallel.py, which gathers each round's counts from every rank and scans them
 * identically everywhere.  Host-only, no device work. */
typedef struct rsac_scan_state {
    int64_t niters;   /* current iteration budget (starts at max_iters) */
    int64_t best;     /* index of the best hypothesis so far, -1 = none */
    int64_t iter;     /* hypotheses consumed */
    int32_t max_good; /* inliers of the best */
    int32_t done;     /* budget reached or sampler exhausted */
} rsac_scan_state;
RSAC_EXPORT void rsac_scan_init(rsac_scan_state *st, int32_t max_iters);
/* consume hypotheses [st->iter, st->iter + count); status < 0 = sampler gave up (ends the scan) */
RSAC_EXPORT int rsac_scan(rsac_scan_state *st, const int32_t *counts, const int8_t *status, int64_t count, int32_t n,
                          int32_t model_points, double confidence);
/* LO-RANSAC drivers: as rsac_scan, but return right after a new best (*improved = 1,
 * st->iter = its index + 1) so that it can be optimised locally before the scan goes on */
RSAC_EXPORT int rsac_scan_until_best(rsac_scan_state *st, const int32_t *counts, const int8_t *status, int64_t count,
                                     int32_t n, int32_t model_points, double confidence, int32_t *improved);
/* apply a locally optimised inlier count: raises max_good and lowers the iteration bound */
RSAC_EXPORT int rsac_scan_raise(rsac_scan_state *st, int32_t count, int32_t n, int32_t model_points, double confidence);

/* The multi-GPU adaptive loop's exchange format and scan (rsac/parallel.py):
 * rsac_pnp_hypothesis_rows evaluates Philox hypotheses [hyp_begin, hyp_begin + n_hyps) of one
 * problem and writes {status, count} int32 pairs into rows_out (DEVICE, n_hyps x 2), enqueued on
 * `stream` without waiting; ranks all-gather their rows into one device buffer (RCCL).
 * rsac_scan_device consumes such rows (device, count x 2) as rsac_scan / rsac_scan_until_best
 * would (stop_on_improve: return after a new best, *improved = 1): the improvements are listed on
 * the device and only they reach the host, where the iteration bound is applied. */
/* The sharded adaptive loop's first round (rsac/parallel.py sharded_ransac):
 * rsac_pnp_ransac of one problem (RSAC_F_ADAPTIVE, Philox sampler; RSAC_F_LO allowed) capped at
 * its first round, the 256 hypotheses rsac_pnp_ransac starts with.  Every rank runs it
 * redundantly, with no collective: most scans end inside that round (C2, C5).
 *   - The round ended the scan: the call IS rsac_pnp_ransac (R, t, mask, refit as there; the
 *     device's speculative finish, one synchronisation) and returns RSAC_OK / RSAC_NO_MODEL,
 *     with *st_out the final scan state (done = 1).
 *   - Otherwise it returns RSAC_MORE: *st_out is the scan state after the round (iter = its
 *     length, done = 0), R_out / t_out the best model so far (LO: the locally optimised one),
 *     mask_out undefined; the caller continues the scan from st_out->iter (sharded rounds).
 * stats (optional) as rsac_pnp_ransac. */
RSAC_EXPORT int rsac_pnp_ransac_first_round(rsac_ctx *ctx, const void *pts3d, const void *pts2d, int32_t n,
                                            const double K[9], int32_t n_iters, double reproj_thresh,
                                            double confidence, uint64_t seed, uint32_t flags, double R_out[9],
                                            double t_out[3], uint8_t *mask_out, rsac_scan_state *st_out,
                                            rsac_stats *stats, void *stream);
RSAC_EXPORT int rsac_pnp_hypothesis_rows(rsac_ctx *ctx, const void *pts3d, const void *pts2d, int32_t n,
                                         const double K[9], int64_t hyp_begin, int32_t n_hyps, double reproj_thresh,
                                         uint64_t seed, uint32_t flags, int32_t *rows_out, void *stream);
RSAC_EXPORT int rsac_scan_device(rsac_ctx *ctx, rsac_scan_state *st, const int32_t *rows, int64_t count, int32_t n,
                                 int32_t model_points, double confidence, int32_t stop_on_improve,
                                 int32_t *improved, void *stream);

/* One LO-RANSAC local optimisation (RSAC_F_LO's step) of a pose on the device: up to 4
 * rounds of LM refit on the current RANSAC inliers + recount, kept while the count rises.
 * model_in / model_out: R 9 row-major, t 3.  *count_out = the final inlier count (>= the
 * model's own count), *steps_out = refits that raised it.  flags: RSAC_F_DEVICE_IN. */
RSAC_EXPORT int rsac_pnp_local_opt(rsac_ctx *ctx, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                                   const double model_in[12], double thresh, uint32_t flags, double model_out[12],
                                   int32_t *count_out, int32_t *steps_out, void *stream);

/* Lens distortion (DESIGN.md "Lens distortion").  dist: host f64, n_dist coefficients in OpenCV's
 * order (k1, k2, p1, p2[, k3[, k4, k5, k6]]); n_dist = 4, 5 or 8 (8 adds the rational factor, even
 * when k4..k6 are zero); 12 and 14 (thin prism, tilt) return RSAC_EINVAL.  dist NULL, n_dist 0 or
 * all-zero coefficients: the call IS its pinhole twin, bit for bit.
 * Every point is undistorted once (cvUndistortPoints' five rounds) into an ideal pixel; the minimal
 * solvers and the final solve (RSAC_F_REFINE / RSAC_F_EPNP) run unchanged on the ideal pixels, and
 * the RANSAC test, the counts and the masks compare the raw pixels with cvProjectPoints2's
 * distorted projection, all f64 (RSAC_F_EXACT_ONLY is implied).
 * rsac_pnp_ransac_dist: rsac_pnp_ransac with (dist, n_dist); flags SAMPLER_OPENCV, ADAPTIVE, REFINE,
 * EPNP, MINIMAL_EPNP5, RVEC_ROUNDTRIP, DEVICE_IN, DEVICE_OUT, EXACT_ONLY; RSAC_F_LO,
 * RSAC_F_DEVICE_SOA and RSAC_F_ASYNC return RSAC_EINVAL.  The others extend their twins the same way. */
RSAC_EXPORT int rsac_pnp_ransac_dist(rsac_ctx *ctx, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                                     const double *dist, int32_t n_dist, int32_t n_iters, double reproj_thresh,
                                     double confidence, uint64_t seed, uint32_t flags, double R_out[9],
                                     double t_out[3], uint8_t *inlier_mask_out, rsac_stats *stats, void *stream);
RSAC_EXPORT int rsac_pnp_hypotheses_dist(rsac_ctx *ctx, const void *pts3d, const void *pts2d, int32_t n,
                                         const double K[9], const double *dist, int32_t n_dist, int64_t hyp_begin,
                                         int32_t n_hyps, double reproj_thresh, uint64_t seed, uint32_t flags,
                                         const int32_t *subsets, int32_t *counts_out, int8_t *status_out,
                                         double *models_out, void *stream);
RSAC_EXPORT int rsac_score_poses_dist(rsac_ctx *ctx, const void *pts3d, const void *pts2d, int32_t n,
                                      const double K[9], const double *dist, int32_t n_dist, const double *poses,
                                      int32_t n_poses, double reproj_thresh, uint32_t flags, int32_t *counts_out,
                                      void *stream);
RSAC_EXPORT int rsac_pnp_mask_dist(rsac_ctx *ctx, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                                   const double *dist, int32_t n_dist, const double model[12], double reproj_thresh,
                                   uint32_t flags, uint8_t *mask_out, int32_t *count_out, void *stream);
/* cv2.projectPoints with distortion + the per-point L2 norm, f64 on the f64 inputs (no rounding) */
RSAC_EXPORT int rsac_pnp_reprojection_errors_dist(rsac_ctx *ctx, const double *pts3d, const double *pts2d, int32_t n,
                                                  const double K[9], const double *dist, int32_t n_dist,
                                                  const double R[9], const double t[3], uint32_t flags,
                                                  double *proj_out, double *err_out, void *stream);
/* cv2.undistortPoints' iteration on the f32-rounded pixels (host, no GPU needed): norm_out n x 2 f64
 * normalised points, ideal_out n x 2 f32 ideal pixels (x fx + cx, y fy + cy); either may be NULL.
 * rsac_undistort_points_device: the same bits from the kernel; host arrays, or (RSAC_F_DEVICE_IN)
 * device arrays for the input and the outputs alike, then only enqueued on `stream`. */
RSAC_EXPORT int rsac_undistort_points(const double *pts2d, int32_t n, const double K[9], const double *dist,
                                      int32_t n_dist, double *norm_out, float *ideal_out);
RSAC_EXPORT int rsac_undistort_points_device(rsac_ctx *ctx, const double *pts2d, int32_t n, const double K[9],
                                             const double *dist, int32_t n_dist, uint32_t flags, double *norm_out,
                                             float *ideal_out, void *stream);
/* cv2.projectPoints with distortion on the host (no GPU needed), f64: proj_out n x 2 */
RSAC_EXPORT int rsac_project_points_dist(const double *pts3d, int32_t n, const double K[9], const double *dist,
                                         int32_t n_dist, const double R[9], const double t[3], double *proj_out);

/* MSAC scoring (RSAC_F_MSAC; DESIGN.md "MSAC scoring").  With e the f32 squared reprojection error of
 * the RANSAC test and thr2 = (float)(thresh * thresh): k = 19 - ilogb(thr2), q(e) = (uint32) floor(e 2^k),
 * Q = q(thr2) in [2^19, 2^20).  A point with e <= thr2 costs q(e), every other point (a NaN error
 * included) Q; a hypothesis' cost is the int64 sum over the problem's points, in units of 2^-k px^2,
 * exact and independent of the summation order; a hypothesis without a model has count 0, cost -1.
 * Among the hypotheses with a model and more than model_points - 1 inliers, scanned in index order
 * within the iteration bound, the one with the strictly lowest cost wins (ties keep the earlier
 * index); each new winner's count updates the bound through RANSACUpdateNumIters, which never
 * raises it.  The finish (mask, RSAC_F_REFINE / RSAC_F_EPNP) is that of the count rule on the
 * winner.  The threshold must be finite and positive.
 * rsac_last_costs: the winners' costs of the context's last RSAC_F_MSAC call (-1: no model, or
 * a problem of the count == model_points branch); n_problems must be that call's. */
RSAC_EXPORT int rsac_last_costs(rsac_ctx *ctx, int64_t *costs_out, int32_t n_problems);
/* rsac_pnp_hypotheses / rsac_score_poses with the all-f64 test and the per-hypothesis costs */
RSAC_EXPORT int rsac_pnp_hypotheses_msac(rsac_ctx *ctx, const void *pts3d, const void *pts2d, int32_t n,
                                         const double K[9], int64_t hyp_begin, int32_t n_hyps, double reproj_thresh,
                                         uint64_t seed, uint32_t flags, const int32_t *subsets, int32_t *counts_out,
                                         int8_t *status_out, double *models_out, int64_t *costs_out, void *stream);
RSAC_EXPORT int rsac_score_poses_msac(rsac_ctx *ctx, const void *pts3d, const void *pts2d, int32_t n,
                                      const double K[9], const double *poses, int32_t n_poses, double reproj_thresh,
                                      uint32_t flags, int32_t *counts_out, int64_t *costs_out, void *stream);
/* Host-only (no GPU needed).  rsac_msac_shift: k of a threshold.  rsac_pnp_cost_host: count and cost
 * of one pose (R 9, t 3) over f64 AoS points rounded to f32 like every other path; the source the
 * kernel runs.  rsac_scan_msac: the MSAC scan over (status, count, cost) in hypothesis order, as
 * rsac_scan is the count rule's. */
RSAC_EXPORT int rsac_msac_shift(double thresh);
RSAC_EXPORT int rsac_pnp_cost_host(const double *pts3d, const double *pts2d, int32_t n, const double K[9],
                                   const double model[12], double thresh, int32_t *count_out, int64_t *cost_out);
typedef struct rsac_scan_msac_state {
    int64_t niters;    /* as rsac_scan_state */
    int64_t best;
    int64_t iter;
    int32_t max_good;  /* inliers of the best (not necessarily the largest count seen) */
    int32_t done;
    int64_t best_cost; /* cost of the best, -1 = none */
} rsac_scan_msac_state;
RSAC_EXPORT void rsac_scan_msac_init(rsac_scan_msac_state *st, int32_t max_iters);
RSAC_EXPORT int rsac_scan_msac(rsac_scan_msac_state *st, const int32_t *counts, const int64_t *costs,
                               const int8_t *status, int64_t count, int32_t n, int32_t model_points,
                               double confidence);
/* MSAC for homographies (DESIGN.md "MSAC scoring for homographies"): the same cost with e the f32
 * squared transfer error of the homography test (H's first 8 entries rounded to f32) and thr2 taken
 * after the `thresh <= 0 -> 3.0` default; model_points = 4; a 4-point problem keeps findHomography's
 * direct branch and reports cost -1.  rsac_location_search leaves one cost per location.
 * rsac_homography_hypotheses_msac: rsac_homography_hypotheses plus the per-hypothesis costs
 * (costs_out required; Philox or caller subsets; the threshold is taken as given).
 * rsac_hom_cost_host (host-only): count and cost of one homography (H 9 row-major) over f64 AoS points
 * rounded to f32; the source the kernels run. */
RSAC_EXPORT int rsac_homography_hypotheses_msac(rsac_ctx *ctx, const void *src, const void *dst, int32_t n,
                                                int64_t hyp_begin, int32_t n_hyps, double reproj_thresh,
                                                uint64_t seed, uint32_t flags, const int32_t *subsets,
                                                int32_t *counts_out, int8_t *status_out, double *models_out,
                                                int64_t *costs_out, void *stream);
RSAC_EXPORT int rsac_hom_cost_host(const double *src, const double *dst, int32_t n, const double H[9], double thresh,
                                   int32_t *count_out, int64_t *cost_out);

/* LMedS homography (cv2.findHomography(src, dst, cv2.LMEDS); DESIGN.md "LMedS homography"): least
 * median of squares, the robust method that takes no pixel threshold.  Subsets and minimal models
 * are those of rsac_homography_ransac.  A hypothesis is ranked by the median of its f32 transfer
 * errors over all n points: with key(e) = the bit pattern of e (0x7FC00000 for a NaN of either sign,
 * so a NaN ranks above +inf) and s the ascending keys read back as f32, median = (double)s[n/2] for
 * odd n and (double)(s[n/2-1] + s[n/2]) * 0.5 for even n (the sum in f32); a hypothesis without a
 * model reports -1.  Scanned in index order over niters hypotheses, the strictly lowest median wins
 * (f64 compare; ties keep the earlier index; a NaN median never wins; status < 0 ends the scan).
 * niters = max(RANSACUpdateNumIters(confidence, 0.45, 4, max_iters), 3) with RSAC_F_ADAPTIVE
 * (OpenCV's fixed rule: 55 at 0.995 / 2000), else max_iters.  Then sigma = max(2.5 * 1.4826 *
 * (1 + 5 / (n - 4)) * sqrt(median), 0.001), mask bit i = err_i <= (float)(sigma * sigma), and the
 * call succeeds iff the mask has >= 4 ones (else RSAC_NO_MODEL, H and mask zero).  A 4-point
 * problem takes findHomography's direct branch (its four points' model, mask all ones, median 0).
 * RSAC_F_REFINE with n > 4: the least-squares + LM refit of rsac_homography_ransac on the mask.
 * Flags: SAMPLER_OPENCV, ADAPTIVE, REFINE, DEVICE_IN, DEVICE_SOA, DEVICE_OUT; any other returns
 * RSAC_EINVAL.  n < 4: RSAC_ETOOFEW.  confidence must lie in (0, 1).
 * median_out / medians_out (optional): the winner's median (-1 without a model).
 * stats (optional): score_ms times the median kernel, iters = hypotheses consumed. */
RSAC_EXPORT int rsac_homography_lmeds(rsac_ctx *ctx, const void *src, const void *dst, int32_t n, int32_t max_iters,
                                      double confidence, uint64_t seed, uint32_t flags, double H_out[9],
                                      uint8_t *mask_out, double *median_out, rsac_stats *stats, void *stream);
RSAC_EXPORT int rsac_homography_lmeds_batched(rsac_ctx *ctx, const void *src, const void *dst, const int64_t *offsets,
                                              int32_t n_problems, int32_t max_iters, double confidence, uint64_t seed,
                                              uint32_t flags, double *H_out, int32_t *status_out,
                                              int32_t *n_inliers_out, double *medians_out, uint8_t *mask_out,
                                              void *stream);
/* per-hypothesis probe, the twin of rsac_homography_hypotheses: status, median (f64; -1 without a
 * model) and model of hypotheses [hyp_begin, hyp_begin + n_hyps); flags DEVICE_IN, DEVICE_SOA,
 * DEVICE_OUT (device outputs, enqueued without waiting) */
RSAC_EXPORT int rsac_homography_medians(rsac_ctx *ctx, const void *src, const void *dst, int32_t n, int64_t hyp_begin,
                                        int32_t n_hyps, uint64_t seed, uint32_t flags, const int32_t *subsets,
                                        double *medians_out, int8_t *status_out, double *models_out, void *stream);
/* Host-only (no GPU needed).  rsac_hom_median_host: the median of one homography (H 9 row-major)
 * over f64 AoS points rounded to f32, the source the kernel runs.  rsac_lmeds_sigma: the sigma
 * above, floored at 0.001.  rsac_lmeds_num_iters: the RSAC_F_ADAPTIVE iteration count.
 * rsac_scan_lmeds: the scan over (status, median) rows in hypothesis order; it may be fed in
 * chunks, as rsac_scan_msac. */
RSAC_EXPORT int rsac_hom_median_host(const double *src, const double *dst, int32_t n, const double H[9],
                                     double *median_out);
RSAC_EXPORT double rsac_lmeds_sigma(double median, int32_t n, int32_t model_points);
RSAC_EXPORT int rsac_lmeds_num_iters(double confidence, int32_t model_points, int32_t max_iters);
typedef struct rsac_scan_lmeds_state {
    int64_t niters;     /* iteration budget (fixed) */
    int64_t best;       /* index of the best hypothesis so far, -1 = none */
    int64_t iter;       /* hypotheses consumed */
    int32_t done;       /* budget reached or sampler exhausted */
    double best_median; /* median of the best, DBL_MAX = none */
} rsac_scan_lmeds_state;
RSAC_EXPORT void rsac_scan_lmeds_init(rsac_scan_lmeds_state *st, int64_t n_iters);
RSAC_EXPORT int rsac_scan_lmeds(rsac_scan_lmeds_state *st, const int8_t *status, const double *medians,
                                int64_t count);

/* MSAC and LMedS for the fundamental matrix (DESIGN.md "MSAC and LMedS for the fundamental matrix").
 * The per-point error of both is the f32 squared Sampson distance: with r and den the residual and
 * the denominator of the inlier test r^2 <= T den (the same f64 fma chain), e = 0 when r^2 == 0,
 * else (float)(r^2 / den), the IEEE f64 quotient rounded once; +inf for den == 0 < r^2, NaN only
 * from a NaN or infinite operand.  The inlier decision stays the division-free f64 test at
 * T = (double)thr2, so counts and masks are the count rule's; an inlier has e <= thr2.
 * MSAC (RSAC_F_MSAC on rsac_fundamental_ransac): the cost above with the point term
 * inlier ? min(q(e), Q) : Q and model_points = 8 (eligible iff status > 0 and count > 7); it
 * implies the exact f64 path; threshold finite and positive; rsac_last_costs returns the one cost.
 * rsac_fundamental_hypotheses_msac: rsac_fundamental_hypotheses plus the per-hypothesis costs
 * (costs_out required; exact path).
 * LMedS (rsac_fundamental_lmeds): one problem, Philox sampler; a hypothesis is ranked by the
 * median of key(e) over all n points exactly as rsac_homography_lmeds defines it, scanned over
 * niters = rsac_lmeds_num_iters(confidence, 8, max_iters) hypotheses with RSAC_F_ADAPTIVE (548 at
 * 0.99 / 2000), else max_iters.  Then sigma = rsac_lmeds_sigma(median, n, 8), thr2 =
 * (float)(sigma * sigma), and the mask is the count rule's at that bound; success iff it has >= 8
 * ones (else RSAC_NO_MODEL, F and mask zero).  No refit.  Flags: ADAPTIVE, DEVICE_IN, DEVICE_SOA,
 * DEVICE_OUT; any other returns RSAC_EINVAL.  n < 9: RSAC_ETOOFEW (sigma divides by n - 8).
 * confidence must lie in (0, 1).  median_out (optional): the winner's median (-1 without a model).
 * stats (optional): score_ms times the median kernel.
 * rsac_fundamental_medians: the twin of rsac_homography_medians (no caller subsets).
 * Host-only (no GPU needed), over f64 AoS points rounded to f32, the source the kernels run:
 * rsac_fm_err_host (n errors), rsac_fm_cost_host (count and cost of one F, 9 row-major),
 * rsac_fm_median_host (n >= 1). */
RSAC_EXPORT int rsac_fundamental_hypotheses_msac(rsac_ctx *ctx, const void *pts1, const void *pts2, int32_t n,
                                                 int64_t hyp_begin, int32_t n_hyps, double thresh, uint64_t seed,
                                                 uint32_t flags, int32_t *counts_out, int8_t *status_out,
                                                 double *models_out, int64_t *costs_out, void *stream);
RSAC_EXPORT int rsac_fundamental_lmeds(rsac_ctx *ctx, const void *pts1, const void *pts2, int32_t n, int32_t max_iters,
                                       double confidence, uint64_t seed, uint32_t flags, double F_out[9],
                                       uint8_t *mask_out, double *median_out, rsac_stats *stats, void *stream);
RSAC_EXPORT int rsac_fundamental_medians(rsac_ctx *ctx, const void *pts1, const void *pts2, int32_t n,
                                         int64_t hyp_begin, int32_t n_hyps, uint64_t seed, uint32_t flags,
                                         double *medians_out, int8_t *status_out, double *models_out, void *stream);
RSAC_EXPORT int rsac_fm_err_host(const double *pts1, const double *pts2, int32_t n, const double F[9], float *err_out);
RSAC_EXPORT int rsac_fm_cost_host(const double *pts1, const double *pts2, int32_t n, const double F[9], double thresh,
                                  int32_t *count_out, int64_t *cost_out);
RSAC_EXPORT int rsac_fm_median_host(const double *pts1, const double *pts2, int32_t n, const double F[9],
                                    double *median_out);

/* Seven-point fundamental matrix (RSAC_F_FM_7POINT; DESIGN.md §23 defines the semantics -- there is
 * no OpenCV parity claim).
 *   Samples: sample s draws 7 distinct indices with the Philox subset draw of the 8-point path,
 *   keyed by (seed, rng_base + s).  A sample owns three consecutive hypothesis records 3s, 3s + 1,
 *   3s + 2: record 3s + r holds the model of the r-th real root of det(G1 + lambda G2) in ascending
 *   root order (status 1); a record past the sample's model count has status 0, a zero model, count 0,
 *   cost -1 and median -1, as a failed 8-point sample has; a failed draw gives status -1 on all three.
 *   Units: max_iters, the RANSACUpdateNumIters bound (model_points = 7; eligibility count > 6) and
 *   rsac_stats.iters count samples; rsac_stats.best_hyp is the record index (sample best_hyp / 3,
 *   root best_hyp % 3) and hyps_scored counts records.  A scan tests its bound where a sample begins,
 *   so a sample is consumed whole.  The probes take hyp_begin and n_hyps in samples and write
 *   3 * n_hyps rows.  The hypothesis buffers hold n_problems * 3 * max_iters records.
 *   Point counts: RANSAC needs n >= 7 (RSAC_ETOOFEW below; n == 7 runs the ordinary loop), LMedS
 *   n >= 8 (sigma = rsac_lmeds_sigma(median, n, 7) divides by n - 7) and succeeds with >= 7 ones in
 *   the mask.  RSAC_F_REFINE and the fit calls are unchanged: they still need 8 masked points, and a
 *   fit without a model keeps the minimal F.
 * Host-only (no GPU needed), the source the kernel runs, bit for bit:
 *   rsac_cubic_real_roots: the real roots of c[0] + c[1] x + c[2] x^2 + c[3] x^3 in ascending order
 *   -> roots_out[0 .. count); returns the count (0 .. 3).  c[3] == 0 is the quadratic, c[3] == c[2]
 *   == 0 the linear case; no roots when c[1] is zero too.
 *   rsac_fm_minimal7: 7 correspondences (7 x 2 f64 AoS each, rounded to f32 like every other path)
 *   -> *n_models (0 .. 3) models, row-major 3 x 3 each at unit Frobenius norm, in F_out[0 .. 9 n) in
 *   ascending root order; the rest of F_out is zeroed.  RSAC_OK, or RSAC_EINVAL for a null pointer. */
RSAC_EXPORT int rsac_cubic_real_roots(const double c[4], double roots_out[3]);
RSAC_EXPORT int rsac_fm_minimal7(const double *pts1, const double *pts2, double F_out[27], int32_t *n_models);

/* Essential matrix from five points (DESIGN.md §24 defines the semantics -- there is no parity claim
 * with cv2.findEssentialMat, which normalises the threshold by the focal length and uses another
 * error measure).  K1, K2: row-major 3 x 3 intrinsics of the two views; K2 == NULL means K1 for both.
 * Kinv = adj(K) / det(K) in f64 is computed once on the host and is what the kernel reads; a singular
 * or non-finite K is RSAC_EINVAL.
 *   Samples: sample s draws 5 distinct indices with the Philox subset draw of the 8-point path, keyed
 *   by (seed, rng_base + s).  The solver (Nister's construction, rsac_em5.h) returns up to ten models;
 *   a hypothesis is stored as the pixel-space matrix F = Kinv2^T E Kinv1 at unit Frobenius norm, so
 *   every fundamental-matrix scorer, mask and fit runs on it unchanged, and thresh is in pixels on the
 *   Sampson distance of F, as for rsac_fundamental_ransac.  A sample owns ten consecutive hypothesis
 *   records 10 s .. 10 s + 9: record 10 s + r holds the model of the r-th real root in ascending
 *   order (status 1); a record past the sample's model count has status 0, a zero model, count 0 and
 *   cost -1; a failed draw gives status -1 on all ten.
 *   Units: max_iters, the RANSACUpdateNumIters bound (model_points = 5; eligibility count > 4) and
 *   rsac_stats.iters count samples; rsac_stats.best_hyp is the record index (sample best_hyp / 10,
 *   root best_hyp % 10) and hyps_scored counts records.  A scan tests its bound where a sample
 *   begins, so a sample is consumed whole.  The hypothesis buffers hold n_problems * 10 * max_iters
 *   records (16 doubles each and the f32 pre-filter record): choose max_iters with that in mind.
 * rsac_essential_ransac: rsac_fundamental_ransac's loop on such samples.  n < 5 is RSAC_ETOOFEW;
 *   n == 5 runs the ordinary loop.  Flags: RSAC_F_ADAPTIVE, RSAC_F_MSAC, RSAC_F_REFINE,
 *   RSAC_F_EXACT_ONLY, RSAC_F_DEVICE_IN, RSAC_F_DEVICE_SOA, RSAC_F_DEVICE_OUT; every other flag
 *   (RSAC_F_FM_7POINT included) is RSAC_EINVAL.  RSAC_F_REFINE runs the fundamental-matrix fit on the
 *   winner's mask; a fit without a model (always under 8 masked points) keeps the minimal F.
 *   F_out (optional): the F returned; E_out (required) = rsac_essential_from_fundamental of it;
 *   zeros without a model.  mask_out, stats as rsac_fundamental_ransac.
 * rsac_essential_ransac_batched: as rsac_fundamental_ransac_batched, with K1s / K2s of n_problems x 9
 *   (K2s may be NULL) and an extra E_out of n_problems x 9; problem p returns the bits of the single
 *   call on its points and intrinsics.
 * rsac_essential_hypotheses: the per-hypothesis probe in sample units: hyp_begin and n_hyps count
 *   samples, the outputs hold 10 * n_hyps rows.  costs_out (optional) selects the exact path and
 *   returns the MSAC costs, as the _msac probes do.  Flags: RSAC_F_EXACT_ONLY and the DEVICE flags.
 * Host-only (no GPU needed):
 *   rsac_poly_real_roots: the real roots of c[0] + c[1] x + .. + c[degree] x^degree, degree <= 10, in
 *   ascending order -> roots_out[0 .. count) (room for 10); returns the count.  Zero (or, against the
 *   rest, vanishing) leading coefficients lower the degree; a constant or all-zero polynomial has no
 *   roots.  Roots of even multiplicity are not reported.
 *   rsac_em_minimal5: 5 correspondences (5 x 2 f64 AoS each, rounded to f32 like every other path)
 *   -> *n_models (0 .. 10) models in ascending root order: F_out[0 .. 9 n) as the kernel stores them,
 *   E_out[0 .. 9 n) (optional) the solver's E at unit Frobenius norm; the rest is zeroed.  The source
 *   the kernel runs, bit for bit.
 *   rsac_essential_from_fundamental: M = K2^T F K1 with its singular values set to (1, 1, 0) / sqrt 2
 *   (unit Frobenius norm); sign: the largest-magnitude entry, the first in row-major order, is
 *   positive.  RSAC_NO_MODEL (zeros) when M has rank < 2 or is not finite.
 *   rsac_essential_recover_pose: (R, t) with x2 ~ R x1 + t, det R = +1, |t| = 1 from E.  The four
 *   candidates in the order (R_a, +t), (R_a, -t), (R_b, +t), (R_b, -t); every point with mask[i] != 0
 *   (mask == NULL: all) is triangulated from its two normalised rays, and the candidate with the most
 *   points at positive depth in both cameras wins, ties keeping the earlier one.  n_front_out
 *   (optional): the four counts.  RSAC_NO_MODEL when no point is in front for any candidate. */
RSAC_EXPORT int rsac_essential_ransac(rsac_ctx *ctx, const void *pts1, const void *pts2, int32_t n,
                                      const double K1[9], const double K2[9], int32_t max_iters, double thresh,
                                      double confidence, uint64_t seed, uint32_t flags, double E_out[9],
                                      double F_out[9], uint8_t *mask_out, rsac_stats *stats, void *stream);
RSAC_EXPORT int rsac_essential_ransac_batched(rsac_ctx *ctx, const void *pts1, const void *pts2,
                                              const int64_t *offsets, int32_t n_problems, const double *K1s,
                                              const double *K2s, int32_t max_iters, double thresh, double confidence,
                                              uint64_t seed, uint32_t flags, double *E_out, double *F_out,
                                              int32_t *status_out, int32_t *n_inliers_out, uint8_t *mask_out,
                                              void *stream);
RSAC_EXPORT int rsac_essential_hypotheses(rsac_ctx *ctx, const void *pts1, const void *pts2, int32_t n,
                                          const double K1[9], const double K2[9], int64_t hyp_begin, int32_t n_hyps,
                                          double thresh, uint64_t seed, uint32_t flags, int32_t *counts_out,
                                          int8_t *status_out, double *models_out, int64_t *costs_out, void *stream);
RSAC_EXPORT int rsac_poly_real_roots(const double *c, int32_t degree, double *roots_out);
RSAC_EXPORT int rsac_em_minimal5(const double *pts1, const double *pts2, const double K1[9], const double K2[9],
                                 double F_out[90], double E_out[90], int32_t *n_models);
RSAC_EXPORT int rsac_essential_from_fundamental(const double F[9], const double K1[9], const double K2[9],
                                                double E_out[9]);
RSAC_EXPORT int rsac_essential_recover_pose(const double *pts1, const double *pts2, int32_t n, const double K1[9],
                                            const double K2[9], const double E[9], const uint8_t *mask,
                                            double R_out[9], double t_out[3], int32_t n_front_out[4]);

/* Essential matrix: the calibrated refit and the local optimisation (DESIGN.md §25 defines the
 * semantics; additions, RSAC_ABI_VERSION unchanged).  The refit minimises the sum of squared Sampson
 * residuals of F = Kinv2^T [t]x R Kinv1 over the masked points (mask[i] != 0; mask == NULL: all) by
 * Levenberg-Marquardt on the five parameters of (R, |t| = 1), started from the decomposition of E_in
 * (rsac_emfit.h: a fixed number of passes, one summation order), so the result is an essential
 * matrix and a least-squares fit at once.  Pixels are rounded to f32 and taken in f64, as on every
 * other path.  Outputs: E_out (unit Frobenius norm, the largest-magnitude entry -- the first in
 * row-major order -- positive), F_out = Kinv2^T E Kinv1 at unit norm, cost_out the final sum of
 * squared residuals (never above the start's), count_out the masked points, steps_out the accepted
 * LM steps; all but E_out optional.  RSAC_NO_MODEL (zeros; the count is still reported once the
 * start was accepted) for fewer than 5 masked points, a non-finite coordinate or a degenerate point
 * under the mask, and an E_in that is not finite or has rank < 2 (w1 <= 1e-8 w0).  A singular or
 * non-finite K is RSAC_EINVAL.  None of these calls touches rsac_last_stats.
 *   rsac_essential_refine: on the host, no GPU needed; pts1, pts2 n x 2 f64.
 *   rsac_essential_refine_device: the same bits from k_em_refine.  Flags: RSAC_F_DEVICE_IN,
 *   RSAC_F_DEVICE_SOA; the mask is a device pointer when the points are.
 *   rsac_essential_refine_batched_device: n_problems problems in one launch; offsets as the batched
 *   fundamental-matrix calls, K1s / K2s n_problems x 9 (K2s may be NULL), masks concatenated or NULL,
 *   E_in and the outputs one row per problem; status_out[p] RSAC_OK or RSAC_NO_MODEL.  Returns
 *   RSAC_OK when any problem has a model.
 *   rsac_essential_local_opt, _batched: rsac_fundamental_local_opt's loop with the refit in place of
 *   the fit.  mask_0 is the count rule's mask of F(E_in) at thresh; round k refits E_(k-1) on
 *   mask_(k-1) and takes the mask of the result; it is accepted iff its count rises strictly; at most
 *   max_rounds rounds are accepted; a count under 5 or a refit without a model ends the loop.  -> the
 *   last accepted E (E_in itself after 0 steps), its count, the accepted rounds, its mask.  An E_in
 *   row the refit cannot start from (all zero included) gives a zero row, count 0, steps 0.  Flags:
 *   RSAC_F_DEVICE_IN, RSAC_F_DEVICE_SOA, RSAC_F_DEVICE_OUT.  max_rounds < 1 or a threshold that is not
 *   finite and positive is RSAC_EINVAL.
 *   rsac_essential_to_fundamental (host only): F = Kinv2^T E Kinv1 at unit Frobenius norm, the
 *   formula the calls above use; RSAC_NO_MODEL for a zero or non-finite product. */
RSAC_EXPORT int rsac_essential_refine(const double *pts1, const double *pts2, int32_t n, const double K1[9],
                                      const double K2[9], const uint8_t *mask, const double E_in[9], double E_out[9],
                                      double F_out[9], double *cost_out, int32_t *count_out, int32_t *steps_out);
RSAC_EXPORT int rsac_essential_refine_device(rsac_ctx *ctx, const void *pts1, const void *pts2, int32_t n,
                                             const double K1[9], const double K2[9], const uint8_t *mask,
                                             const double E_in[9], uint32_t flags, double E_out[9], double F_out[9],
                                             double *cost_out, int32_t *count_out, int32_t *steps_out, void *stream);
RSAC_EXPORT int rsac_essential_refine_batched_device(rsac_ctx *ctx, const void *pts1, const void *pts2,
                                                     const int64_t *offsets, int32_t n_problems, const double *K1s,
                                                     const double *K2s, const uint8_t *masks, const double *E_in,
                                                     uint32_t flags, double *E_out, double *F_out, double *cost_out,
                                                     int32_t *count_out, int32_t *steps_out, int32_t *status_out,
                                                     void *stream);
RSAC_EXPORT int rsac_essential_local_opt(rsac_ctx *ctx, const void *pts1, const void *pts2, int32_t n,
                                         const double K1[9], const double K2[9], const double E_in[9], double thresh,
                                         int32_t max_rounds, uint32_t flags, double E_out[9], int32_t *count_out,
                                         int32_t *steps_out, uint8_t *mask_out, void *stream);
RSAC_EXPORT int rsac_essential_local_opt_batched(rsac_ctx *ctx, const void *pts1, const void *pts2,
                                                 const int64_t *offsets, int32_t n_problems, const double *K1s,
                                                 const double *K2s, const double *E_in, double thresh,
                                                 int32_t max_rounds, uint32_t flags, double *E_out,
                                                 int32_t *counts_out, int32_t *steps_out, uint8_t *mask_out,
                                                 void *stream);
RSAC_EXPORT int rsac_essential_to_fundamental(const double E[9], const double K1[9], const double K2[9],
                                              double F_out[9]);

/* LMedS PnP (DESIGN.md "LMedS PnP"): a camera pose without a pixel threshold.  Samples and minimal
 * models are those of rsac_pnp_ransac under the same flags (P3P, or EPnP on 5 points with
 * RSAC_F_MINIMAL_EPNP5; the rvec round trip with RSAC_F_RVEC_ROUNDTRIP).  The per-point error is the
 * exact RANSAC test's: the f64 projection of the f32-rounded points, the pixel differences rounded
 * to f32, dx * dx + dy * dy in f32 (the call implies the all-f64 path, as RSAC_F_MSAC does: no frame,
 * no f32 records, no pre-filter).  A hypothesis is ranked by the median of key(e) over all n points
 * exactly as rsac_homography_lmeds defines it (a NaN ranks above +inf, odd and even n, the sum of the
 * two middle values in f32); status <= 0 reports -1.  The scan is rsac_scan_lmeds over niters
 * hypotheses in one round: niters = rsac_lmeds_num_iters(confidence, model_points, max_iters) with
 * RSAC_F_ADAPTIVE (48 for P3P and 89 for EPnP-5 at 0.99 / 2000), else max_iters; model_points = the
 * sample size, 4 or 5.  Then sigma = rsac_lmeds_sigma(median, n, model_points), thr2 =
 * (float)(sigma * sigma), mask bit i = err_i <= thr2, and the call succeeds iff the mask has >=
 * model_points ones (else RSAC_NO_MODEL: R, t and the mask zero, median -1).  A problem of exactly
 * model_points points (4; 5 with RSAC_F_MINIMAL_EPNP5) keeps rsac_pnp_ransac's direct branch: its
 * minimal model, mask all ones, median 0.  RSAC_F_REFINE and / or RSAC_F_EPNP: rsac_pnp_ransac's
 * final solve on the LMedS mask; without either the winner's minimal model is returned.
 * Flags: SAMPLER_OPENCV, ADAPTIVE, REFINE, EPNP, MINIMAL_EPNP5, RVEC_ROUNDTRIP, DEVICE_IN, DEVICE_SOA,
 * DEVICE_OUT; any other returns RSAC_EINVAL.  confidence must lie in (0, 1), max_iters >= 1.
 * n < 4 (any problem of a batch): RSAC_ETOOFEW.
 * rsac_pnp_lmeds_batched: n_problems independent problems (offsets, K n_problems x 9; a K sweep
 * repeats the point rows, as for rsac_pnp_ransac_batched); returns RSAC_OK when any has a model.
 * median_out / medians_out (optional): the winner's median.  stats (optional; also
 * rsac_last_stats under rsac_set_timing): score_ms times the median kernel, iters = hypotheses
 * consumed, n_inliers = ones in the mask, rounds = 1.
 * rsac_pnp_medians: the per-hypothesis probe, the twin of rsac_homography_medians: status, median
 * and model record of hypotheses [hyp_begin, hyp_begin + n_hyps) (Philox, or caller subsets of
 * n_hyps x 4 indices, x 5 with MINIMAL_EPNP5); flags MINIMAL_EPNP5, RVEC_ROUNDTRIP, DEVICE_IN,
 * DEVICE_SOA, DEVICE_OUT (device outputs, enqueued without waiting).
 * rsac_pnp_median_host (host-only, n >= 1): the median of one pose (R 9 row-major, then t) over f64
 * AoS points rounded to f32, the source the kernels run. */
RSAC_EXPORT int rsac_pnp_lmeds(rsac_ctx *ctx, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                               int32_t max_iters, double confidence, uint64_t seed, uint32_t flags, double R_out[9],
                               double t_out[3], uint8_t *mask_out, double *median_out, rsac_stats *stats,
                               void *stream);
RSAC_EXPORT int rsac_pnp_lmeds_batched(rsac_ctx *ctx, const void *pts3d, const void *pts2d, const int64_t *offsets,
                                       int32_t n_problems, const double *K, int32_t max_iters, double confidence,
                                       uint64_t seed, uint32_t flags, double *R_out, double *t_out,
                                       int32_t *status_out, int32_t *n_inliers_out, double *medians_out,
                                       uint8_t *mask_out, void *stream);
RSAC_EXPORT int rsac_pnp_medians(rsac_ctx *ctx, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                                 int64_t hyp_begin, int32_t n_hyps, uint64_t seed, uint32_t flags,
                                 const int32_t *subsets, double *medians_out, int8_t *status_out, double *models_out,
                                 void *stream);
RSAC_EXPORT int rsac_pnp_median_host(const double *pts3d, const double *pts2d, int32_t n, const double K[9],
                                     const double model[12], double *median_out);

/* Least-squares fundamental matrix and local optimisation (DESIGN.md "Fundamental matrix:
 * least-squares refit and local optimisation").
 * The fit: the normalised 8-point least squares over the masked points (mask NULL = all; f64 AoS
 * points rounded to f32, taken in f64) -- centroids and mean distances over the masked points,
 * s = sqrt 2 / mean, the 9 x 9 moment matrix of fm's rows, its smallest eigenvector by cyclic
 * Jacobi (ties: the lower index), then the rank-2 step, denormalisation and unit Frobenius norm of
 * the minimal solver.  Every O(n) sum is taken in one order defined over point indices (ranges of
 * 4096 points, 512 slots each), so every backend returns the same bits.  Fewer than 8 masked
 * points, a non-finite coordinate under the mask, coincident points: RSAC_NO_MODEL, F_out zero.
 * rsac_fundamental_fit: host-only (no GPU needed), the source the kernels run.
 * rsac_fundamental_fit_device: the same bits from the kernels.  Flags: DEVICE_IN, DEVICE_SOA; the
 * mask is a device pointer when the points are.  F_out is host memory; the call synchronises.
 * rsac_fundamental_local_opt: from F_in, mask_0 = the count rule's mask of F_in at thresh (the
 * test of rsac_fundamental_ransac), c_0 its count; round k: F_k = fit(mask_{k-1}), mask_k the mask
 * of F_k; accepted iff c_k > c_{k-1}, else the loop stops and keeps round k - 1; at most
 * max_rounds accepted rounds; c < 8 or a fit without a model ends it the same way.  Outputs: the
 * last accepted F (F_in itself after 0 rounds), its count, the accepted rounds and (optional) its
 * mask -- a device pointer with DEVICE_OUT.  Flags: DEVICE_IN, DEVICE_SOA, DEVICE_OUT.
 * max_rounds < 1 or a threshold that is not finite and positive: RSAC_EINVAL.  One host
 * synchronisation per round.
 * RSAC_F_REFINE on rsac_fundamental_ransac (also with RSAC_F_MSAC): after the loop, one fit on the
 * winner's mask where it lies on the device; F_out is the fit, the mask stays the RANSAC-phase
 * mask (the convention of the PnP and homography refits); a fit without a model leaves the
 * minimal F in F_out.  RSAC_F_LO, RSAC_F_SAMPLER_OPENCV and RSAC_F_EPNP stay RSAC_EINVAL there;
 * rsac_fundamental_lmeds keeps rejecting RSAC_F_REFINE (fit on its mask by a second call).
 * None of these calls touches rsac_last_stats. */
RSAC_EXPORT int rsac_fundamental_fit(const double *pts1, const double *pts2, int32_t n, const uint8_t *mask,
                                     double F_out[9]);
RSAC_EXPORT int rsac_fundamental_fit_device(rsac_ctx *ctx, const void *pts1, const void *pts2, int32_t n,
                                            const uint8_t *mask, uint32_t flags, double F_out[9], void *stream);
RSAC_EXPORT int rsac_fundamental_local_opt(rsac_ctx *ctx, const void *pts1, const void *pts2, int32_t n,
                                           const double F_in[9], double thresh, int32_t max_rounds, uint32_t flags,
                                           double F_out[9], int32_t *count_out, int32_t *steps_out,
                                           uint8_t *mask_out, void *stream);

/* Homography refit and local optimisation on the device (DESIGN.md "Homography: least-squares and
 * LM refit and local optimisation on GPU").
 * The fit is rsac_homography_fit's: findHomography's normalised least-squares DLT over the masked
 * points (mask NULL = all; f64 AoS points rounded to f32, taken in f64) -- masked centroids and
 * mean absolute deviations, the 9 x 9 LtL, its smallest eigenvector by cyclic Jacobi,
 * denormalisation -- then ten iterations of OpenCV's LMSolver on h0..h7.  Every sum is one
 * left-to-right chain over the masked points in ascending index, on the host and on the device, so
 * both return the same nine doubles.  Fewer than 4 masked points or a zero deviation sum:
 * RSAC_NO_MODEL, H_out zero.
 * rsac_homography_fit_device: the kernel's result for one problem (n >= 4, else RSAC_ETOOFEW).
 * Flags: DEVICE_IN, DEVICE_SOA, or none (host f64 AoS, staged like every other call); the mask is
 * a device pointer when the points are.  H_out is host memory; the call synchronises.
 * rsac_homography_fit_batched_device: n_problems independent fits in one launch, one wave each;
 * offsets (n_problems + 1, host) index the concatenated points and masks (NULL = all points);
 * H_out n_problems x 9 (a row of zeros without a model), status_out (optional) RSAC_OK or
 * RSAC_NO_MODEL per problem; returns RSAC_OK when any problem has a model.  A problem may have
 * fewer than 4 points (no model).
 * rsac_homography_local_opt: from H_in, mask_0 = the homography test's mask of H_in at thresh (the
 * f32 error of H's first eight entries rounded to f32, against (float)(thresh * thresh): the test
 * of rsac_homography_ransac), c_0 its count; round k: H_k = fit(mask_{k-1}), mask_k the mask of
 * H_k; accepted iff c_k > c_{k-1}, else the loop stops and keeps round k - 1; at most max_rounds
 * accepted rounds; c < 4 or a fit without a model ends it the same way.  Outputs: the last
 * accepted H (H_in itself after 0 rounds), its count, the accepted rounds and (optional) its mask
 * -- a device pointer with DEVICE_OUT.  Flags: DEVICE_IN, DEVICE_SOA, DEVICE_OUT.  max_rounds < 1
 * or a threshold that is not finite and positive: RSAC_EINVAL.  One host synchronisation per round.
 * RSAC_F_REFINE on the homography RANSAC and LMedS calls and in rsac_location_search runs this fit
 * on the device, from the mask where it lies and without copying points or masks to the host,
 * where that was measured faster than the host refit (the location search and batches of at least
 * 8 problems of at least 2000 points on average: DESIGN.md); a single problem keeps the host
 * refit.  The same bits either way (RSAC_DBG_HOM_FIT forces one or the other).  RSAC_F_LO on those
 * calls is unchanged.
 * None of these calls touches rsac_last_stats. */
RSAC_EXPORT int rsac_homography_fit_device(rsac_ctx *ctx, const void *src, const void *dst, int32_t n,
                                           const uint8_t *mask, uint32_t flags, double H_out[9], void *stream);
RSAC_EXPORT int rsac_homography_fit_batched_device(rsac_ctx *ctx, const void *src, const void *dst,
                                                   const int64_t *offsets, int32_t n_problems, const uint8_t *masks,
                                                   uint32_t flags, double *H_out, int32_t *status_out, void *stream);
RSAC_EXPORT int rsac_homography_local_opt(rsac_ctx *ctx, const void *src, const void *dst, int32_t n,
                                          const double H_in[9], double thresh, int32_t max_rounds, uint32_t flags,
                                          double H_out[9], int32_t *count_out, int32_t *steps_out,
                                          uint8_t *mask_out, void *stream);

/* Batched fundamental matrix: many image pairs in one launch sequence (DESIGN.md "Batched
 * fundamental matrix").  offsets (n_problems + 1, host, offsets[0] = 0) index the concatenated
 * points, masks and mask_out; 1 <= n_problems <= 65535.  Problem p of every call below returns, bit
 * for bit, what the single call returns for its points with the same arguments: the Philox draw does
 * not depend on the problem, so it sees the same hypotheses.
 * rsac_fundamental_ransac_batched: rsac_fundamental_ransac per problem (its own scan and, with
 * ADAPTIVE, its own iteration bound).  F_out n_problems x 9 (a zero row without a model), status_out
 * RSAC_OK or RSAC_NO_MODEL per problem, n_inliers_out the winners' counts, mask_out the RANSAC-phase
 * masks (a device pointer with DEVICE_OUT); the three are optional.  Returns RSAC_OK when any problem
 * has a model.  Flags: ADAPTIVE, REFINE, MSAC, EXACT_ONLY, DEVICE_IN, DEVICE_SOA, DEVICE_OUT;
 * SAMPLER_OPENCV, LO, EPNP and ASYNC: RSAC_EINVAL.  A problem of fewer than 8 points: RSAC_ETOOFEW
 * for the call.  MSAC implies the exact path; rsac_last_costs(ctx, costs, n_problems) then returns
 * the winners' costs.  REFINE: one batched fit on the masks where they lie; a problem whose fit has no
 * model keeps its minimal F; the masks stay the RANSAC phase's.  The hypothesis buffers hold
 * n_problems x max_iters records.  Under rsac_set_timing the figures go to rsac_last_stats.
 * rsac_fundamental_lmeds_batched: rsac_fundamental_lmeds per problem; the number of hypotheses is the
 * same for all, every problem's sigma and bound come from its own median and point count, success
 * needs at least 8 ones in its mask; medians_out -1.0 without a model.  Flags: ADAPTIVE, DEVICE_IN,
 * DEVICE_SOA, DEVICE_OUT (REFINE: RSAC_EINVAL).  A problem of fewer than 9 points: RSAC_ETOOFEW.
 * rsac_fundamental_fit_batched_device: rsac_fundamental_fit per problem in three launches whatever
 * n_problems; masks NULL or the concatenated masks, a device pointer when the points are.  A problem
 * may have fewer than 8 (masked) points: no model, a zero row.  Flags: DEVICE_IN, DEVICE_SOA.  Does
 * not touch rsac_last_stats.
 * rsac_fundamental_local_opt_batched: rsac_fundamental_local_opt per problem from the rows of F_in
 * (n_problems x 9; an all-zero row: no model, count 0, steps 0, a zero mask).  Every round is one
 * batched mask, one batched fit and one host synchronisation for the problems still rising; a
 * problem that has stopped is frozen.  Flags: DEVICE_IN, DEVICE_SOA, DEVICE_OUT.  Does not touch
 * rsac_last_stats. */
RSAC_EXPORT int rsac_fundamental_ransac_batched(rsac_ctx *ctx, const void *pts1, const void *pts2,
                                                const int64_t *offsets, int32_t n_problems, int32_t max_iters,
                                                double thresh, double confidence, uint64_t seed, uint32_t flags,
                                                double *F_out, int32_t *status_out, int32_t *n_inliers_out,
                                                uint8_t *mask_out, void *stream);
RSAC_EXPORT int rsac_fundamental_lmeds_batched(rsac_ctx *ctx, const void *pts1, const void *pts2,
                                               const int64_t *offsets, int32_t n_problems, int32_t max_iters,
                                               double confidence, uint64_t seed, uint32_t flags, double *F_out,
                                               int32_t *status_out, int32_t *n_inliers_out, double *medians_out,
                                               uint8_t *mask_out, void *stream);
RSAC_EXPORT int rsac_fundamental_fit_batched_device(rsac_ctx *ctx, const void *pts1, const void *pts2,
                                                    const int64_t *offsets, int32_t n_problems, const uint8_t *masks,
                                                    uint32_t flags, double *F_out, int32_t *status_out, void *stream);
RSAC_EXPORT int rsac_fundamental_local_opt_batched(rsac_ctx *ctx, const void *pts1, const void *pts2,
                                                   const int64_t *offsets, int32_t n_problems, const double *F_in,
                                                   double thresh, int32_t max_rounds, uint32_t flags, double *F_out,
                                                   int32_t *counts_out, int32_t *steps_out, uint8_t *mask_out,
                                                   void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RSAC_H */
