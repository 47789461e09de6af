// rsac_api.hip -- the C ABI of include/rsac.h: context, input staging,
// round loop (solve + score on the GPU, sequential scan on the host),
// masks and refits.
//
// One call == one cv2.solvePnPRansac / cv2.findHomography of the reference
// (main_v1.py:497 / main_v1.py:312), or the whole Python loop around it for
// the batched entry points (main_v1.py:274-284, testpro-K.py:58-75).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <atomic>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/rsac.h"
#include "rsac_em5.h"
#include "rsac_emfit.h"
#include "rsac_host.h"
#include "rsac_internal.h"
#include "rsac_math.h"

using namespace rsac;

static thread_local std::string g_err;

static int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

static int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return fail(RSAC_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    uint64_t gen = 0;  // allocations so far: what a buffer held is gone when it moves (the address may come back)
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        ++gen;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max<size_t>(bytes + bytes / 4, 4096);
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T *as() const { return (T *)p; }
};

struct PinBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max<size_t>(bytes + bytes / 4, 4096);
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T *as() const { return (T *)p; }
};

constexpr size_t kMaxModelBytes = size_t(32) << 30;  // hypothesis records kept resident per call
// OpenCV-sampler rounds up to this many bytes of subsets + statuses are read by the solve kernels
// from pinned host memory instead of being copied (run_loop)
constexpr int64_t kSubsetZeroCopyBytes = 64 << 10;

// hipMemcpy2DAsync, as one linear copy when the rows are contiguous (one problem): the 2-D path
// costs tens of microseconds more per call on this runtime (measured in the adaptive loop)
hipError_t copy_rows(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height,
                     hipMemcpyKind kind, hipStream_t s) {
    if (height == 1 || (dpitch == width && spitch == width))
        return hipMemcpyAsync(dst, src, width * height, kind, s);
    return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, kind, s);
}

}  // namespace

// "The same problem as this context's last call" (DESIGN.md §16): what the set-up of an
// rsac_pnp_evaluate_range call on device f64 inputs read, and where it wrote.  valid only from
// the end of such a call until the next entry point that stages points or builds a frame
// (stage_points and pnp_args clear it); a reallocated scratch buffer fails the comparison.
struct SetupRecord {
    bool valid = false;
    const void *p3 = nullptr, *p2 = nullptr;
    int32_t n = 0;
    double cam[4] = {0, 0, 0, 0};
    float thr2 = 0.f;
    uint32_t flags = 0;  // the flags that shape the set-up (kSetupFlags)
    hipStream_t stream = nullptr;
    const void *buf[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    uint64_t gen[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // ... and their allocation counts (DevBuf::gen)
    bool same(const SetupRecord &o) const {
        return valid && o.valid && p3 == o.p3 && p2 == o.p2 && n == o.n && memcmp(cam, o.cam, sizeof cam) == 0 &&
               memcmp(&thr2, &o.thr2, sizeof thr2) == 0 && flags == o.flags && stream == o.stream &&
               memcmp(buf, o.buf, sizeof buf) == 0 && memcmp(gen, o.gen, sizeof gen) == 0;
    }
};
constexpr uint32_t kSetupFlags = RSAC_F_DEVICE_IN | RSAC_F_DEVICE_SOA | RSAC_F_EXACT_ONLY;

struct rsac_ctx {
    int device = 0;
    SetupRecord setup_rec;      // the last rsac_pnp_evaluate_range's set-up, while nothing rewrote it
    bool setup_reused = false;  // RSAC_DBG_SETUP_REUSED: the last rsac_pnp_evaluate_range launched no set-up
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    // the last async copy out of h_pts / h_small: the host waits on it before rewriting the
    // buffer (calls may return before their copies ran, RSAC_F_ASYNC)
    hipEvent_t ev_pts = nullptr, ev_small = nullptr;
    int64_t round_size = 4096;
    // rsac_set_timing: every PnP call records HIP events around its solve and score launches and
    // leaves its statistics in last_stats (rsac_last_stats)
    bool timing = false;
    rsac_stats last_stats{};
    // device scratch
    DevBuf pts, tables, models, status, counts, subsets, substatus, best, bestmodels, mask;
    int64_t *d_off = nullptr;  // views into `tables`: offsets (P+1), cams (P x 4), thr2 (P)
    double *d_cams = nullptr;
    float *d_thr2 = nullptr;
    DevBuf bounds_ws, frame, fconst, fmodels, queue;  // float32 pre-filter state (PnP)
    DevBuf mxpts;                                              // MFMA point operands (PF, UV: 40 B / point)
    DevBuf epnp5;                                              // EPnP-5 minimal solve: kEpnpRec doubles / hypothesis of a launch
    DevBuf direct;                                             // count == model_points problems (direct_solve)
    PinBuf h_direct;
    DevBuf loc;                                                // location search: inputs, pos2, H, err
    DevBuf lo;                                                 // LO-RANSAC: 2 model records, chain state, 2 masks
    const void *lo_state_base = nullptr;                       // the lo allocation whose LoState is zeroed
    PinBuf h_lo;                                               // LO chain state, written by the device
    PinBuf h_lmfail;                                           // multi-block refit failure word (device-written)
    int dbg_refit_max_blocks = 0;                              // RSAC_DBG_REFIT_MAX_BLOCKS (0: device limit)
    int64_t spec_finishes = 0, spec_redos = 0;                 // RSAC_DBG_SPEC_FINISHES / _REDOS
    int32_t scanrec_copy = 0;  // problems whose device scan records still go to h_scanrec (issue_scanrec_copy)
    int32_t dbg_cell_pts = 0;                                  // RSAC_DBG_MF_CELL_PTS
    bool dbg_spec_overflow = false;                            // RSAC_DBG_SPEC_OVERFLOW
    int64_t dbg_f64_selftest = -1;                             // RSAC_DBG_F64_SELFTEST's last mismatch count
    DevBuf bound;                // bounded scoring: the plan record (64 B), then the survivor list (H int32)
    int dbg_bound = 0;           // RSAC_DBG_BOUND: 0 by size, 1 always, 2 never
    int dbg_bound_slab = 0;      // RSAC_DBG_BOUND_SLAB: 0 the default (the slab body where the guard allows), 1 pass 1
                                 // exact, 2 the slab body whatever the guard says
    int64_t dbg_slab_selftest = -1;  // RSAC_DBG_SLAB_SELFTEST's last count
    bool bound_last = false;     // the last rsac_pnp_evaluate_range took the bounded sequence
    int32_t bound_last_n = 0;    // ... and its point count (RSAC_DBG_BOUND_N1 of an unbounded call)
    int bound_rec = 0;           // ... and which of the two plan records it wrote
    uint64_t bound_hint_gen = 0;  // the `bound` allocation (DevBuf::gen) that record lies in
    bool bound_hinted = false;   // RSAC_DBG_BOUND_HINTED: the last call took the hinted sequence
    int bound_last_exact = 0;    // ... its PnpArgs::bound_exact (RSAC_DBG_BOUND_SLAB_RAN)
    int32_t bound_last_h = 0;    // ... and its hypotheses (RSAC_DBG_BOUND_COUNT)
    int32_t dbg_bound_count = 0;  // RSAC_DBG_BOUND_COUNT: the hypothesis whose count the hook reads
    int32_t dbg_bound_p2_min = 0;  // RSAC_DBG_BOUND_P2_MIN: pass 2's shortest share (0 = as built)
    DevBuf win;                                                // rsac_pnp_winner: the re-derived record
    DevBuf reproj;                                             // reprojection errors / the K sweep's inputs
    DevBuf geo;                                                // geodesy / DEM: staged host inputs and outputs
    DevBuf epnp;                                               // EPnP stage records (P x (stage 1 + stage 2))
    DevBuf lmscr;                                              // multi-block LM refit: tagged wave sums
    DevBuf setup_scr;                                          // k_pnp_setup_fc: ticket + per-block bounds
    DevBuf distbuf;                                            // lens distortion: 8 coefficients, then Uu, Vu (dist_setup)
    DevBuf costs;                                              // RSAC_F_MSAC: per-hypothesis int64 costs (P x hyp_stride)
    PinBuf h_costs;                                            // ... one round's rows on the host
    DevBuf medians;                                            // LMedS: per-hypothesis f64 medians (P x hyp_stride)
    PinBuf h_medians;                                          // ... on the host, then the problems' thr2 (hom_lmeds_core)
    DevBuf medkeys;                                            // LMedS PnP past a block's registers: uint32 key rows
    int64_t dbg_lmeds_keys = 0;                                // RSAC_DBG_LMEDS_KEYS: 0 default budget, > 0 bytes, < 0 none
    int dbg_hom_fit = 0;                                       // RSAC_DBG_HOM_FIT: 0 by policy, 1 host, 2 device
    std::vector<int64_t> last_costs;                           // the winners' costs of the last MSAC call (rsac_last_costs)
    DevBuf em_kinv;                                            // essential matrix: Kinv1, Kinv2 per problem (18 doubles)
    DevBuf emfit;                                              // essential refit: Kinv, E_in, records, on (em_fit_plan)
    PinBuf h_emfit;                                            // ... the records on the host
    DevBuf fmfit;                                              // fm_fit: range sums, then the result (launch_fm_fit)
    DevBuf fmfit_mask;                                         // ... an uploaded host mask / local optimisation's two masks
    PinBuf h_fmfit;                                            // the batched fit: P result records, then the range prefix
    DevBuf homfit;                                             // hom_fit: one result record per problem (launch_hom_fit)
    PinBuf h_homfit;                                           // ... on the host
    DevBuf homfit_mask;                                        // ... an uploaded host mask / local optimisation's two masks
    // a one-problem set-up pnp_args deferred into the first P3P solve (run_loop launches it with
    // the solve as k_pnp_setup_solve4; flush_setup launches it alone where nothing fuses)
    PnpSetupFuse pending_setup{};
    bool pending_on = false;
    LmScratch lm;                                              // ... and its launch counter
    std::vector<char> last_tables;                             // the tables last uploaded (stage_tables)
    void *last_tables_dev = nullptr;
    // pinned host staging
    DevBuf scanrec;                                            // first-round improvement records (P > 1)
    PinBuf h_scanrec;
    PinBuf h_pts, h_small, h_counts, h_status, h_subsets, h_substatus, h_best, h_bestmodels, h_mask, h_epnp;
    PinBuf h_rowinfo;  // rsac_pnp_ransac_batched_rows: {record, n_inliers} per problem
};

// ---------------------------------------------------------------------------
// problem staging
// ---------------------------------------------------------------------------
namespace {

struct Staged {
    int P = 0;
    int64_t total = 0;
    std::vector<int64_t> off;
    int32_t max_n() const {
        int64_t m = 0;
        for (size_t p = 0; p + 1 < off.size(); ++p) m = std::max(m, off[p + 1] - off[p]);
        return (int32_t)m;
    }
    const float *d[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // device SoA
    std::vector<float> hbuf;                                            // host SoA copy (refits, MWC check)
    const float *h[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    bool host_ready = false;
    PnpPrepare prep;  // stage_points(defer): the conversion pnp_args fuses into its frame launch
};

// ncomp3 = 3 for PnP (pts3d N x 3, pts2d N x 2 -> X Y Z U V), 2 for 2D-2D (src, dst -> SX SY DX DY)
// defer: one device-input PnP problem of <= 65536 points, or a batch of problems of at most
// kSetupBatchMaxN points each, is converted by pnp_args' frame launch (the caller must call
// pnp_args next)
int stage_points(rsac_ctx *c, const void *a, const void *b, int ncomp_a, const int64_t *offsets, int32_t P, int32_t n,
                 uint32_t flags, hipStream_t s, Staged &st, bool defer = false) {
    c->setup_rec.valid = false;  // the staged points are about to change (rsac_pnp_evaluate_range keeps a copy)
    st.P = P;
    st.off.resize(P + 1);
    if (offsets) {
        for (int p = 0; p <= P; ++p) st.off[p] = offsets[p];
        if (st.off[0] != 0) return fail(RSAC_EINVAL, "offsets[0] must be 0");
        for (int p = 0; p < P; ++p)
            if (st.off[p + 1] < st.off[p]) return fail(RSAC_EINVAL, "offsets must be non-decreasing");
    } else {
        st.off[0] = 0;
        st.off[1] = n;
    }
    const int64_t N = st.off[P];
    st.total = N;
    const int nc = ncomp_a + 2;
    if (flags & RSAC_F_DEVICE_SOA) {
        const float *A = (const float *)a, *B = (const float *)b;
        for (int k = 0; k < ncomp_a; ++k) st.d[k] = A + k * N;
        st.d[ncomp_a] = B;
        st.d[ncomp_a + 1] = B + N;
        return RSAC_OK;
    }
    HIPCHK(c->pts.ensure(sizeof(float) * nc * std::max<int64_t>(N, 1)));
    float *D = c->pts.as<float>();
    for (int k = 0; k < nc; ++k) st.d[k] = D + k * N;
    if (flags & RSAC_F_DEVICE_IN) {
        int64_t max_n = 0;
        for (int p = 0; p < P; ++p) max_n = std::max<int64_t>(max_n, st.off[p + 1] - st.off[p]);
        if (ncomp_a == 3 && defer && N > 0 && (P == 1 ? N <= 65536 : max_n <= kSetupBatchMaxN)) {
            st.prep = PnpPrepare{(const double *)a, (const double *)b, D, D + N, D + 2 * N, D + 3 * N, D + 4 * N};
            return RSAC_OK;
        }
        if (ncomp_a == 3)
            HIPCHK(launch_pnp_prepare((const double *)a, (const double *)b, N, D, D + N, D + 2 * N, D + 3 * N,
                                      D + 4 * N, s));
        else
            HIPCHK(launch_hom_prepare((const double *)a, (const double *)b, N, D, D + N, D + 2 * N, D + 3 * N, s));
        return RSAC_OK;
    }
    // host float64 AoS -> float32 SoA (the CV_32F conversion of OpenCV), pinned, one H2D copy
    HIPCHK(hipEventSynchronize(c->ev_pts));
    HIPCHK(c->h_pts.ensure(sizeof(float) * nc * std::max<int64_t>(N, 1)));
    float *H = c->h_pts.as<float>();
    const double *A = (const double *)a, *B = (const double *)b;
    auto convert = [&](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            for (int k = 0; k < ncomp_a; ++k) H[k * N + i] = (float)A[ncomp_a * i + k];
            H[ncomp_a * N + i] = (float)B[2 * i];
            H[(ncomp_a + 1) * N + i] = (float)B[2 * i + 1];
        }
    };
    // large batches (C3 handed over as host arrays: 2M points) convert in chunks on the host pool
    // (converting and copying in slices, the copies overlapping the conversion, measured no
    // faster within the host's run-to-run spread: DESIGN.md §6)
    constexpr int64_t kChunk = 16384;
    if (N > 4 * kChunk)
        parallel_for((int)((N + kChunk - 1) / kChunk),
                     [&](int ch) { convert(ch * kChunk, std::min<int64_t>(N, (int64_t)(ch + 1) * kChunk)); });
    else
        convert(0, N);
    HIPCHK(hipMemcpyAsync(D, H, sizeof(float) * nc * N, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(c->ev_pts, s));
    for (int k = 0; k < nc; ++k) st.h[k] = H + k * N;
    st.host_ready = true;
    return RSAC_OK;
}

// host copy of the staged SoA (needed by refits / the MWC homography check)
int ensure_host_points(Staged &st, int nc, hipStream_t s) {
    if (st.host_ready) return RSAC_OK;
    const int64_t N = st.total;
    st.hbuf.resize(std::max<int64_t>(nc * N, 1));
    for (int k = 0; k < nc; ++k) {
        HIPCHK(hipMemcpyAsync(st.hbuf.data() + k * N, st.d[k], sizeof(float) * N, hipMemcpyDeviceToHost, s));
        st.h[k] = st.hbuf.data() + k * N;
    }
    HIPCHK(hipStreamSynchronize(s));
    st.host_ready = true;
    return RSAC_OK;
}

// small per-problem tables, one H2D copy: offsets (int64 P+1), cams (P x fx fy cx cy, f64),
// thr2 (f32, findInliers' float t = (float)(thresh*thresh))
int stage_tables(rsac_ctx *c, const Staged &st, const double *K, double thresh, hipStream_t s) {
    const int P = st.P;
    auto al = [](size_t b) { return (b + 15) & ~size_t(15); };
    const size_t off_b = al(sizeof(int64_t) * (P + 1)), cam_b = al(sizeof(double) * 4 * P), thr_b = al(sizeof(float) * P);
    const size_t tot = off_b + cam_b + thr_b;
    HIPCHK(c->tables.ensure(tot));
    // the same tables as the previous call (a bench or a multi-GPU driver step): no upload
    std::vector<char> &prev = c->last_tables;
    const bool same_buf = c->last_tables_dev == c->tables.p && prev.size() == tot;
    HIPCHK(hipEventSynchronize(c->ev_small));
    HIPCHK(c->h_small.ensure(tot));
    char *hs = c->h_small.as<char>();
    memcpy(hs, st.off.data(), sizeof(int64_t) * (P + 1));
    double *hc = (double *)(hs + off_b);
    for (int p = 0; p < P; ++p) {
        if (K) {
            const double *k = K + 9 * p;
            hc[4 * p] = k[0]; hc[4 * p + 1] = k[4]; hc[4 * p + 2] = k[2]; hc[4 * p + 3] = k[5];
        } else {
            hc[4 * p] = hc[4 * p + 1] = 1.0; hc[4 * p + 2] = hc[4 * p + 3] = 0.0;
        }
    }
    float *ht = (float *)(hs + off_b + cam_b);
    const float t2 = (float)(thresh * thresh);
    for (int p = 0; p < P; ++p) ht[p] = t2;
    char *d = c->tables.as<char>();
    if (!(same_buf && memcmp(prev.data(), hs, tot) == 0)) {
        HIPCHK(hipMemcpyAsync(d, hs, tot, hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(c->ev_small, s));
        prev.assign(hs, hs + tot);
        c->last_tables_dev = c->tables.p;
    }
    c->d_off = (int64_t *)d;
    c->d_cams = (double *)(d + off_b);
    c->d_thr2 = (float *)(d + off_b + cam_b);
    return RSAC_OK;
}

int ensure_hyp_buffers(rsac_ctx *c, int P, int64_t stride, bool subsets) {
    const size_t recs = (size_t)P * (size_t)stride;
    if (recs * kModelStride * sizeof(double) > kMaxModelBytes)
        return fail(RSAC_ENOMEM, "%lld hypothesis records exceed the resident budget", (long long)recs);
    HIPCHK(c->models.ensure(recs * kModelStride * sizeof(double)));
    HIPCHK(c->fmodels.ensure(recs * kFModelStride * sizeof(float)));
    HIPCHK(c->status.ensure(recs));
    HIPCHK(c->counts.ensure(recs * sizeof(int32_t)));
    HIPCHK(c->best.ensure(sizeof(int64_t) * P));
    HIPCHK(c->bestmodels.ensure(sizeof(double) * kModelStride * P));
    HIPCHK(c->h_best.ensure(sizeof(int64_t) * P));
    HIPCHK(c->h_bestmodels.ensure(sizeof(double) * kModelStride * P));
    if (subsets) {
        HIPCHK(c->subsets.ensure(recs * 5 * sizeof(int32_t)));  // up to 5 indices per sample
        HIPCHK(c->substatus.ensure(recs));
        HIPCHK(c->h_subsets.ensure(recs * 5 * sizeof(int32_t)));
        HIPCHK(c->h_substatus.ensure(recs));
    }
    return RSAC_OK;
}

hipStream_t pick_stream(rsac_ctx *c, void *stream) { return stream ? (hipStream_t)stream : c->stream; }

// PnpArgs for a staged problem set, with the float32 pre-filter frame built
// on the device (unless RSAC_F_EXACT_ONLY).  Call after stage_tables and
// ensure_hyp_buffers.
// defer_setup: a one-problem P3P call's set-up (converted device inputs, k_pnp_setup_fc) is left to
// the first solve launch (c->pending_setup), which runs it beside the solve (k_pnp_setup_solve4);
// the caller launches nothing that reads the points, the frame or the queue before that solve, or
// calls flush_setup.
// no_frame: no frame launch at all (the distorted paths: exact scoring only, nothing reads the
// frame, the key or the queue; the points must not be a deferred conversion)
// reuse / made (rsac_pnp_evaluate_range): `made` describes this call's set-up inputs; when it
// equals `reuse`, the previous call's record, with the same scratch buffers, the set-up is not
// launched (a.key_reset: the solve launch that must follow resets the key)
int pnp_args(rsac_ctx *c, const Staged &st, uint32_t flags, uint64_t seed, int64_t stride, int64_t rng_base,
             hipStream_t s, PnpArgs &a, unsigned long long *best_key = nullptr, bool defer_setup = false,
             bool no_frame = false, const SetupRecord *reuse = nullptr, SetupRecord *made = nullptr) {
    c->pending_on = false;
    c->setup_rec.valid = false;
    a = PnpArgs{};
    a.X = st.d[0]; a.Y = st.d[1]; a.Z = st.d[2]; a.U = st.d[3]; a.V = st.d[4];
    a.offsets = c->d_off;
    a.max_n = st.max_n();
    a.cams = c->d_cams;
    a.thr2 = c->d_thr2;
    a.models = c->models.as<double>();
    a.status = c->status.as<int8_t>();
    a.hyp_stride = stride;
    a.rng_base = rng_base;
    a.seed = seed;
    a.best_key = best_key;
    const int P = st.P;
    const int64_t N = st.total;
    HIPCHK(c->queue.ensure(4096));  // kQWords ints (rsac_kernels.hip)
    HIPCHK(c->bounds_ws.ensure(sizeof(int32_t) * 10 * P));
    HIPCHK(c->frame.ensure(sizeof(double) * kFrameStride * P));
    HIPCHK(c->fconst.ensure(sizeof(float) * kFconstStride * P));
    a.queue = c->queue.as<int>();
    a.exact_only = (flags & RSAC_F_EXACT_ONLY) ? 1 : 0;
    a.sample_k = (flags & RSAC_F_MINIMAL_EPNP5) ? 5 : 4;  // EPnP-5: ensure_epnp5 before each solve
    a.rvec_rt = (flags & RSAC_F_RVEC_ROUNDTRIP) ? 1 : 0;
    a.dbg_cell_pts = c->dbg_cell_pts;
    const int32_t max_n = a.max_n;
    // resets best_key and the queue, then builds the frame (also in exact mode: cheap)
    // one problem: k_pnp_setup_fc's scratch (its ticket starts at 0; the kernel resets it)
    if (!a.exact_only) {  // the MFMA scorer's point operands, written with the centring
        HIPCHK(c->mxpts.ensure(40 * std::max<int64_t>(N, 1)));
        a.PF = c->mxpts.as<uint4>();
        a.UV = reinterpret_cast<float2 *>(c->mxpts.as<char>() + 32 * std::max<int64_t>(N, 1));
    }
    PnpPrepare prep = st.prep;
    if (P == 1) {
        if (!c->setup_scr.p) {
            HIPCHK(c->setup_scr.ensure(64 + sizeof(float) * 10 * kSetupMaxBlocks));
            HIPCHK(hipMemsetAsync(c->setup_scr.p, 0, 64, s));
        }
        prep.ticket = c->setup_scr.as<int>();
        prep.part = (float *)(c->setup_scr.as<char>() + 64);
    }
    if (defer_setup && P == 1 && a.sample_k == 4 && !a.exact_only && !(flags & RSAC_F_LO) && prep.p3 && prep.part &&
        prep.ticket && max_n <= 65536) {
        c->pending_setup = PnpSetupFuse{prep, max_n, c->bounds_ws.as<int32_t>(), c->frame.as<double>(),
                                        c->fconst.as<float>()};
        c->pending_on = true;
    } else if (no_frame) {
        if (!a.exact_only || prep.p3) return fail(RSAC_EINVAL, "internal: frameless set-up needs staged points");
    } else {
        // made: the caller's description of this set-up's inputs, completed here with the buffers
        // it writes; valid for the one-problem device-f64 launch (k_pnp_setup_fc<true>) alone
        if (made && P == 1 && prep.p3 && prep.part && prep.ticket && max_n <= 65536) {
            const void *bufs[8] = {c->pts.p, a.PF, c->bounds_ws.p, c->frame.p, c->fconst.p, c->tables.p,
                                   c->queue.p, c->setup_scr.p};
            const uint64_t gens[8] = {c->pts.gen, c->mxpts.gen, c->bounds_ws.gen, c->frame.gen, c->fconst.gen,
                                      c->tables.gen, c->queue.gen, c->setup_scr.gen};
            memcpy(made->buf, bufs, sizeof bufs);
            memcpy(made->gen, gens, sizeof gens);
            made->valid = true;
        }
        if (reuse && made && made->same(*reuse) && best_key && pnp_setup_reuse_built()) {
            // every output of the set-up is still in place: no launch; the solve's first thread
            // resets the key (and, as always, the unit queue); the ticket stays 0
            a.key_reset = best_key;
            c->setup_reused = true;
        } else {
            HIPCHK(launch_pnp_frame(a, P, max_n, c->bounds_ws.as<int32_t>(), nullptr, nullptr, nullptr,
                                    c->frame.as<double>(), c->fconst.as<float>(), s, &prep));
        }
    }
    if (!a.exact_only) {
        a.counts_out = c->counts.as<int32_t>();
        a.frame = c->frame.as<double>();
        a.fconst = c->fconst.as<float>();
        a.fmodels = c->fmodels.as<float>();
        a.fform = 2;  // MFMA records (form 1 for small rounds and out-of-f16-range problems)
    }
    return RSAC_OK;
}

// Lens distortion (DESIGN.md "Lens distortion").  parse_dist: (dist, n_dist) of the ABI -> the eight
// coefficients, missing ones zero; n_dist 0 / dist NULL = none; 4, 5 or 8 accepted (12 and 14, the
// thin-prism and tilt models, are not built).  active: some coefficient is non-zero (all-zero
// coefficients take the pinhole path, bit for bit).
int parse_dist(const double *dist, int32_t n_dist, DistK &kd, bool &active) {
    memset(&kd, 0, sizeof kd);
    active = false;
    if (!dist || n_dist == 0) return RSAC_OK;
    if (n_dist == 12 || n_dist == 14)
        return fail(RSAC_EINVAL, "%d distortion coefficients (thin prism / tilt) are not supported: 4, 5 or 8", n_dist);
    if (n_dist != 4 && n_dist != 5 && n_dist != 8)
        return fail(RSAC_EINVAL, "bad distortion coefficient count %d: 4, 5 or 8", n_dist);
    for (int i = 0; i < n_dist; ++i) {
        kd.k[i] = dist[i];
        active = active || dist[i] != 0.0;
    }
    return RSAC_OK;
}

// the opening of a _dist entry point: the coefficients, then the flags no distorted path takes
// (host-only entry points pass flags 0)
int parse_dist_for(const char *what, const double *dist, int32_t n_dist, uint32_t flags, DistK &kd, bool &active) {
    if (int r = parse_dist(dist, n_dist, kd, active)) return r;
    if (active && (flags & (RSAC_F_DEVICE_SOA | RSAC_F_ASYNC)))
        return fail(RSAC_EINVAL, "%s: RSAC_F_DEVICE_SOA and RSAC_F_ASYNC are not supported with lens distortion", what);
    return RSAC_OK;
}

// MSAC costs are in units of thr2 = (float)(thr * thr), which must be a positive finite float
int check_msac_thr(const char *what, double thr) {
    const float t2 = (float)(thr * thr);
    if (!(t2 > 0.f && t2 <= 3.402823466e38f)) return fail(RSAC_EINVAL, "%s needs a finite positive threshold", what);
    return RSAC_OK;
}

// one staged problem (points already f32 on the device): every point undistorted once into the
// ideal pixels a.Uu / a.Vu, the coefficients left on the device for the scoring and mask launches
int dist_setup(rsac_ctx *c, const Staged &st, const double *K, const DistK &kd, int32_t n_dist, PnpArgs &a,
               hipStream_t s) {
    if (st.P != 1) return fail(RSAC_EINVAL, "lens distortion: one problem per call");
    const int64_t N = std::max<int64_t>(st.total, 1);
    HIPCHK(c->distbuf.ensure(64 + sizeof(float) * 2 * N));
    double *dk = c->distbuf.as<double>();
    float *Uu = (float *)(c->distbuf.as<char>() + 64), *Vu = Uu + N;
    const double cam[4] = {K[0], K[4], K[2], K[5]};
    HIPCHK(launch_pnp_undistort(st.d[3], st.d[4], nullptr, st.total, cam, kd, Uu, Vu, nullptr, nullptr, dk, s));
    a.dist = dk;
    a.n_dist = n_dist;
    a.Uu = Uu;
    a.Vu = Vu;
    return RSAC_OK;
}

// the deferred set-up alone (a path that does not start with a fusable P3P solve)
int flush_setup(rsac_ctx *c, const PnpArgs &a, hipStream_t s) {
    if (!c->pending_on) return RSAC_OK;
    c->pending_on = false;
    const PnpSetupFuse &f = c->pending_setup;
    HIPCHK(launch_pnp_frame(a, 1, f.max_n, f.ws, nullptr, nullptr, nullptr, f.frame, f.fconst, s, &f.prep));
    return RSAC_OK;
}

// the EPnP-5 solve's scratch for launches of up to P x H hypotheses (kEpnpRec doubles each, at
// launch-local positions: one round's worth, not one per hypothesis record), within the resident
// budget; a no-op for P3P
int ensure_epnp5(rsac_ctx *c, PnpArgs &a, int32_t P, int64_t H) {
    if (a.sample_k != 5) return RSAC_OK;
    const size_t bytes = (size_t)std::max(P, 1) * (size_t)std::max<int64_t>(H, 1) * kEpnpRec * sizeof(double);
    if (bytes > kMaxModelBytes)
        return fail(RSAC_ENOMEM, "EPnP-5 scratch for %lld hypotheses exceeds the resident budget",
                    (long long)P * (long long)H);
    HIPCHK(c->epnp5.ensure(bytes));
    a.epnp = c->epnp5.as<double>();
    return RSAC_OK;
}

// HomArgs (homography and fundamental matrix) for a staged problem set.  Call after stage_tables
// and ensure_hyp_buffers.  subsets: the solve reads c->subsets / c->substatus (run_loop points it
// at each round's rows itself)
HomArgs hom_args(rsac_ctx *c, const Staged &st, uint64_t seed, int64_t rng_base, int64_t stride, bool subsets) {
    HomArgs a{};
    a.SX = st.d[0]; a.SY = st.d[1]; a.DX = st.d[2]; a.DY = st.d[3];
    a.offsets = c->d_off;
    a.max_n = st.max_n();
    a.thr2 = c->d_thr2;
    a.models = c->models.as<double>();
    a.status = c->status.as<int8_t>();
    a.subsets = subsets ? c->subsets.as<int32_t>() : nullptr;
    a.sub_status = subsets ? c->substatus.as<int8_t>() : nullptr;
    a.hyp_stride = stride;
    a.rng_base = rng_base;
    a.seed = seed;
    return a;
}

// fundamental matrix: the f32 Sampson pre-filter's records and coordinate bounds (unless
// RSAC_F_EXACT_ONLY, which keeps the all-f64 scoring kernel).  Call after ensure_hyp_buffers.
int fm_prefilter(rsac_ctx *c, HomArgs &a, int32_t P, uint32_t flags, hipStream_t s) {
    if (flags & RSAC_F_EXACT_ONLY) return RSAC_OK;
    HIPCHK(c->bounds_ws.ensure(sizeof(int32_t) * 10 * P));  // >= 8 per problem
    a.fmodels = c->fmodels.as<float>();
    a.fbounds = c->bounds_ws.as<int>();
    HIPCHK(c->queue.ensure(4096));  // kQWords ints (rsac_kernels.hip)
    a.fm_queue = c->queue.as<int>() + 8;  // its own counter (the PnP kernels use word 0)
    HIPCHK(launch_fm_bounds(a, P, a.max_n, c->bounds_ws.as<int>(), s));
    return RSAC_OK;
}

enum class Model { PnP, Hom, Fm };  // Fm: fundamental matrix on the HomArgs block
constexpr int kFmBatchMaxP = 65535;  // the batched fundamental-matrix calls: a problem is a grid row (blockIdx.y)

// RSAC_F_FM_7POINT belongs to the fundamental-matrix RANSAC / LMedS drivers and probes alone
int reject_fm7(const char *what, uint32_t flags) {
    if (flags & RSAC_F_FM_7POINT) return fail(RSAC_EINVAL, "%s does not take RSAC_F_FM_7POINT", what);
    return RSAC_OK;
}

// Essential mode: an internal bit, never a public flag.  The essential drivers add it
// after their own flag check, and with it Model::Fm samples 5 points (k_em_solve_g5 over c->em_kinv)
// and owns kEm5Records records per sample; the fundamental-matrix entry points turn it away.
constexpr uint32_t kFlagEm5 = 1u << 31;
int reject_em5(const char *what, uint32_t flags) {
    if (flags & kFlagEm5) return fail(RSAC_EINVAL, "%s: unknown flag bit 31", what);
    return RSAC_OK;
}

// The RANSAC loop of RANSACPointSetRegistrator::run for P problems at once:
// rounds of `round` hypotheses are solved + scored on the GPU, then every
// unfinished problem's scan consumes them in index order.
struct LoopOut {
    std::vector<ScanState> scan;
    std::vector<int64_t> best_cost;  // RSAC_F_MSAC: the cost of scan[p].best (-1: none), scan_step_msac's state
    int rounds = 0;
    int64_t scored = 0;
    double gpu_ms = 0, solve_ms = 0, score_ms = 0;
    int32_t lo_improvements = 0;
    // speculative first round (run_loop with a ScanDecide): the records are on their way to
    // the host and the device has picked the winner; spec_resolve replays and verifies
    bool spec_pending = false;
    ScanFuse fuse;  // a pending speculative PnP scan: the finish's mask launch runs it (k_scan_mask)
    int64_t spec_H = 0;
    bool timing = true;  // HIP events around solve / score (the caller wants rsac_stats)
    // OpenCV's sampler: one MWC state per problem, carried across rounds and across the resume of a
    // speculative first round
    std::vector<Mwc> rngs;
    // records per sample (records_per_sample): scan[p].iter / best and `scored` count records,
    // scan[p].niters counts samples
    int rps = 1;
};

// every problem's scan at its start, with a budget of H hypotheses
void reset_scans(LoopOut &lo, int P, int64_t H) {
    lo.scan.assign(P, ScanState());
    for (auto &sc : lo.scan) sc.reset((int)H);
    lo.best_cost.assign(P, -1);
}

// a call's rsac_stats: problem 0's scan and the loop's totals
void fill_stats(rsac_stats &o, const LoopOut &lo) {
    o = rsac_stats{};
    o.best_hyp = lo.scan[0].best;
    o.iters = lo.scan[0].iter / lo.rps;  // samples consumed; best_hyp stays the record index
    o.hyps_scored = lo.scored;
    o.n_inliers = lo.scan[0].max_good;
    o.rounds = lo.rounds;
    o.gpu_ms = lo.gpu_ms;
    o.solve_ms = lo.solve_ms;
    o.score_ms = lo.score_ms;
    o.lo_improvements = lo.lo_improvements;
}

// LO-RANSAC local optimisation of the new best of problem 0 (DESIGN.md "LO-RANSAC";
// the oracle's orc_pnp_ransac_lo): up to 4 rounds of LM refit on the current inliers +
// recount, kept while the count rises.  An improved model replaces the best
// hypothesis' record, so the final mask / gather / refit see it.
constexpr int kLoSteps = 4;

// the multi-block LM refit's scratch (rsac_internal.h LmScratch; granules zeroed once here),
// the device's co-resident block limit for it, and the pinned failure word
LmScratch *lm_scratch(rsac_ctx *c, hipStream_t s) {
    if (!c->lmscr.p) {
        if (c->lmscr.ensure(kLmGranuleBytes) != hipSuccess) return nullptr;
        if (hipMemsetAsync(c->lmscr.p, 0, kLmGranuleBytes, s) != hipSuccess) return nullptr;
        if (c->h_lmfail.ensure(sizeof(int32_t)) != hipSuccess) return nullptr;
        *c->h_lmfail.as<int32_t>() = 0;
        c->lm.gran = (unsigned long long *)c->lmscr.p;
        c->lm.fail = c->h_lmfail.as<int32_t>();
        c->lm.launch = 0;
        int coop = 0;
        const char *ev = getenv("RSAC_REFIT_COOP");
        if (hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, c->device) == hipSuccess)
            c->lm.coop = coop && ev && ev[0] == '1';  // opt-in: +25 us on C2 ms-to-best (scripts/refit_coop_ab.py)
    }
    if (c->lm.max_blocks == 0) {
        c->lm.max_blocks = pnp_refine_coresident(c->device);
        if (c->dbg_refit_max_blocks > 0) c->lm.max_blocks = std::min(c->lm.max_blocks, c->dbg_refit_max_blocks);
    }
    return &c->lm;
}

// after the synchronisation that follows refits: a multi-block refit whose range sums never
// all arrived (its blocks were not all co-resident: other work held the CUs for longer than the
// kernel's ~1 s wait) kept the start pose and set the failure word.  The caller then redoes the
// call with one block per refit (with_one_refit_block), which needs no co-residency and gives
// the same bits.
constexpr int kRetryOneBlock = -1000;  // internal: not an RSAC_* code, never returned to callers
int lm_check(rsac_ctx *c) {
    int32_t *f = c->h_lmfail.as<int32_t>();
    if (f && __atomic_load_n(f, __ATOMIC_ACQUIRE)) {
        *f = 0;
        if (c->lm.max_blocks > 1) return kRetryOneBlock;
        return fail(RSAC_EHIP, "pose refit: a single-block LM refit lost its own range sums");
    }
    return RSAC_OK;
}

// run `call` (an API body); when one of its multi-block refits failed for lack of co-residency,
// run it again with every refit on one block
template <class F>
int with_one_refit_block(rsac_ctx *c, F call) {
    int r = call();
    if (r != kRetryOneBlock) return r;
    const int saved = c->lm.max_blocks;
    c->lm.max_blocks = 1;
    c->lo_state_base = nullptr;  // an LO chain's device state starts from zero again
    r = call();
    c->lm.max_blocks = saved;
    return r == kRetryOneBlock ? fail(RSAC_EHIP, "pose refit failed with one block") : r;
}

// The kLoSteps steps are enqueued at once and decided on the device (k_pnp_lo_count): step k
// refits record src_k on mask k into rec[(k + 1) % 2], recounts it, and either makes it the best
// (copied over the best hypothesis' record) or ends the chain, after which the remaining
// launches are no-ops.  One synchronisation per LO call; the state comes back in pinned memory.
int local_opt(rsac_ctx *c, const PnpArgs &a, int32_t n, ScanState &sc, double confidence, hipStream_t s,
              int32_t &improvements) {
    const size_t rec_bytes = sizeof(double) * kModelStride;
    HIPCHK(c->lo.ensure(2 * rec_bytes + 64 + 2 * (size_t)std::max(n, 1)));
    HIPCHK(c->h_lo.ensure(sizeof(LoState)));
    double *rec[2] = {c->lo.as<double>(), c->lo.as<double>() + kModelStride};
    LoState *st = (LoState *)(rec[1] + kModelStride);
    uint8_t *mk[2] = {(uint8_t *)st + 64, (uint8_t *)st + 64 + std::max(n, 1)};
    if (c->lo_state_base != c->lo.p) {  // count and ticket must start at 0 (then self-resetting)
        HIPCHK(hipMemsetAsync(st, 0, sizeof(LoState), s));
        c->lo_state_base = c->lo.p;
    }
    LoState *hst = c->h_lo.as<LoState>();
    double *best_rec = a.models + sc.best * kModelStride;  // problem 0: record index = hypothesis
    HIPCHK(launch_pnp_lo_count(a, n, best_rec, mk[0], st, -1, sc.max_good, nullptr, hst, s));
    for (int step = 0; step < kLoSteps; ++step) {
        const double *src = step == 0 ? best_rec : rec[step & 1];
        double *dst = rec[(step + 1) & 1];
        HIPCHK(launch_pnp_refine(a, 1, mk[step & 1], dst, nullptr, s, lm_scratch(c, s), nullptr, nullptr, src,
                                 &st->stopped));
        HIPCHK(launch_pnp_lo_count(a, n, dst, mk[(step + 1) & 1], st, step, 0, best_rec, hst, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (int r = lm_check(c)) return r;
    improvements += hst->improvements;
    if (hst->improvements > 0 && hst->cur > sc.max_good) {
        sc.max_good = hst->cur;
        sc.niters = update_num_iters(confidence, (double)(n - hst->cur) / n, a.sample_k, (int)sc.niters);
        if (sc.iter >= sc.niters) sc.done = true;
    }
    return RSAC_OK;
}

void add_times(rsac_ctx *c, double &gpu, double &solve, double &score) {
    float a = 0, b = 0;
    if (hipEventElapsedTime(&a, c->ev0, c->ev1) == hipSuccess) solve += a;
    if (hipEventElapsedTime(&b, c->ev1, c->ev2) == hipSuccess) score += b;
    gpu += (double)a + (double)b;
}

// OpenCV's subset sequence, drawn on the host: hypotheses [hb, hb + Hr) of every problem's row of
// c->h_subsets / c->h_substatus from the problem's MWC state (problems in parallel).  A problem
// with fewer than sk points, or that `skip` names, draws nothing: its statuses are -1, which the
// solve kernels pass over.  The caller uploads the rows.
template <class Skip>
void draw_mwc_rows(rsac_ctx *c, const Staged &st, Model model, std::vector<Mwc> &rngs, Skip skip, int64_t hb,
                   int64_t Hr, int64_t stride, int sk) {
    int32_t *hs = c->h_subsets.as<int32_t>();
    int8_t *hss = c->h_substatus.as<int8_t>();
    parallel_for(st.P, [&](int p) {
        int8_t *os = hss + (size_t)p * stride + hb;
        const int np = (int)(st.off[p + 1] - st.off[p]);
        if (np < sk || skip(p)) {
            memset(os, -1, Hr);
            return;
        }
        const float *hom[4];
        if (model == Model::Hom)
            for (int k = 0; k < 4; ++k) hom[k] = st.h[k] + st.off[p];
        mwc_subsets(rngs[p], np, Hr, model == Model::Hom ? hom : nullptr, hs + ((size_t)p * stride + hb) * sk, os, sk);
    });
}

// caller-supplied subsets of one n-point problem (H x sk indices): a subset with an index out of
// range gets status -1, the table and the statuses go to c->subsets / c->substatus
int upload_subsets(rsac_ctx *c, const int32_t *subsets, int32_t H, int sk, int32_t n, hipStream_t s) {
    int8_t *hss = c->h_substatus.as<int8_t>();
    memcpy(c->h_subsets.p, subsets, sizeof(int32_t) * sk * (size_t)H);
    for (int32_t h = 0; h < H; ++h) {
        bool ok = true;
        for (int j = 0; j < sk; ++j) ok = ok && subsets[sk * h + j] >= 0 && subsets[sk * h + j] < n;
        hss[h] = ok ? 1 : -1;
    }
    HIPCHK(hipMemcpyAsync(c->subsets.p, c->h_subsets.p, sizeof(int32_t) * sk * (size_t)H, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->substatus.p, hss, H, hipMemcpyHostToDevice, s));
    return RSAC_OK;
}

// hypotheses [hb, hb + Hr) of every problem's counts and statuses (and MSAC costs) -> the packed
// rows of c->h_counts / c->h_status (/ c->h_costs), Hr per problem; returns synchronised
int fetch_round_rows(rsac_ctx *c, int P, int64_t hb, int64_t Hr, int64_t stride, bool with_costs, hipStream_t s) {
    HIPCHK(copy_rows(c->h_counts.p, sizeof(int32_t) * Hr, c->counts.as<int32_t>() + hb, sizeof(int32_t) * stride,
                     sizeof(int32_t) * Hr, P, hipMemcpyDeviceToHost, s));
    HIPCHK(copy_rows(c->h_status.p, Hr, c->status.as<int8_t>() + hb, stride, Hr, P, hipMemcpyDeviceToHost, s));
    if (with_costs)
        HIPCHK(copy_rows(c->h_costs.p, sizeof(int64_t) * Hr, c->costs.as<int64_t>() + hb, sizeof(int64_t) * stride,
                         sizeof(int64_t) * Hr, P, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RSAC_OK;
}

// the count scan of the problems in `full` over their fetched rows (a first round whose
// improvements did not fit the device's scan records)
void scan_full_rows(rsac_ctx *c, const Staged &st, std::vector<ScanState> &scan, const std::vector<int> &full,
                    int64_t Hr, int model_points, double confidence, int rps = 1) {
    for (int p : full) {
        const int np = (int)(st.off[p + 1] - st.off[p]);
        scan_step(scan[p], c->h_counts.as<int32_t>() + (size_t)p * Hr, c->h_status.as<int8_t>() + (size_t)p * Hr, Hr,
                  np, model_points, confidence, false, rps);
    }
}

// RANSACUpdateNumIters' model_points = the sample size (5 for the EPnP-5 minimal solver, 7 for the
// fundamental matrix under RSAC_F_FM_7POINT)
int sample_size(Model, const PnpArgs &a, uint32_t) { return a.sample_k; }
int sample_size(Model model, const HomArgs &, uint32_t flags) {
    return model == Model::Fm ? ((flags & kFlagEm5) ? 5 : (flags & RSAC_F_FM_7POINT) ? 7 : 8) : 4;
}
int fm_sample_size(uint32_t flags) { return (flags & kFlagEm5) ? 5 : (flags & RSAC_F_FM_7POINT) ? 7 : 8; }
// the hypothesis records a sample owns: the 7-point solver's up to three models
int records_per_sample(Model model, uint32_t flags) {
    if (model == Model::Fm && (flags & kFlagEm5)) return kEm5Records;
    return model == Model::Fm && (flags & RSAC_F_FM_7POINT) ? kFm7Records : 1;
}
// the fundamental-matrix solve of a round or a probe: sample_k 5 is the essential drivers' (kFlagEm5)
hipError_t fm_solve(rsac_ctx *c, const HomArgs &a, int32_t P, int64_t hyp_begin, int32_t H, hipStream_t s, int sk) {
    if (sk == 5) return launch_em_solve_g5(a, c->em_kinv.as<double>(), P, hyp_begin, H, s);
    return launch_fm_solve(a, P, hyp_begin, H, s, sk);
}

// one round's solve and scoring launches, the timing events around them
int launch_round(rsac_ctx *c, Model, PnpArgs &a, int P, int64_t hb, int64_t Hr, bool msac, bool timing,
                 hipStream_t s, int) {
    // the deferred set-up beside the round's solve; the scorer then builds the records
    const bool fused = c->pending_on && P == 1 && pnp_setup_fusable(a, (int32_t)Hr);
    if (fused) {
        c->pending_on = false;
        HIPCHK(launch_pnp_solve(a, P, hb, Hr, s, &c->pending_setup));
    } else {
        if (int r = flush_setup(c, a, s)) return r;
        HIPCHK(launch_pnp_solve(a, P, hb, Hr, s));
    }
    if (timing) HIPCHK(hipEventRecord(c->ev1, s));
    a.fm_inline = fused ? 1 : 0;
    const hipError_t se = msac ? launch_pnp_cost(a, P, hb, Hr, c->counts.as<int32_t>(), c->costs.as<int64_t>(), s)
                               : launch_pnp_score(a, P, hb, Hr, c->counts.as<int32_t>(), s);
    a.fm_inline = 0;
    HIPCHK(se);
    return RSAC_OK;
}

int launch_round(rsac_ctx *c, Model model, HomArgs &a, int P, int64_t hb, int64_t Hr, bool msac, bool timing,
                 hipStream_t s, int sk) {
    HIPCHK(model == Model::Fm ? fm_solve(c, a, P, hb, Hr, s, sk) : launch_hom_solve(a, P, hb, Hr, s));
    if (timing) HIPCHK(hipEventRecord(c->ev1, s));
    int32_t *counts = c->counts.as<int32_t>();
    int64_t *costs = c->costs.as<int64_t>();
    if (model == Model::Fm)
        HIPCHK(msac ? launch_fm_cost(a, P, hb, Hr, counts, costs, s) : launch_fm_score(a, P, hb, Hr, counts, s));
    else
        HIPCHK(msac ? launch_hom_cost(a, P, hb, Hr, counts, costs, s) : launch_hom_score(a, P, hb, Hr, counts, s));
    return RSAC_OK;
}

// a: the PnpArgs (Model::PnP) or HomArgs (Model::Hom, Model::Fm) of the staged problems; the loop
// points its record, status and subset fields at the context's buffers
template <class Args>
int run_loop(rsac_ctx *c, Model model, const Staged &st, Args &a, int32_t max_iters, double confidence,
             uint32_t flags, hipStream_t s, LoopOut &out, const ScanDecide *spec = nullptr, bool resume = false,
             int max_rounds = 0) {
    constexpr bool is_pnp = std::is_same<Args, PnpArgs>::value;
    const int P = st.P;
    // rps records per sample: max_iters and the scans' bounds count samples, everything else here
    // (H, the rounds, the buffers) counts records, and a round is a whole number of samples
    const int rps = records_per_sample(model, flags);
    out.rps = rps;
    const auto whole = [rps](int64_t v) { return (v + rps - 1) / rps * rps; };
    const int64_t H = (int64_t)std::max(max_iters, 1) * rps;
    const bool adaptive = (flags & RSAC_F_ADAPTIVE) != 0;
    const bool lo = (flags & RSAC_F_LO) != 0 && model == Model::PnP && P == 1;
    // MSAC (DESIGN.md "MSAC scoring"): k_pnp_cost / k_hom_cost / k_fm_cost score, and every round's
    // status, counts and costs go to the host scan (no device scan records, no speculative finish),
    // as LO's rounds do
    const bool msac = (flags & RSAC_F_MSAC) != 0;
    const int64_t round = adaptive ? std::min<int64_t>(whole(std::max<int64_t>(c->round_size, 64)), H) : H;
    const int64_t stride = H;
    int r = ensure_hyp_buffers(c, P, stride, (flags & RSAC_F_SAMPLER_OPENCV) != 0);
    if (r) return r;
    HIPCHK(c->h_counts.ensure(sizeof(int32_t) * P * round));
    HIPCHK(c->h_status.ensure((size_t)P * round));
    if (msac) {
        HIPCHK(c->costs.ensure(sizeof(int64_t) * (size_t)P * stride));
        HIPCHK(c->h_costs.ensure(sizeof(int64_t) * P * round));
    }

    if constexpr (is_pnp) {  // a round is at most `round` hypotheses of each problem
        r = ensure_epnp5(c, a, P, round);
        if (r) return r;
    }
    const int model_points = sample_size(model, a, flags);
    const int sk = model_points;  // indices per drawn subset
    // OpenCV's subset sequence is sequential in one MWC state per problem and call: the
    // states persist across rounds, each round's slice is drawn on the host (problems in
    // parallel) and uploaded before its solve
    const bool opencv = (flags & RSAC_F_SAMPLER_OPENCV) != 0;
    std::vector<Mwc> &rngs = out.rngs;
    if (opencv && !resume) rngs.assign(P, Mwc());
    a.models = c->models.as<double>();
    a.status = c->status.as<int8_t>();
    a.hyp_stride = stride;
    a.subsets = opencv ? c->subsets.as<int32_t>() : nullptr;
    a.sub_status = opencv ? c->substatus.as<int8_t>() : nullptr;

    // adaptive: the first round is short (most runs stop within it), later ones double
    int64_t cur = adaptive ? std::min<int64_t>(round, whole(256)) : round;
    int64_t hb0 = 0;
    if (resume) {  // after a verified speculative first round (OpenCV's sampler: out.rngs carries on)
        hb0 = out.spec_H;
        cur = std::min<int64_t>(cur * 2, round);
    } else {
        reset_scans(out, P, H / rps);
    }
    for (int64_t hb = hb0, Hr = 0; hb < H; hb += Hr) {
        if (max_rounds > 0 && out.rounds >= max_rounds) break;  // the caller goes on (first-round mode)
        Hr = std::min<int64_t>(cur, H - hb);
        cur = std::min<int64_t>(cur * 2, round);
        if (opencv) {
            draw_mwc_rows(c, st, model, rngs, [&](int p) { return out.scan[p].done; }, hb, Hr, stride, sk);
            // a small round's subsets are read by the solve straight from the pinned host rows (no
            // copy launches in the latency path: an adaptive run's first round); larger rounds go
            // to the device in two copies.  Either way the host rewrites the rows only after the
            // round's synchronisation.
            const int32_t *hs = c->h_subsets.as<int32_t>();
            const int8_t *hss = c->h_substatus.as<int8_t>();
            const bool zero_copy = (int64_t)P * Hr * (4 * sk + 1) <= kSubsetZeroCopyBytes;
            a.subsets = zero_copy ? hs : c->subsets.as<int32_t>();
            a.sub_status = zero_copy ? hss : c->substatus.as<int8_t>();
            if (!zero_copy) {
                HIPCHK(copy_rows(c->subsets.as<int32_t>() + hb * sk, sizeof(int32_t) * sk * stride, hs + hb * sk,
                                 sizeof(int32_t) * sk * stride, sizeof(int32_t) * sk * Hr, P, hipMemcpyHostToDevice,
                                 s));
                HIPCHK(copy_rows(c->substatus.as<int8_t>() + hb, stride, hss + hb, stride, Hr, P,
                                 hipMemcpyHostToDevice, s));
            }
        }
        if (out.timing) HIPCHK(hipEventRecord(c->ev0, s));
        r = launch_round(c, model, a, P, hb, Hr, msac, out.timing, s, sk);
        if (r) return r;
        if (out.timing) HIPCHK(hipEventRecord(c->ev2, s));
        // the first round without LO: the device lists each problem's scan improvements
        // (prefix-maximum records) and the host replays the exact scan on them; later rounds (and
        // LO) copy every count
        std::vector<int> full;  // problems scanned from their full count / status rows
        if (!lo && !msac && hb == 0) {
            HIPCHK(c->h_scanrec.ensure(sizeof(ScanRecords) * P));
            // a speculative one-problem PnP round: the finish's mask launch replays the scan itself
            // (k_scan_mask), one launch fewer in front of the refit.  (Batches keep the two launches:
            // every mask block of every problem replaying its problem's scan made C3's scan + masks
            // 39 us against 21, r05.)
            const bool fuse = spec && P == 1 && model == Model::PnP && scan_mask_fusable((int32_t)Hr);
            if (fuse) {
                out.fuse = ScanFuse{true, c->counts.as<int32_t>(), c->status.as<int8_t>(), stride, (int32_t)Hr,
                                    model_points, c->h_scanrec.as<ScanRecords>(), *spec};
            } else if (P == 1) {
                // one problem: the kernel writes its record straight into pinned host memory (no
                // copy launch); many problems: device records and one copy (thousands of scattered
                // 4-byte writes over PCIe cost more than the copy)
                HIPCHK(launch_scan_records(c->counts.as<int32_t>(), c->status.as<int8_t>(), stride, P, (int32_t)Hr,
                                           model_points, c->h_scanrec.as<ScanRecords>(), s,
                                           spec ? *spec : ScanDecide()));
            } else {
                HIPCHK(c->scanrec.ensure(sizeof(ScanRecords) * P));
                HIPCHK(launch_scan_records(c->counts.as<int32_t>(), c->status.as<int8_t>(), stride, P, (int32_t)Hr,
                                           model_points, c->scanrec.as<ScanRecords>(), s,
                                           spec ? *spec : ScanDecide()));
                // a speculative finish: copied behind the finish's mask kernel (issue_scanrec_copy),
                // which would otherwise wait for the copy
                if (spec)
                    c->scanrec_copy = P;
                else
                    HIPCHK(hipMemcpyAsync(c->h_scanrec.p, c->scanrec.p, sizeof(ScanRecords) * P,
                                          hipMemcpyDeviceToHost, s));
            }
            if (spec) {  // no synchronisation: the caller enqueues the finish, then spec_resolve
                out.spec_pending = true;
                out.spec_H = Hr;
                return RSAC_OK;
            }
            HIPCHK(hipStreamSynchronize(s));
            const ScanRecords *rec = c->h_scanrec.as<ScanRecords>();
            for (int p = 0; p < P; ++p) {
                if (rec[p].nrec < 0) {
                    full.push_back(p);
                    continue;
                }
                const int np = (int)(st.off[p + 1] - st.off[p]);
                scan_records(out.scan[p], rec[p].idx, rec[p].cnt, rec[p].nrec, rec[p].first_neg, (int64_t)Hr, np,
                             model_points, confidence, false, rps);  // the first round: the scan starts at 0
            }
            if (!full.empty()) {
                r = fetch_round_rows(c, P, hb, Hr, stride, false, s);
                if (r) return r;
                scan_full_rows(c, st, out.scan, full, Hr, model_points, confidence, rps);
            }
            if (out.timing) add_times(c, out.gpu_ms, out.solve_ms, out.score_ms);
            out.rounds++;
            out.scored += (int64_t)Hr;
            bool all_done = true;
            for (int p = 0; p < P; ++p) all_done = all_done && out.scan[p].done;
            if (all_done) break;
            continue;  // later rounds copy their counts
        }
        r = fetch_round_rows(c, P, hb, Hr, stride, msac, s);
        if (r) return r;
        if (out.timing) add_times(c, out.gpu_ms, out.solve_ms, out.score_ms);
        out.rounds++;
        out.scored += (int64_t)Hr;
        bool all_done = true;
        if (msac) {  // the cost scan, problems in parallel (each touches only its own state)
            parallel_for(P, [&](int p) {
                if (out.scan[p].done) return;
                const int np = (int)(st.off[p + 1] - st.off[p]);
                scan_step_msac(out.scan[p], out.best_cost[p], c->h_counts.as<int32_t>() + (size_t)p * Hr,
                               c->h_costs.as<int64_t>() + (size_t)p * Hr, c->h_status.as<int8_t>() + (size_t)p * Hr,
                               Hr, np, model_points, confidence, rps);
            });
            for (int p = 0; p < P; ++p) all_done = all_done && out.scan[p].done;
            if (all_done) break;
            continue;
        }
        for (int p = 0; p < P; ++p) {
            ScanState &sc = out.scan[p];
            const int np = (int)(st.off[p + 1] - st.off[p]);
            const int32_t *cr = c->h_counts.as<int32_t>() + (size_t)p * Hr;
            const int8_t *sr = c->h_status.as<int8_t>() + (size_t)p * Hr;
            if (lo) {
                // stop at every new best, optimise it locally, continue with the raised floor
                while (!sc.done && sc.iter < hb + Hr) {
                    scan_step(sc, cr + (sc.iter - hb), sr + (sc.iter - hb), hb + Hr - sc.iter, np, model_points,
                              confidence, true);
                    if (sc.improved) {
                        sc.improved = false;
                        if constexpr (is_pnp) r = local_opt(c, a, np, sc, confidence, s, out.lo_improvements);
                        if (r) return r;
                    }
                }
            } else if (!sc.done) {
                scan_step(sc, cr, sr, Hr, np, model_points, confidence, false, rps);
            }
            all_done = all_done && sc.done;
        }
        if (all_done) break;
    }
    return RSAC_OK;
}

// the deferred copy of a speculative round's device scan records to the host (run_loop)
hipError_t issue_scanrec_copy(rsac_ctx *c, hipStream_t s) {
    if (!c->scanrec_copy) return hipSuccess;
    const size_t bytes = sizeof(ScanRecords) * c->scanrec_copy;
    c->scanrec_copy = 0;
    return hipMemcpyAsync(c->h_scanrec.p, c->scanrec.p, bytes, hipMemcpyDeviceToHost, s);
}

// after the stream synchronised: the host's replay of a speculative first round (one problem).
// ok: it ended the scan with the winner the device picked (the finish enqueued on the device's
// pick is the result); otherwise the caller starts over without speculation.
int spec_resolve(rsac_ctx *c, const Staged &st, LoopOut &out, int model_points, double confidence, bool &ok,
                 bool fixed, int64_t stride, hipStream_t s) {
    const int P = fixed ? st.P : 1;
    if (c->scanrec_copy) {  // not yet issued by a finish: copy and wait here
        HIPCHK(issue_scanrec_copy(c, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    const ScanRecords *recs = c->h_scanrec.as<ScanRecords>();
    out.spec_pending = false;
    ok = false;
    if (!fixed && (recs[0].nrec < 0 || c->dbg_spec_overflow)) {  // more improvements than records: the caller runs the loop afresh
        out.scan[0].reset((int)out.scan[0].niters);
        out.spec_H = 0;
        return RSAC_OK;
    }
    std::vector<int> full;  // problems with more improvements than records: their full rows
    for (int p = 0; p < P; ++p) {
        const ScanRecords &rec = recs[p];
        if (rec.nrec < 0) {
            full.push_back(p);
            continue;
        }
        const int np = (int)(st.off[p + 1] - st.off[p]);
        scan_records(out.scan[p], rec.idx, rec.cnt, rec.nrec, rec.first_neg, out.spec_H, np, model_points,
                     confidence, false, out.rps);
    }
    if (!full.empty()) {
        const int64_t Hr = out.spec_H;
        HIPCHK(c->h_counts.ensure(sizeof(int32_t) * P * Hr));
        HIPCHK(c->h_status.ensure((size_t)P * Hr));
        if (int r = fetch_round_rows(c, P, 0, Hr, stride, false, s)) return r;
        scan_full_rows(c, st, out.scan, full, Hr, model_points, confidence, out.rps);
    }
    if (out.timing) add_times(c, out.gpu_ms, out.solve_ms, out.score_ms);
    out.rounds = 1;
    out.scored = out.spec_H;
    ok = true;
    for (int p = 0; p < P; ++p) {
        const ScanRecords &rec = recs[p];
        // (fixed budget: the round was the whole budget, whether or not the scan flagged it done)
        ok = ok && (fixed || out.scan[p].done) && rec.dev_done && out.scan[p].best == (int64_t)rec.dev_best;
    }
    return RSAC_OK;
}

// masks + winning models of every problem; records of winners -> c->best
// defer_sync: leave the stream running (the caller enqueues more work, synchronises, then
// calls finish_masks_host to copy a host mask out)
// dev_best: the winners' record indices are already on the device (c->best, a speculative
// first round), not in lo
int finish_masks(rsac_ctx *c, Model model, const Staged &st, void *args, const LoopOut &lo, int64_t stride,
                 uint8_t *mask_out, uint32_t flags, hipStream_t s, bool defer_sync = false, bool dev_best = false) {
    const int P = st.P;
    int64_t *hb = c->h_best.as<int64_t>();
    for (int p = 0; p < P; ++p) hb[p] = lo.scan[p].best >= 0 ? (int64_t)p * stride + lo.scan[p].best : -1;
    // one problem: the record index goes as a kernel argument (no upload)
    const int64_t *dbest = P == 1 && !dev_best ? nullptr : c->best.as<int64_t>();
    if (P > 1 && !dev_best)
        HIPCHK(hipMemcpyAsync(c->best.p, hb, sizeof(int64_t) * P, hipMemcpyHostToDevice, s));
    const int64_t N = st.total;
    // PnP: the mask kernel also gathers the winners' records (one launch fewer)
    const bool fused_gather = model == Model::PnP && N > 0;
    if (!fused_gather)
        HIPCHK(launch_gather_models(c->models.as<double>(), dbest, P, c->bestmodels.as<double>(), s, hb[0]));
    const int32_t max_n = st.max_n();
    uint8_t *dmask;
    if (flags & RSAC_F_DEVICE_OUT) {
        dmask = mask_out;
    } else {
        HIPCHK(c->mask.ensure(std::max<int64_t>(N, 1)));
        dmask = c->mask.as<uint8_t>();
    }
    if (N > 0) {
        // without a refit the winners also go straight to the pinned host records
        double *hmodels = defer_sync ? nullptr : c->h_bestmodels.as<double>();
        if (model == Model::PnP && dev_best && lo.fuse.pending)  // the speculative round's scan, then the masks
            HIPCHK(launch_scan_mask(lo.fuse, *(PnpArgs *)args, P, max_n, dmask, c->bestmodels.as<double>(), hmodels,
                                    s));
        else if (model == Model::PnP)
            HIPCHK(launch_pnp_mask(*(PnpArgs *)args, P, max_n, dbest, dmask, s, hb[0], c->bestmodels.as<double>(),
                                   hmodels));
        else if (model == Model::Fm)
            HIPCHK(launch_fm_mask(*(HomArgs *)args, P, max_n, dbest, dmask, s, hb[0]));
        else
            HIPCHK(launch_hom_mask(*(HomArgs *)args, P, max_n, dbest, dmask, s, hb[0]));
    }
    HIPCHK(issue_scanrec_copy(c, s));
    // the winners' records for the host (a refit copies the refined ones instead)
    if (!defer_sync && !(model == Model::PnP && N > 0))
        HIPCHK(hipMemcpyAsync(c->h_bestmodels.p, c->bestmodels.p, sizeof(double) * kModelStride * P,
                              hipMemcpyDeviceToHost, s));
    if (!(flags & RSAC_F_DEVICE_OUT) && mask_out && N > 0) {
        HIPCHK(c->h_mask.ensure(N));
        HIPCHK(hipMemcpyAsync(c->h_mask.p, dmask, N, hipMemcpyDeviceToHost, s));
        if (defer_sync) return RSAC_OK;
        HIPCHK(hipStreamSynchronize(s));
        memcpy(mask_out, c->h_mask.p, N);
    } else if (!defer_sync) {
        HIPCHK(hipStreamSynchronize(s));
    }
    return RSAC_OK;
}

// after a deferred finish_masks and a stream synchronisation: the host mask copy-out
void finish_masks_host(rsac_ctx *c, const Staged &st, uint8_t *mask_out, uint32_t flags) {
    if (!(flags & RSAC_F_DEVICE_OUT) && mask_out && st.total > 0) memcpy(mask_out, c->h_mask.p, st.total);
}

int check_device(rsac_ctx *c) {
    if (!c) return fail(RSAC_EINVAL, "null context");
    HIPCHK(hipSetDevice(c->device));
    return RSAC_OK;
}

// where a call's masks are on the device: the caller's buffer (RSAC_F_DEVICE_OUT) or c->mask
bool mask_in_caller_buffer(const uint8_t *mask_out, uint32_t flags) { return (flags & RSAC_F_DEVICE_OUT) && mask_out; }
uint8_t *device_mask_ptr(rsac_ctx *c, uint8_t *mask_out, uint32_t flags) {
    return mask_in_caller_buffer(mask_out, flags) ? mask_out : c->mask.as<uint8_t>();
}

// mask for refits when the caller wanted the mask on the device (or not at all)
int host_mask(rsac_ctx *c, const Staged &st, uint8_t *mask_out, uint32_t flags, hipStream_t s,
              std::vector<uint8_t> &tmp, const uint8_t **hm) {
    if (mask_out && !(flags & RSAC_F_DEVICE_OUT)) {
        *hm = mask_out;
        return RSAC_OK;
    }
    tmp.resize(std::max<int64_t>(st.total, 1));
    HIPCHK(hipMemcpyAsync(tmp.data(), device_mask_ptr(c, mask_out, flags), st.total, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *hm = tmp.data();
    return RSAC_OK;
}

// the winners' masks, then the final solve on the device, one block per problem, on the
// RANSAC-phase inliers: EPnP (solvePnPRansac with SOLVEPNP_P3P), then / or LM
// (solvePnPRefineLM); returns with the stream synchronised and c->h_bestmodels filled.
// dev_best: the winners come from the device's speculative replay (c->best)
int pnp_finish(rsac_ctx *c, const Staged &st, const PnpArgs &a, const LoopOut &lo, int64_t stride, const double *K,
               uint8_t *mask_out, uint32_t flags, hipStream_t s, bool refit, bool dev_best) {
    const int P = st.P;
    int r = finish_masks(c, Model::PnP, st, (void *)&a, lo, stride, mask_out, flags, s, refit, dev_best);
    if (r || !refit) return r;
    const uint8_t *dmask = device_mask_ptr(c, mask_out, flags);
    if (flags & RSAC_F_EPNP) {
        // stage 1 (sums) on the device, stage 2 (12 x 12 eigenvectors + betas, O(1)) on the
        // host, stage 3 (pose candidates) on the device
        const size_t b1 = sizeof(EpnpStage1) * P, b2 = sizeof(EpnpStage2) * P;
        HIPCHK(c->epnp.ensure(b1 + b2));
        HIPCHK(c->h_epnp.ensure(b1 + b2));
        EpnpStage1 *d1 = c->epnp.as<EpnpStage1>(), *h1 = c->h_epnp.as<EpnpStage1>();
        EpnpStage2 *d2 = (EpnpStage2 *)(d1 + P), *h2 = (EpnpStage2 *)(h1 + P);
        HIPCHK(launch_pnp_epnp_s1(a, P, dmask, c->bestmodels.as<double>(), d1, s));
        HIPCHK(hipMemcpyAsync(h1, d1, b1, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        parallel_for(P, [&](int p) {
            const double *Kp = K + 9 * p;
            if (h1[p].ok != 0.0) epnp_stage2(h1[p], Cam{Kp[0], Kp[4], Kp[2], Kp[5]}, h2[p]);
            else memset(&h2[p], 0, sizeof(EpnpStage2));
        });
        HIPCHK(hipMemcpyAsync(d2, h2, b2, hipMemcpyHostToDevice, s));
        HIPCHK(launch_pnp_epnp_s3(a, P, dmask, d1, d2, c->bestmodels.as<double>(), s));
    }
    if (flags & RSAC_F_REFINE)  // the refit also writes R, t into the pinned host records
        HIPCHK(launch_pnp_refine(a, P, dmask, c->bestmodels.as<double>(), nullptr, s, lm_scratch(c, s),
                                 st.off.data(), c->h_bestmodels.as<double>()));
    else
        HIPCHK(hipMemcpyAsync(c->h_bestmodels.p, c->bestmodels.p, sizeof(double) * kModelStride * P,
                              hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (flags & RSAC_F_REFINE)
        if (int r = lm_check(c)) return r;
    finish_masks_host(c, st, mask_out, flags);
    return RSAC_OK;
}

// OpenCV's `count == model_points` branches ([OpenCV, unvendored] solvepnp.cpp solvePnPRansac,
// fundam.cpp findHomography; reached from main_v1.py:497-502, testpro-K.py:72-75, main_v1.py:312):
// no RANSAC.  The minimal kernel runs once on all the points in input order (no subset check), the
// result is its model with every index an inlier, and there is no final solve (no LM / EPnP refit,
// no homography LM).  PnP: 4 points -> P3P whatever the flags (model_points is 4 for
// SOLVEPNP_P3P / AP3P and for npoints == 4), 5 points under the default flags -> EPnP
// (model_points 5; RSAC_F_MINIMAL_EPNP5).  Homography: 4 points -> runKernel, method 0's path.
// A failed solve -> no model and no inliers.  kind[p] = the direct sample size of problem p, 0 for
// a RANSAC problem.
std::vector<int8_t> direct_kinds(const Staged &st, Model model, int sample_k, int &count) {
    std::vector<int8_t> kind(st.P, 0);
    count = 0;
    for (int p = 0; p < st.P; ++p) {
        const int64_t np = st.off[p + 1] - st.off[p];
        int8_t k = 0;
        if (model == Model::PnP)
            k = np == 4 ? 4 : (np == 5 && sample_k == 5) ? 5 : 0;
        else if (model == Model::Hom)
            k = np == 4 ? 4 : 0;
        kind[p] = k;
        count += k != 0;
    }
    return kind;
}

// the direct problems' minimal solves (one record per problem and kind, sample = 0 .. k-1 with
// status 1, every other problem status -1 so the kernels skip it), then k_direct_finish: their
// records -> c->bestmodels / the pinned c->h_bestmodels and their mask rows (dmask, device) set
// to 1 (model) or 0.  The caller synchronises, then reads the outcome with direct_apply.
int direct_solve(rsac_ctx *c, Model model, const Staged &st, const void *args, const std::vector<int8_t> &kind,
                 uint8_t *dmask, hipStream_t s) {
    const int P = st.P;
    // device layout: rec4, rec5 (P x kModelStride f64 each) | sub4 (P x 4), sub5 (P x 5) i32 |
    // sst4, sst5, st4, st5, kind (P i8 each)
    const size_t recb = sizeof(double) * kModelStride * P, subb = sizeof(int32_t) * 9 * P;
    const size_t bytes = 2 * recb + subb + 5 * (size_t)P;
    HIPCHK(c->direct.ensure(bytes));
    HIPCHK(c->h_direct.ensure(subb + 5 * (size_t)P));
    char *d = c->direct.as<char>();
    double *rec4 = (double *)d, *rec5 = rec4 + (size_t)kModelStride * P;
    int32_t *dsub4 = (int32_t *)(d + 2 * recb), *dsub5 = dsub4 + 4 * (size_t)P;
    int8_t *dsst4 = (int8_t *)(d + 2 * recb + subb), *dsst5 = dsst4 + P, *dst4 = dsst5 + P, *dst5 = dst4 + P,
           *dkind = dst5 + P;
    char *h = c->h_direct.as<char>();
    int32_t *hsub4 = (int32_t *)h, *hsub5 = hsub4 + 4 * (size_t)P;
    int8_t *hsst4 = (int8_t *)(h + subb), *hsst5 = hsst4 + P, *hkind = hsst5 + 3 * (size_t)P;
    bool any5 = false;
    for (int p = 0; p < P; ++p) {
        for (int j = 0; j < 4; ++j) hsub4[4 * p + j] = j;
        for (int j = 0; j < 5; ++j) hsub5[5 * p + j] = j;
        hsst4[p] = kind[p] == 4 ? 1 : -1;
        hsst5[p] = kind[p] == 5 ? 1 : -1;
        hkind[p] = kind[p];
        any5 = any5 || kind[p] == 5;
    }
    HIPCHK(hipMemcpyAsync(dsub4, h, subb + 2 * (size_t)P, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dkind, hkind, P, hipMemcpyHostToDevice, s));
    if (model == Model::PnP) {
        for (int k = 4; k <= 5; ++k) {
            if (k == 5 && !any5) break;
            PnpArgs ad = *(const PnpArgs *)args;
            ad.models = k == 4 ? rec4 : rec5;
            ad.status = k == 4 ? dst4 : dst5;
            ad.hyp_stride = 1;
            ad.subsets = k == 4 ? dsub4 : dsub5;
            ad.sub_status = k == 4 ? dsst4 : dsst5;
            ad.sample_k = k;
            ad.counts_out = nullptr;
            ad.fmodels = nullptr;
            ad.queue = nullptr;
            ad.best_key = nullptr;
            int r = ensure_epnp5(c, ad, P, 1);
            if (r) return r;
            HIPCHK(launch_pnp_solve(ad, P, 0, 1, s));
        }
    } else {
        HomArgs ad = *(const HomArgs *)args;
        ad.models = rec4;
        ad.status = dst4;
        ad.hyp_stride = 1;
        ad.subsets = dsub4;
        ad.sub_status = dsst4;
        HIPCHK(launch_hom_solve(ad, P, 0, 1, s));
    }
    HIPCHK(c->bestmodels.ensure(sizeof(double) * kModelStride * P));
    HIPCHK(c->h_bestmodels.ensure(sizeof(double) * kModelStride * P));
    HIPCHK(launch_direct_finish(rec4, rec5, dst4, dst5, dkind, c->d_off, P, c->bestmodels.as<double>(),
                                c->h_bestmodels.as<double>(), dmask, s));
    return RSAC_OK;
}

// after the synchronisation that follows direct_solve: the direct problems' scan states (best 0 or
// -1, every point or none an inlier, no iterations) and their rows of a host mask
void direct_apply(rsac_ctx *c, const Staged &st, const std::vector<int8_t> &kind, std::vector<ScanState> &scan,
                  uint8_t *host_mask) {
    const double *bm = c->h_bestmodels.as<double>();
    for (int p = 0; p < st.P; ++p) {
        if (!kind[p]) continue;
        const int np = (int)(st.off[p + 1] - st.off[p]);
        const bool ok = bm[(size_t)kModelStride * p + kValidSlot] != 0.0;
        ScanState &sc = scan[p];
        sc.best = ok ? 0 : -1;
        sc.max_good = ok ? np : 0;
        sc.iter = 0;
        sc.done = true;
        if (host_mask) memset(host_mask + st.off[p], ok ? 1 : 0, np);
    }
}

// the direct branch of a driver: the direct problems' models and device mask rows (the caller's
// buffer or c->mask), then, synchronised, their scan states and host mask rows
int run_direct(rsac_ctx *c, Model model, const Staged &st, const void *args, const std::vector<int8_t> &dkind,
               LoopOut &lo, uint8_t *mask_out, uint32_t flags, hipStream_t s) {
    const bool dev_mask = mask_in_caller_buffer(mask_out, flags);
    if (!dev_mask) HIPCHK(c->mask.ensure(std::max<int64_t>(st.total, 1)));
    int r = direct_solve(c, model, st, args, dkind, device_mask_ptr(c, mask_out, flags), s);
    if (r) return r;
    HIPCHK(hipStreamSynchronize(s));
    direct_apply(c, st, dkind, lo.scan, dev_mask ? nullptr : mask_out);
    return RSAC_OK;
}

// hom_refine of every staged problem over the device mask dmask (concatenated, NULL = all) by
// k_hom_fit, enqueued on s; the records (kHomFitRes doubles per problem) are then copied to
// c->h_homfit -- the caller synchronises before reading them.  More than one problem: after stage_tables.
int hom_fit_enqueue(rsac_ctx *c, const Staged &st, const uint8_t *dmask, hipStream_t s) {
    const size_t b = sizeof(double) * kHomFitRes * (size_t)st.P;
    HIPCHK(c->homfit.ensure(b));
    HIPCHK(c->h_homfit.ensure(b));
    HIPCHK(launch_hom_fit(st.d[0], st.d[1], st.d[2], st.d[3], st.P == 1 ? nullptr : c->d_off, st.P, (int32_t)st.total,
                          dmask, c->homfit.as<double>(), s));
    HIPCHK(hipMemcpyAsync(c->h_homfit.p, c->homfit.p, b, hipMemcpyDeviceToHost, s));
    return RSAC_OK;
}

// RSAC_F_REFINE of a homography driver fits on the device, from the mask where it lies, where
// that was measured faster than the host tail (rsac_internal.h): the location
// search (loc) and the larger batches, whatever the inputs' residence
bool hom_fit_on_device(const rsac_ctx *c, const Staged &st, uint32_t flags, bool loc) {
    if (!(flags & RSAC_F_REFINE)) return false;
    if (c->dbg_hom_fit) return c->dbg_hom_fit == 2;
    if (loc) return kHomFitLocationOnDevice;
    return st.P >= kHomFitDeviceMinP && st.total >= kHomFitDeviceMinMeanN * (int64_t)st.P;
}

// the host tail of the homography drivers: every problem's H (refitted on its inliers hm under
// RSAC_F_REFINE, more than 4 points), status and inlier count -> RSAC_OK, or RSAC_NO_MODEL when
// no problem has a model.  A problem without a model reports zeros (zero_no_model, LMedS) or its
// record of c->h_bestmodels (RANSAC: zeros from the gather, a failed direct solve's own record).
// best_median (LMedS): the RANSAC problems' best medians, for medians_out.
int hom_outputs(rsac_ctx *c, const Staged &st, const LoopOut &lo, uint32_t flags, const uint8_t *hm,
                bool zero_no_model, const std::vector<int8_t> &dkind, const double *best_median, double *H_out,
                int32_t *status_out, int32_t *ninl_out, double *medians_out, const double *dev_fit = nullptr) {
    const double *bm = c->h_bestmodels.as<double>();
    parallel_for(st.P, [&](int p) {
        const ScanState &sc = lo.scan[p];
        double Hm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        const bool ok = sc.best >= 0;
        const int64_t o = st.off[p];
        const int np = (int)(st.off[p + 1] - o);
        if (ok || !zero_no_model) memcpy(Hm, bm + kModelStride * p, sizeof Hm);
        if (ok && (flags & RSAC_F_REFINE) && np > 4) {
            double Hr[9];
            if (dev_fit) {  // the device's records (hom_fit_enqueue): the same bits
                if (dev_fit[(size_t)kHomFitRes * p + 9] != 0.0) memcpy(Hm, dev_fit + (size_t)kHomFitRes * p, sizeof Hm);
            } else if (hom_refine(st.h[0] + o, st.h[1] + o, st.h[2] + o, st.h[3] + o, hm + o, np, Hr)) {
                memcpy(Hm, Hr, sizeof Hm);
            }
        }
        if (H_out) memcpy(H_out + 9 * p, Hm, sizeof Hm);
        if (status_out) status_out[p] = ok ? RSAC_OK : RSAC_NO_MODEL;
        if (ninl_out) ninl_out[p] = sc.max_good;
        if (medians_out) medians_out[p] = !ok ? -1.0 : dkind[p] ? 0.0 : best_median[p];
    });
    int any = 0;
    for (int p = 0; p < st.P; ++p) any |= lo.scan[p].best >= 0;
    return any ? RSAC_OK : RSAC_NO_MODEL;
}

int pnp_core(rsac_ctx *c, const void *pts3d, const void *pts2d, const int64_t *offsets, int32_t P, int32_t n,
             const double *K, int32_t n_iters, double thr, double conf, uint64_t seed, uint32_t flags, double *R_out,
             double *t_out, int32_t *status_out, int32_t *ninl_out, uint8_t *mask_out, rsac_stats *stats,
             hipStream_t s, rsac_scan_state *first_round = nullptr, double *rows_dev = nullptr,
             const DistK *dist = nullptr, int32_t n_dist = 0) {
    // RSAC_DBG_PHASES=1: the host-side phases of every call on stderr (microseconds; a diagnostic)
    static const bool dbg_phases = [] {
        const char *e = getenv("RSAC_DBG_PHASES");
        return e && e[0] == '1';
    }();
    using dbg_clock = std::chrono::steady_clock;
    dbg_clock::time_point tp[6];
    auto mark = [&](int i) {
        if (dbg_phases) tp[i] = dbg_clock::now();
    };
    mark(0);
    int r = check_device(c);
    if (r) return r;
    if (P <= 0 || !K) return fail(RSAC_EINVAL, "bad problem count or K");
    if (int e = reject_fm7("PnP RANSAC", flags)) return e;
    // (first-round mode continues in the caller with model_points 4: P3P only)
    if (first_round &&
        (P != 1 || !(flags & RSAC_F_ADAPTIVE) || (flags & (RSAC_F_SAMPLER_OPENCV | RSAC_F_MINIMAL_EPNP5))))
        return fail(RSAC_EINVAL, "first-round mode: one problem, adaptive, Philox sampler, P3P");
    // lens distortion: exact scoring only, the points converted now (the undistort kernel reads
    // them), no frame and no fused set-up
    if (dist) flags |= RSAC_F_EXACT_ONLY;
    const bool msac = (flags & RSAC_F_MSAC) != 0;
    if (msac) {
        if (dist) return fail(RSAC_EINVAL, "RSAC_F_MSAC is not supported with lens distortion");
        if (flags & (RSAC_F_LO | RSAC_F_ASYNC))
            return fail(RSAC_EINVAL, "RSAC_F_MSAC cannot be combined with RSAC_F_LO or RSAC_F_ASYNC");
        if (first_round || rows_dev)
            return fail(RSAC_EINVAL, "RSAC_F_MSAC is honoured by rsac_pnp_ransac and rsac_pnp_ransac_batched only");
        r = check_msac_thr("RSAC_F_MSAC", thr);
        if (r) return r;
        flags |= RSAC_F_EXACT_ONLY;  // MSAC implies the all-f64 test (k_pnp_cost)
    }
    Staged st;
    r = stage_points(c, pts3d, pts2d, 3, offsets, P, n, flags, s, st, !dist);
    if (r) return r;
    r = stage_tables(c, st, K, thr, s);
    if (r) return r;
    const int64_t stride = std::max(n_iters, 1);
    r = ensure_hyp_buffers(c, P, stride, (flags & RSAC_F_SAMPLER_OPENCV) != 0);
    if (r) return r;
    PnpArgs a;
    // one P3P problem: the set-up runs inside the first solve launch (k_pnp_setup_solve4)
    r = pnp_args(c, st, flags, seed, stride, 0, s, a, nullptr, !dist, dist != nullptr);
    if (r) return r;
    if (dist) {
        r = dist_setup(c, st, K, *dist, n_dist, a, s);
        if (r) return r;
    }
    int n_direct = 0;  // problems of OpenCV's count == model_points branch (direct_kinds)
    const std::vector<int8_t> dkind = direct_kinds(st, Model::PnP, a.sample_k, n_direct);
    const bool all_direct = n_direct == P;
    if (all_direct || n_direct > 0) {  // the direct branch solves without run_loop
        r = flush_setup(c, a, s);
        if (r) return r;
    }
    // one adaptive problem: the device replays the first round's scan itself and the final mask
    // and refit are enqueued behind it, so the call synchronises once; the host verifies the
    // device's pick afterwards and redoes the call without speculation on a mismatch (a libm
    // ulp in RANSACUpdateNumIters) or when the first round did not end the scan
    // fixed budget (adaptive off, any number of problems): the one round covers every problem's
    // budget and the device replays every problem's scan, so the finish is enqueued behind the
    // scan the same way, with no host round trip in between
    const bool adaptive = (flags & RSAC_F_ADAPTIVE) != 0;
    const bool spec_fixed = !adaptive && !(flags & (RSAC_F_LO | RSAC_F_MSAC)) && st.total > 0;
    // (OpenCV's sampler too: its MWC state after the first round is kept in lo.rngs for the resume)
    const bool spec = spec_fixed || (P == 1 && adaptive && !(flags & (RSAC_F_LO | RSAC_F_MSAC)) && st.total > 0);
    ScanDecide dec;
    if (spec) {
        dec.best_out = c->best.as<int64_t>();
        dec.n = (int32_t)st.total;
        dec.max_iters = std::max(n_iters, 1);
        dec.confidence = conf;
        dec.fixed = spec_fixed ? 1 : 0;
        dec.offsets = spec_fixed ? c->d_off : nullptr;
    }
    LoopOut lo;
    lo.timing = stats != nullptr || c->timing;
    mark(1);
    // first-round mode (rsac_pnp_ransac_first_round): the loop stops after its first round when
    // that round did not end the scan; the caller continues from the exported scan state
    auto more = [&]() -> int {
        const ScanState &sc = lo.scan[0];
        *first_round = rsac_scan_state{sc.niters, sc.best, sc.iter, sc.max_good, sc.done ? 1 : 0};
        if (sc.best >= 0 && (R_out || t_out)) {  // the best record so far (LO: the optimised model)
            double m[kModelStride];
            HIPCHK(hipMemcpyAsync(m, c->models.as<double>() + (size_t)kModelStride * sc.best,
                                  sizeof(double) * kModelStride, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (R_out) memcpy(R_out, m, 9 * sizeof(double));
            if (t_out) memcpy(t_out, m + 9, 3 * sizeof(double));
        }
        if (ninl_out) ninl_out[0] = sc.max_good;
        if (stats) fill_stats(*stats, lo);  // the first round's figures (timing fields included)
        if (c->timing) fill_stats(c->last_stats, lo);
        return RSAC_MORE;
    };
    if (all_direct) {  // no RANSAC at all: run_direct below is the whole call
        reset_scans(lo, P, stride);
    } else {
    r = run_loop(c, Model::PnP, st, a, n_iters, conf, flags, s, lo, spec ? &dec : nullptr, false,
                 first_round ? 1 : 0);
    if (r == RSAC_OK) r = flush_setup(c, a, s);  // (a loop that launched no solve)
    c->pending_on = false;
    if (r) return r;
    if (first_round && !spec && !lo.scan[0].done) return more();
    mark(2);
    const bool refit = (flags & (RSAC_F_REFINE | RSAC_F_EPNP)) != 0;
    r = pnp_finish(c, st, a, lo, stride, K, mask_out, flags, s, refit, lo.spec_pending);
    if (r) return r;
    mark(3);
    if (lo.spec_pending) {
        bool ok = false;
        r = spec_resolve(c, st, lo, a.sample_k, conf, ok, spec_fixed, stride, s);
        if (r) return r;
        c->spec_finishes++;
        if (!ok) {
            c->spec_redos++;
            // the host's replay rules: later rounds if the scan goes on, then the finish again
            if (first_round && !lo.scan[0].done) {
                if (lo.spec_H == 0) {  // the replay started over: the first round without speculation
                    r = run_loop(c, Model::PnP, st, a, n_iters, conf, flags, s, lo, nullptr, false, 1);
                    if (r) return r;
                }
                if (!lo.scan[0].done) return more();
            }
            if (!spec_fixed && !lo.scan[0].done) {
                // resume after the verified first round; a replay that started over (spec_H = 0)
                // runs afresh, so OpenCV's MWC states restart with the scan
                r = run_loop(c, Model::PnP, st, a, n_iters, conf, flags, s, lo, nullptr, lo.spec_H > 0);
                if (r) return r;
            }
            r = pnp_finish(c, st, a, lo, stride, K, mask_out, flags, s, refit, false);
            if (r) return r;
        }
    }
    }  // !all_direct
    if (n_direct) {  // OpenCV's count == model_points problems: their minimal model, every point an inlier
        r = run_direct(c, Model::PnP, st, &a, dkind, lo, mask_out, flags, s);
        if (r) return r;
    }

    mark(4);
    const double *bm = c->h_bestmodels.as<double>();
    for (int p = 0; p < P; ++p) {
        const bool ok = lo.scan[p].best >= 0;
        if (R_out) memcpy(R_out + 9 * p, bm + kModelStride * p, 9 * sizeof(double));
        if (t_out) memcpy(t_out + 3 * p, bm + kModelStride * p + 9, 3 * sizeof(double));
        if (status_out) status_out[p] = ok ? RSAC_OK : RSAC_NO_MODEL;
        if (ninl_out) ninl_out[p] = lo.scan[p].max_good;
    }
    int any = 0;
    for (int p = 0; p < P; ++p) any |= lo.scan[p].best >= 0;
    if (msac) {  // the winners' costs (rsac_last_costs); the direct branch and "no model" report -1
        c->last_costs.assign(P, -1);
        for (int p = 0; p < P; ++p)
            if (!dkind[p] && lo.scan[p].best >= 0) c->last_costs[p] = lo.best_cost[p];
    } else {
        c->last_costs.clear();
    }
    if (rows_dev) {  // the result rows on the device (rsac_pnp_ransac_batched_rows)
        HIPCHK(c->h_rowinfo.ensure(sizeof(int64_t) * 2 * P));
        int64_t *info = c->h_rowinfo.as<int64_t>();
        for (int p = 0; p < P; ++p) {
            info[2 * p] = lo.scan[p].best;
            info[2 * p + 1] = lo.scan[p].max_good;
        }
        HIPCHK(launch_pnp_rows(info, c->bestmodels.as<double>(), P, rows_dev, s));
        HIPCHK(hipStreamSynchronize(s));  // h_rowinfo is reused by the next call
    }
    if (first_round) {  // the call ran to the end: the caller has rsac_pnp_ransac's result
        const ScanState &sc = lo.scan[0];
        *first_round = rsac_scan_state{sc.niters, sc.best, sc.iter, sc.max_good, 1};
    }
    if (c->timing) fill_stats(c->last_stats, lo);
    if (stats) fill_stats(*stats, lo);
    mark(5);
    if (dbg_phases) {
        auto us = [&](int i, int j) { return std::chrono::duration<double, std::micro>(tp[j] - tp[i]).count(); };
        fprintf(stderr, "rsac phases (us): setup %.1f loop %.1f finish %.1f resolve %.1f out %.1f total %.1f\n",
                us(0, 1), us(1, 2), us(2, 3), us(3, 4), us(4, 5), us(0, 5));
    }
    return any ? RSAC_OK : RSAC_NO_MODEL;
}

int hom_core(rsac_ctx *c, const void *src, const void *dst, const int64_t *offsets, int32_t P, int32_t n,
             int32_t max_iters, double thr, double conf, uint64_t seed, uint32_t flags, double *H_out,
             int32_t *status_out, int32_t *ninl_out, uint8_t *mask_out, rsac_stats *stats, hipStream_t s,
             bool loc = false) {
    int r = check_device(c);
    if (r) return r;
    if (P <= 0) return fail(RSAC_EINVAL, "bad problem count");
    if (int e = reject_fm7("homography RANSAC", flags)) return e;
    if (thr <= 0) thr = 3.0;  // defaultRANSACReprojThreshold of findHomography
    const bool msac = (flags & RSAC_F_MSAC) != 0;
    if (msac) {
        if (flags & (RSAC_F_LO | RSAC_F_ASYNC))
            return fail(RSAC_EINVAL, "RSAC_F_MSAC cannot be combined with RSAC_F_LO or RSAC_F_ASYNC");
        r = check_msac_thr("RSAC_F_MSAC", thr);
        if (r) return r;
    }
    Staged st;
    r = stage_points(c, src, dst, 2, offsets, P, n, flags, s, st);
    if (r) return r;
    r = stage_tables(c, st, nullptr, thr, s);
    if (r) return r;
    const bool dev_fit = hom_fit_on_device(c, st, flags, loc);
    if ((flags & RSAC_F_SAMPLER_OPENCV) || ((flags & RSAC_F_REFINE) && !dev_fit)) {
        r = ensure_host_points(st, 4, s);
        if (r) return r;
    }
    const int64_t stride = std::max(max_iters, 1);
    HomArgs a = hom_args(c, st, seed, 0, stride, false);
    LoopOut lo;  // (its timing stays on: the homography calls always time their rounds)
    int n_direct = 0;  // 4-point problems: findHomography's method-0 path (direct_kinds)
    const std::vector<int8_t> dkind = direct_kinds(st, Model::Hom, 4, n_direct);
    if (n_direct == P) {
        r = ensure_hyp_buffers(c, P, 1, false);
        if (r) return r;
        reset_scans(lo, P, stride);
    } else {
        r = run_loop(c, Model::Hom, st, a, max_iters, conf, flags, s, lo);
        if (r) return r;
        r = finish_masks(c, Model::Hom, st, &a, lo, stride, mask_out, flags, s);
        if (r) return r;
    }
    if (n_direct) {  // runKernel on the 4 points, mask all ones, no LM; rows of c->mask too (the
                     // location search scores every problem from it)
        r = run_direct(c, Model::Hom, st, &a, dkind, lo, mask_out, flags, s);
        if (r) return r;
    }
    std::vector<uint8_t> tmpmask;
    const uint8_t *hm = nullptr;
    if (dev_fit) {
        r = hom_fit_enqueue(c, st, device_mask_ptr(c, mask_out, flags), s);
        if (r) return r;
        HIPCHK(hipStreamSynchronize(s));
    } else if (flags & RSAC_F_REFINE) {
        r = host_mask(c, st, mask_out, flags, s, tmpmask, &hm);
        if (r) return r;
    }
    r = hom_outputs(c, st, lo, flags, hm, false, dkind, nullptr, H_out, status_out, ninl_out, nullptr,
                    dev_fit ? c->h_homfit.as<double>() : nullptr);
    if (msac) {  // the winners' costs (rsac_last_costs); the direct branch and "no model" report -1
        c->last_costs.assign(P, -1);
        for (int p = 0; p < P; ++p)
            if (!dkind[p] && lo.scan[p].best >= 0) c->last_costs[p] = lo.best_cost[p];
    }
    if (stats) fill_stats(*stats, lo);
    if (c->timing) fill_stats(c->last_stats, lo);  // rsac_set_timing: the batched call's figures too
    return r;
}

// flags outside `allowed` -> RSAC_EINVAL naming the first of them
int check_flags(const char *what, uint32_t flags, uint32_t allowed) {
    static const struct { uint32_t bit; const char *name; } names[] = {
        {RSAC_F_SAMPLER_OPENCV, "RSAC_F_SAMPLER_OPENCV"}, {RSAC_F_ADAPTIVE, "RSAC_F_ADAPTIVE"},
        {RSAC_F_REFINE, "RSAC_F_REFINE"}, {RSAC_F_DEVICE_IN, "RSAC_F_DEVICE_IN"},
        {RSAC_F_DEVICE_SOA, "RSAC_F_DEVICE_SOA"}, {RSAC_F_DEVICE_OUT, "RSAC_F_DEVICE_OUT"},
        {RSAC_F_EXACT_ONLY, "RSAC_F_EXACT_ONLY"}, {RSAC_F_LO, "RSAC_F_LO"}, {RSAC_F_ASYNC, "RSAC_F_ASYNC"},
        {RSAC_F_EPNP, "RSAC_F_EPNP"}, {RSAC_F_MINIMAL_EPNP5, "RSAC_F_MINIMAL_EPNP5"},
        {RSAC_F_RVEC_ROUNDTRIP, "RSAC_F_RVEC_ROUNDTRIP"}, {RSAC_F_MSAC, "RSAC_F_MSAC"},
        {RSAC_F_FM_7POINT, "RSAC_F_FM_7POINT"}};
    const uint32_t bad = flags & ~allowed;
    if (!bad) return RSAC_OK;
    for (const auto &nm : names)
        if (bad & nm.bit) return fail(RSAC_EINVAL, "%s does not take %s", what, nm.name);
    return fail(RSAC_EINVAL, "%s: unknown flag bits 0x%x", what, bad);
}

// The LMedS round the three LMedS drivers share: H hypotheses per problem (hypothesis stride H) --
// solve(), median() (launches on s, an RSAC_* code each), the statuses and medians to the host, the
// host scan of (status, median) into lo.scan[p] and best_median[p] for every problem but those
// skip(p) names, and the problems' thr2 = sigma^2 (lmeds_sigma at `model_points`; 0 without a
// model) uploaded to c->d_thr2.
template <class Solve, class Median, class Skip>
int lmeds_round(rsac_ctx *c, const Staged &st, int64_t H, int model_points, LoopOut &lo,
                std::vector<double> &best_median, hipStream_t s, Solve solve, Median median, Skip skip, int rps = 1) {
    lo.rps = rps;  // H = rps records for each of H / rps samples (the scan's budget)
    const int P = st.P;
    const size_t recs = (size_t)P * (size_t)H;
    const size_t med_b = (sizeof(double) * recs + 15) & ~size_t(15);
    HIPCHK(c->h_medians.ensure(med_b + sizeof(float) * P));
    float *hthr = (float *)(c->h_medians.as<char>() + med_b);
    for (int p = 0; p < P; ++p) hthr[p] = 0.f;
    HIPCHK(c->medians.ensure(sizeof(double) * recs));
    HIPCHK(c->h_status.ensure(recs));
    if (lo.timing) HIPCHK(hipEventRecord(c->ev0, s));
    if (int e = solve()) return e;
    if (lo.timing) HIPCHK(hipEventRecord(c->ev1, s));
    if (int e = median()) return e;
    if (lo.timing) HIPCHK(hipEventRecord(c->ev2, s));
    HIPCHK(hipMemcpyAsync(c->h_status.p, c->status.p, recs, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(c->h_medians.p, c->medians.p, sizeof(double) * recs, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (lo.timing) add_times(c, lo.gpu_ms, lo.solve_ms, lo.score_ms);
    lo.rounds = 1;
    lo.scored = H;
    parallel_for(P, [&](int p) {
        if (skip(p)) return;
        const int np = (int)(st.off[p + 1] - st.off[p]);
        LmedsScan sc;
        sc.reset(H / rps);
        scan_step_lmeds(sc, c->h_status.as<int8_t>() + (size_t)p * H, c->h_medians.as<double>() + (size_t)p * H, H,
                        rps);
        lo.scan[p].best = sc.best;
        lo.scan[p].iter = sc.iter;
        best_median[p] = sc.best_median;
        if (sc.best >= 0) {
            const double sigma = lmeds_sigma(sc.best_median, np, model_points);
            hthr[p] = (float)(sigma * sigma);
        }
    });
    HIPCHK(hipMemcpyAsync(c->d_thr2, hthr, sizeof(float) * P, hipMemcpyHostToDevice, s));
    return RSAC_OK;
}

// After the masks at those bounds (hm: the host's view of them): a problem's inlier count is the ones
// of its mask, and a winner with fewer than `min_count` of them is no model -- its mask is cleared on
// the host and (enqueued on s; the caller synchronises) on the device.  *cleared: whether any was.
template <class Skip>
int lmeds_count_masks(rsac_ctx *c, const Staged &st, const uint8_t *hm, int min_count, LoopOut &lo, uint8_t *mask_out,
                      uint32_t flags, hipStream_t s, Skip skip, bool *cleared) {
    const bool dev_mask = mask_in_caller_buffer(mask_out, flags);
    uint8_t *dmask = device_mask_ptr(c, mask_out, flags);
    *cleared = false;
    for (int p = 0; p < st.P; ++p) {
        if (skip(p)) continue;
        ScanState &sc = lo.scan[p];
        const int64_t o = st.off[p];
        const int np = (int)(st.off[p + 1] - o);
        int ones = 0;
        for (int i = 0; i < np; ++i) ones += hm[o + i] != 0;
        sc.max_good = sc.best >= 0 ? ones : 0;
        if (sc.best >= 0 && ones < min_count) {
            sc.best = -1;
            sc.max_good = 0;
            if (mask_out && !dev_mask) memset(mask_out + o, 0, np);
            if (np > 0) HIPCHK(hipMemsetAsync(dmask + o, 0, np, s));
            *cleared = true;
        }
    }
    return RSAC_OK;
}

// LMedS homography (DESIGN.md "LMedS homography"), beside hom_core with a round of its own in place of run_loop:
// one round of `niters` hypotheses per problem -- solve, k_hom_median, the host scan of (status,
// median), the problems' thr2 from their best medians, then the RANSAC path's mask / gather /
// direct branch / host refit.
int hom_lmeds_core(rsac_ctx *c, const void *src, const void *dst, const int64_t *offsets, int32_t P, int32_t n,
                   int32_t max_iters, double conf, uint64_t seed, uint32_t flags, double *H_out, int32_t *status_out,
                   int32_t *ninl_out, double *medians_out, uint8_t *mask_out, rsac_stats *stats, hipStream_t s) {
    int r = check_device(c);
    if (r) return r;
    if (P <= 0) return fail(RSAC_EINVAL, "bad problem count");
    r = check_flags("LMedS homography", flags,
                    RSAC_F_SAMPLER_OPENCV | RSAC_F_ADAPTIVE | RSAC_F_REFINE | RSAC_F_DEVICE_IN | RSAC_F_DEVICE_SOA |
                        RSAC_F_DEVICE_OUT);
    if (r) return r;
    if (!(conf > 0.0 && conf < 1.0)) return fail(RSAC_EINVAL, "confidence must lie in (0, 1), got %g", conf);
    if ((flags & RSAC_F_DEVICE_OUT) && !mask_out) return fail(RSAC_EINVAL, "RSAC_F_DEVICE_OUT needs mask_out");
    const bool opencv = (flags & RSAC_F_SAMPLER_OPENCV) != 0;
    const int64_t H = (flags & RSAC_F_ADAPTIVE) ? lmeds_num_iters(conf, 4, max_iters) : std::max(max_iters, 1);
    Staged st;
    r = stage_points(c, src, dst, 2, offsets, P, n, flags, s, st);
    if (r) return r;
    r = stage_tables(c, st, nullptr, 0.0, s);  // thr2 is written after the scan
    if (r) return r;
    // the tables on the device will differ from the staged ones: the next call uploads afresh
    c->last_tables.clear();
    c->last_tables_dev = nullptr;
    const bool dev_fit = hom_fit_on_device(c, st, flags, false);
    if (opencv || ((flags & RSAC_F_REFINE) && !dev_fit)) {
        r = ensure_host_points(st, 4, s);
        if (r) return r;
    }
    int n_direct = 0;  // 4-point problems: findHomography's method-0 path (direct_kinds)
    const std::vector<int8_t> dkind = direct_kinds(st, Model::Hom, 4, n_direct);
    const bool all_direct = n_direct == P;
    const int64_t stride = all_direct ? 1 : H;
    r = ensure_hyp_buffers(c, P, stride, opencv && !all_direct);
    if (r) return r;
    HomArgs a = hom_args(c, st, seed, 0, stride, opencv && !all_direct);
    LoopOut lo;
    lo.timing = stats != nullptr || c->timing;
    reset_scans(lo, P, H);
    std::vector<double> best_median(P, 0.0);
    const auto direct = [&](int p) { return dkind[p] != 0; };
    if (!all_direct) {
        if (opencv) {  // one MWC state per problem and call, as each cv2 call restarts OpenCV's RNG
            const size_t recs = (size_t)P * (size_t)H;
            lo.rngs.assign(P, Mwc());
            draw_mwc_rows(c, st, Model::Hom, lo.rngs, direct, 0, H, H, 4);
            HIPCHK(hipMemcpyAsync(c->subsets.p, c->h_subsets.p, sizeof(int32_t) * 4 * recs, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(c->substatus.p, c->h_substatus.p, recs, hipMemcpyHostToDevice, s));
        }
        r = lmeds_round(
            c, st, H, 4, lo, best_median, s,
            [&]() -> int { HIPCHK(launch_hom_solve(a, P, 0, (int32_t)H, s)); return RSAC_OK; },
            [&]() -> int { HIPCHK(launch_hom_median(a, P, 0, (int32_t)H, c->medians.as<double>(), s)); return RSAC_OK; },
            direct);
        if (r) return r;
        r = finish_masks(c, Model::Hom, st, &a, lo, stride, mask_out, flags, s);
        if (r) return r;
    }
    if (n_direct) {  // runKernel on the 4 points, mask all ones, no LM
        r = run_direct(c, Model::Hom, st, &a, dkind, lo, mask_out, flags, s);
        if (r) return r;
    }
    // the host's view of the masks: the inlier counts, the >= 4 rule, the refit
    std::vector<uint8_t> tmpmask;
    const uint8_t *hm = nullptr;
    r = host_mask(c, st, mask_out, flags, s, tmpmask, &hm);
    if (r) return r;
    bool cleared = false;
    r = lmeds_count_masks(c, st, hm, 4, lo, mask_out, flags, s, direct, &cleared);
    if (r) return r;
    if (cleared) HIPCHK(hipStreamSynchronize(s));
    if (dev_fit) {  // after the masks of the problems without a model are cleared
        r = hom_fit_enqueue(c, st, device_mask_ptr(c, mask_out, flags), s);
        if (r) return r;
        HIPCHK(hipStreamSynchronize(s));
    }
    r = hom_outputs(c, st, lo, flags, hm, true, dkind, best_median.data(), H_out, status_out, ninl_out, medians_out,
                    dev_fit ? c->h_homfit.as<double>() : nullptr);
    if (stats) fill_stats(*stats, lo);
    if (c->timing) fill_stats(c->last_stats, lo);
    return r;
}

// LMedS fundamental matrix (DESIGN.md "MSAC and LMedS for the fundamental matrix"): hom_lmeds_core's
// round for P problems of >= 9 points each -- solve, k_fm_median, the host scan of (status, median),
// every problem's thr2 = sigma^2 from its own best median and point count, then the count rule's
// masks at those bounds (finish_masks).  No direct branch, no refit; a problem succeeds iff its mask
// holds >= 8 ones.  offsets == NULL: rsac_fundamental_lmeds, one problem of n points (c->last_stats
// stays the PnP and homography drivers', as in rsac_fundamental_ransac; status_out / ninl_out
// unused); otherwise rsac_fundamental_lmeds_batched, which returns RSAC_OK when any problem has a
// model and leaves its figures in c->last_stats under rsac_set_timing.
int fm_lmeds_core(rsac_ctx *c, const void *pts1, const void *pts2, const int64_t *offsets, int32_t P, int32_t n,
                  int32_t max_iters, double conf, uint64_t seed, uint32_t flags, double *F_out, int32_t *status_out,
                  int32_t *ninl_out, double *medians_out, uint8_t *mask_out, rsac_stats *stats, hipStream_t s) {
    int r = check_device(c);
    if (r) return r;
    const bool batched = offsets != nullptr;
    r = check_flags(batched ? "rsac_fundamental_lmeds_batched" : "rsac_fundamental_lmeds", flags,
                    RSAC_F_ADAPTIVE | RSAC_F_DEVICE_IN | RSAC_F_DEVICE_SOA | RSAC_F_DEVICE_OUT | RSAC_F_FM_7POINT);
    if (r) return r;
    if (P < 1 || P > kFmBatchMaxP) return fail(RSAC_EINVAL, "bad problem count %d (1 .. %d)", P, kFmBatchMaxP);
    const int sk = fm_sample_size(flags);  // 8, or 7 under RSAC_F_FM_7POINT
    const int rps = records_per_sample(Model::Fm, flags);
    for (int p = 0; p < P; ++p) {
        const int64_t np = batched ? offsets[p + 1] - offsets[p] : n;
        if (np < sk + 1)
            return fail(RSAC_ETOOFEW, "the LMedS fundamental matrix needs >= %d correspondences (got %lld): its sigma "
                                      "divides by n - %d", sk + 1, (long long)np, sk);
    }
    if (!(conf > 0.0 && conf < 1.0)) return fail(RSAC_EINVAL, "confidence must lie in (0, 1), got %g", conf);
    if ((flags & RSAC_F_DEVICE_OUT) && !mask_out) return fail(RSAC_EINVAL, "RSAC_F_DEVICE_OUT needs mask_out");
    // H: the records of the round, rps for each of the budget's samples
    const int64_t H = (int64_t)((flags & RSAC_F_ADAPTIVE) ? lmeds_num_iters(conf, sk, max_iters) : std::max(max_iters, 1)) * rps;
    Staged st;
    r = stage_points(c, pts1, pts2, 2, offsets, P, n, flags, s, st);
    if (r) return r;
    r = stage_tables(c, st, nullptr, 0.0, s);  // thr2 is written after the scan
    if (r) return r;
    // the tables on the device will differ from the staged ones: the next call uploads afresh
    c->last_tables.clear();
    c->last_tables_dev = nullptr;
    r = ensure_hyp_buffers(c, P, H, false);
    if (r) return r;
    HomArgs a = hom_args(c, st, seed, 0, H, false);
    LoopOut lo;
    lo.timing = stats != nullptr || (batched && c->timing);
    reset_scans(lo, P, H / rps);
    std::vector<double> best_median(P, 0.0);
    const auto no_skip = [](int) { return false; };  // no direct branch: every problem takes the round
    r = lmeds_round(
        c, st, H, sk, lo, best_median, s,
        [&]() -> int { HIPCHK(launch_fm_solve(a, P, 0, (int32_t)H, s, sk)); return RSAC_OK; },
        [&]() -> int { HIPCHK(launch_fm_median(a, P, 0, (int32_t)H, c->medians.as<double>(), s)); return RSAC_OK; },
        no_skip, rps);
    if (r) return r;
    r = finish_masks(c, Model::Fm, st, &a, lo, H, mask_out, flags, s);
    if (r) return r;
    std::vector<uint8_t> tmpmask;
    const uint8_t *hm = nullptr;
    r = host_mask(c, st, mask_out, flags, s, tmpmask, &hm);
    if (r) return r;
    bool cleared = false;
    r = lmeds_count_masks(c, st, hm, sk, lo, mask_out, flags, s, no_skip, &cleared);
    if (r) return r;
    if (cleared) HIPCHK(hipStreamSynchronize(s));
    int any = 0;
    for (int p = 0; p < P; ++p) {
        const bool ok = lo.scan[p].best >= 0;
        any |= ok;
        if (F_out) {
            if (ok)
                memcpy(F_out + 9 * (size_t)p, c->h_bestmodels.as<double>() + (size_t)kModelStride * p, 9 * sizeof(double));
            else
                memset(F_out + 9 * (size_t)p, 0, 9 * sizeof(double));
        }
        if (status_out) status_out[p] = ok ? RSAC_OK : RSAC_NO_MODEL;
        if (ninl_out) ninl_out[p] = lo.scan[p].max_good;
        if (medians_out) medians_out[p] = ok ? best_median[p] : -1.0;
    }
    if (stats) fill_stats(*stats, lo);
    if (batched && c->timing) fill_stats(c->last_stats, lo);
    return any ? RSAC_OK : RSAC_NO_MODEL;
}

// launch_pnp_median with the context's key rows: problems past the block kernel's register capacity
// get a scratch of up to kLmedsKeyBytes (RSAC_DBG_LMEDS_KEYS: another budget, or none = recompute)
constexpr int64_t kLmedsKeyBytes = 256ll << 20;
int pnp_median_launch(rsac_ctx *c, const PnpArgs &a, int32_t P, int32_t H, hipStream_t s) {
    uint32_t *scr = nullptr;
    int64_t keys = 0;
    if (a.max_n > kPnpMedianBlockCap && c->dbg_lmeds_keys >= 0) {
        const int64_t budget = (c->dbg_lmeds_keys > 0 ? c->dbg_lmeds_keys : kLmedsKeyBytes) / (int64_t)sizeof(uint32_t);
        const int64_t per_hyp = (int64_t)P * a.max_n;
        keys = std::min<int64_t>(budget / per_hyp, H) * per_hyp;  // whole hypotheses of every problem
        if (keys > 0) {
            HIPCHK(c->medkeys.ensure(sizeof(uint32_t) * (size_t)keys));
            scr = c->medkeys.as<uint32_t>();
        }
    }
    HIPCHK(launch_pnp_median(a, P, 0, H, c->medians.as<double>(), scr, keys, s));
    return RSAC_OK;
}

// LMedS PnP (DESIGN.md "LMedS PnP"): hom_lmeds_core's round with the PnP solve, k_pnp_median* and
// sample size sk = 4 (P3P) or 5 (EPnP-5) as model_points; the all-f64 path without a frame, as the
// distorted calls run it.  The masks at the derived bounds come from the exact mask kernel, the
// final solve is pnp_finish's on those masks, the count == model_points problems keep run_direct.
int pnp_lmeds_core(rsac_ctx *c, const void *pts3d, const void *pts2d, const int64_t *offsets, int32_t P, int32_t n,
                   const double *K, int32_t max_iters, double conf, uint64_t seed, uint32_t flags, double *R_out,
                   double *t_out, int32_t *status_out, int32_t *ninl_out, double *medians_out, uint8_t *mask_out,
                   rsac_stats *stats, hipStream_t s) {
    int r = check_device(c);
    if (r) return r;
    if (P <= 0 || !K) return fail(RSAC_EINVAL, "bad problem count or K");
    r = check_flags("LMedS PnP", flags,
                    RSAC_F_SAMPLER_OPENCV | RSAC_F_ADAPTIVE | RSAC_F_REFINE | RSAC_F_EPNP | RSAC_F_MINIMAL_EPNP5 |
                        RSAC_F_RVEC_ROUNDTRIP | RSAC_F_DEVICE_IN | RSAC_F_DEVICE_SOA | RSAC_F_DEVICE_OUT);
    if (r) return r;
    if (!(conf > 0.0 && conf < 1.0)) return fail(RSAC_EINVAL, "confidence must lie in (0, 1), got %g", conf);
    if (max_iters < 1) return fail(RSAC_EINVAL, "max_iters must be >= 1, got %d", max_iters);
    if ((flags & RSAC_F_DEVICE_OUT) && !mask_out) return fail(RSAC_EINVAL, "RSAC_F_DEVICE_OUT needs mask_out");
    const bool opencv = (flags & RSAC_F_SAMPLER_OPENCV) != 0;
    const int sk = (flags & RSAC_F_MINIMAL_EPNP5) ? 5 : 4;
    const int64_t H = (flags & RSAC_F_ADAPTIVE) ? lmeds_num_iters(conf, sk, max_iters) : max_iters;
    flags |= RSAC_F_EXACT_ONLY;  // the all-f64 error: no frame, no f32 records, no fused set-up
    Staged st;
    r = stage_points(c, pts3d, pts2d, 3, offsets, P, n, flags, s, st);
    if (r) return r;
    r = stage_tables(c, st, K, 0.0, s);  // thr2 is written after the scan
    if (r) return r;
    // the tables on the device will differ from the staged ones: the next call uploads afresh
    c->last_tables.clear();
    c->last_tables_dev = nullptr;
    c->last_costs.clear();
    int n_direct = 0;  // count == model_points problems (direct_kinds)
    const std::vector<int8_t> dkind = direct_kinds(st, Model::PnP, sk, n_direct);
    const bool all_direct = n_direct == P;
    const int64_t stride = all_direct ? 1 : H;
    r = ensure_hyp_buffers(c, P, stride, opencv && !all_direct);
    if (r) return r;
    PnpArgs a;
    r = pnp_args(c, st, flags, seed, stride, 0, s, a, nullptr, false, true);
    if (r) return r;
    LoopOut lo;
    lo.timing = stats != nullptr || c->timing;
    reset_scans(lo, P, H);
    std::vector<double> best_median(P, 0.0);
    const auto direct = [&](int p) { return dkind[p] != 0; };
    const bool refit = (flags & (RSAC_F_REFINE | RSAC_F_EPNP)) != 0;
    if (!all_direct) {
        if (opencv) {  // one MWC state per problem and call, as each cv2 call restarts OpenCV's RNG
            const size_t recs = (size_t)P * (size_t)H;
            lo.rngs.assign(P, Mwc());
            draw_mwc_rows(c, st, Model::PnP, lo.rngs, direct, 0, H, H, sk);
            HIPCHK(hipMemcpyAsync(c->subsets.p, c->h_subsets.p, sizeof(int32_t) * sk * recs, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(c->substatus.p, c->h_substatus.p, recs, hipMemcpyHostToDevice, s));
            a.subsets = c->subsets.as<int32_t>();
            a.sub_status = c->substatus.as<int8_t>();
        }
        r = ensure_epnp5(c, a, P, H);
        if (r) return r;
        r = lmeds_round(
            c, st, H, sk, lo, best_median, s,
            [&]() -> int { HIPCHK(launch_pnp_solve(a, P, 0, (int32_t)H, s)); return RSAC_OK; },
            [&]() -> int { return pnp_median_launch(c, a, P, (int32_t)H, s); }, direct);
        if (r) return r;
        // the masks at the derived bounds and the winners' minimal models
        r = finish_masks(c, Model::PnP, st, &a, lo, stride, mask_out, flags, s);
        if (r) return r;
        std::vector<uint8_t> tmpmask;
        const uint8_t *hm = nullptr;
        r = host_mask(c, st, mask_out, flags, s, tmpmask, &hm);
        if (r) return r;
        bool cleared = false, any = false;  // (cleared or not, a synchronisation follows below)
        r = lmeds_count_masks(c, st, hm, sk, lo, mask_out, flags, s, direct, &cleared);
        if (r) return r;
        for (int p = 0; p < P; ++p) any = any || (!dkind[p] && lo.scan[p].best >= 0);
        // the final solve on the LMedS masks: pnp_finish writes the same masks again (the problems
        // that lost their model above now have none) and refits behind them
        if (refit && any) r = pnp_finish(c, st, a, lo, stride, K, mask_out, flags, s, true, false);
        else HIPCHK(hipStreamSynchronize(s));
        if (r) return r;
    }
    if (n_direct) {  // the minimal model of all the points, mask all ones, no final solve
        r = run_direct(c, Model::PnP, st, &a, dkind, lo, mask_out, flags, s);
        if (r) return r;
    }
    const double *bm = c->h_bestmodels.as<double>();
    int any = 0;
    for (int p = 0; p < P; ++p) {
        const bool ok = lo.scan[p].best >= 0;
        any |= ok;
        double m12[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (ok) memcpy(m12, bm + kModelStride * p, sizeof m12);
        if (R_out) memcpy(R_out + 9 * p, m12, 9 * sizeof(double));
        if (t_out) memcpy(t_out + 3 * p, m12 + 9, 3 * sizeof(double));
        if (status_out) status_out[p] = ok ? RSAC_OK : RSAC_NO_MODEL;
        if (ninl_out) ninl_out[p] = lo.scan[p].max_good;
        if (medians_out) medians_out[p] = !ok ? -1.0 : dkind[p] ? 0.0 : best_median[p];
    }
    if (stats) fill_stats(*stats, lo);
    if (c->timing) fill_stats(c->last_stats, lo);
    return any ? RSAC_OK : RSAC_NO_MODEL;
}

// fm_fit of the staged points over the device mask dmask (NULL = all), enqueued on s; the result
// record (F, ok, masked count: kFmFitRes doubles) is then copied to res (host) -- the caller
// synchronises before reading it
int fm_fit_enqueue(rsac_ctx *c, const Staged &st, const uint8_t *dmask, double *res, hipStream_t s) {
    const int32_t n = (int32_t)st.total;
    const size_t scr = fm_fit_scratch(n);
    HIPCHK(c->fmfit.ensure(sizeof(double) * (scr + kFmFitRes)));
    double *d = c->fmfit.as<double>();
    HIPCHK(launch_fm_fit(st.d[0], st.d[1], st.d[2], st.d[3], dmask, n, d, d + scr, s));
    HIPCHK(hipMemcpyAsync(res, d + scr, sizeof(double) * kFmFitRes, hipMemcpyDeviceToHost, s));
    return RSAC_OK;
}

// The batched fit (launch_fm_fit_batched) of the staged problems.  fm_fit_batch_plan lays c->fmfit
// out as the P result records, the range rows and the range prefix, and uploads the prefix (once per
// call: every round of a local optimisation reuses it); fm_fit_batch_enqueue fits over the device
// masks dmask (concatenated, NULL = all) and copies the records (kFmFitRes doubles per problem) to
// c->h_fmfit -- the caller synchronises before reading them.  Both after stage_tables (the offsets).
struct FmFitBatch {
    int32_t max_ranges = 1, total_ranges = 0;
    double *res = nullptr, *scr = nullptr;
    const int32_t *rbase = nullptr;
};

int fm_fit_batch_plan(rsac_ctx *c, const Staged &st, hipStream_t s, FmFitBatch &fb) {
    const int P = st.P;
    if (P < 1 || P > kFmBatchMaxP) return fail(RSAC_EINVAL, "bad problem count %d (1 .. %d)", P, kFmBatchMaxP);
    const size_t res_d = (size_t)kFmFitRes * P;
    HIPCHK(c->h_fmfit.ensure(sizeof(double) * res_d + sizeof(int32_t) * (P + 1)));
    int32_t *hr = (int32_t *)(c->h_fmfit.as<double>() + res_d);
    int64_t tot = 0;
    fb.max_ranges = 1;
    for (int p = 0; p < P; ++p) {
        const int64_t np = st.off[p + 1] - st.off[p];
        if (np > INT32_MAX) return fail(RSAC_EINVAL, "a problem exceeds 2^31 - 1 points");
        const int nr = fm_fit_ranges((int)np);
        hr[p] = (int32_t)tot;
        fb.max_ranges = std::max(fb.max_ranges, nr);
        tot += nr;
        if (tot > INT32_MAX) return fail(RSAC_EINVAL, "the batch exceeds 2^31 - 1 ranges");
    }
    hr[P] = (int32_t)tot;
    fb.total_ranges = (int32_t)tot;
    const size_t scr_d = (size_t)tot * (kFmFitS1 + kFmFitS2);
    HIPCHK(c->fmfit.ensure(sizeof(double) * (res_d + scr_d) + sizeof(int32_t) * (P + 1)));
    double *d = c->fmfit.as<double>();
    fb.res = d;
    fb.scr = d + res_d;
    fb.rbase = (const int32_t *)(d + res_d + scr_d);
    HIPCHK(hipMemcpyAsync((void *)fb.rbase, hr, sizeof(int32_t) * (P + 1), hipMemcpyHostToDevice, s));
    return RSAC_OK;
}

int fm_fit_batch_enqueue(rsac_ctx *c, const Staged &st, const FmFitBatch &fb, const uint8_t *dmask, hipStream_t s) {
    HIPCHK(launch_fm_fit_batched(st.d[0], st.d[1], st.d[2], st.d[3], dmask, c->d_off, fb.rbase, st.P, fb.max_ranges,
                                 fb.total_ranges, fb.scr, fb.res, s));
    HIPCHK(hipMemcpyAsync(c->h_fmfit.p, fb.res, sizeof(double) * kFmFitRes * (size_t)st.P, hipMemcpyDeviceToHost, s));
    return RSAC_OK;
}

// the mask of a fit call on the device: the caller's for device points, an upload into buf for host points
int fit_mask(DevBuf &buf, const uint8_t *mask, int64_t total, uint32_t flags, hipStream_t s, const uint8_t **dmask) {
    *dmask = mask;
    if (mask && !(flags & (RSAC_F_DEVICE_IN | RSAC_F_DEVICE_SOA))) {  // a host mask goes with host points
        HIPCHK(buf.ensure((size_t)std::max<int64_t>(total, 1)));
        HIPCHK(hipMemcpyAsync(buf.p, mask, (size_t)total, hipMemcpyHostToDevice, s));
        *dmask = buf.as<uint8_t>();
    }
    return RSAC_OK;
}

// the result records of a batched fit (`stride` doubles per problem: the model, then ok) -> out[9 p]
// (zeros without a model) and status_out[p]; whether any problem has a model
bool unpack_fit_records(const double *res, int stride, int32_t P, double *out, int32_t *status_out) {
    bool any = false;
    for (int p = 0; p < P; ++p) {
        const bool ok = res[(size_t)stride * p + 9] != 0.0;
        any = any || ok;
        if (ok)
            memcpy(out + 9 * (size_t)p, res + (size_t)stride * p, 9 * sizeof(double));
        else
            memset(out + 9 * (size_t)p, 0, 9 * sizeof(double));
        if (status_out) status_out[p] = ok ? RSAC_OK : RSAC_NO_MODEL;
    }
    return any;
}

// the argument checks of the local optimisations (`what`: the entry point, for the messages)
int local_opt_checks(rsac_ctx *c, const char *what, bool have_args, double thr, int32_t max_rounds, uint32_t flags,
                     const uint8_t *mask_out) {
    int r = check_device(c);
    if (r) return r;
    r = check_flags(what, flags, RSAC_F_DEVICE_IN | RSAC_F_DEVICE_SOA | RSAC_F_DEVICE_OUT);
    if (r) return r;
    if (!have_args) return fail(RSAC_EINVAL, "%s: bad arguments", what);
    if (max_rounds < 1) return fail(RSAC_EINVAL, "%s: max_rounds must be >= 1 (got %d)", what, max_rounds);
    r = check_msac_thr(what, thr);  // (float)(thr * thr) finite and positive
    if (r) return r;
    if (!(thr > 0.0)) return fail(RSAC_EINVAL, "%s needs a finite positive threshold", what);
    if ((flags & RSAC_F_DEVICE_OUT) && !mask_out) return fail(RSAC_EINVAL, "RSAC_F_DEVICE_OUT needs mask_out");
    return RSAC_OK;
}

// the repeated argument checks of the batched fit and local-optimisation entry points.  limit: the
// per-problem point limit here, before anything is staged (the essential family); the fundamental
// family meets the same limit in fm_fit_batch_plan, after staging.
int batch_checks(const char *what, const void *pts1, const void *pts2, const int64_t *offsets, int32_t P, bool limit) {
    if (P < 1 || P > kFmBatchMaxP || !offsets) return fail(RSAC_EINVAL, "%s: bad arguments", what);
    if (offsets[P] > 0 && (!pts1 || !pts2)) return fail(RSAC_EINVAL, "%s: bad arguments", what);
    for (int p = 0; limit && p < P; ++p)
        if (offsets[p + 1] - offsets[p] > INT32_MAX) return fail(RSAC_EINVAL, "a problem exceeds 2^31 - 1 points");
    return RSAC_OK;
}

// Local optimisation of the two-view models, every rsac_*_local_opt* entry point's
// loop: per problem, the model's own test's mask, the fit on it, and the fit accepted only when the
// masked count rises strictly -- at most max_rounds fits accepted, a fit without a model ends the
// problem's loop.  The fit counts the mask it is given, so one result record carries mask k's count
// and round k + 1's model; "current" and "next" are whole records.  The problems still rising run
// side by side: one mask launch, one fit and one synchronisation per round.
//
// A family is its mask kernel, its mask buffer and its record: `stride` doubles, the model the mask
// kernel takes at `model` (the model returned is at 0; H and F are both, the essential record
// carries F beside E), ok and the masked count at kFitOk and kFitCount.
//   start(p, rec) -> whether M_in's row p is a model; it fills record p (zeros on entry).
//   fit(dmask, recs, on, res): the fit of the staged problems whose `on` byte is set, over the
//     device masks dmask, started from the records recs, enqueued and the stream synchronised;
//     *res: the P result records on the host.
// A problem's model is record p of c->models (hypothesis stride 1); the mask kernel takes it through
// c->best, where -1 names a problem that takes no part in the round: its mask is zero.  One problem
// needs no c->best: best0 says the same.  The uploads are from pageable memory, complete on return.
// One problem keeps two masks and swaps them, so the mask of the model returned is the one already
// computed; more problems stop at different rounds, and their final masks take one more launch.
// After local_opt_checks, stage_points and stage_tables.
constexpr int kFitOk = 9, kFitCount = 10;
struct FitFamily {
    decltype(launch_hom_mask) *launch_mask;
    DevBuf &masks;
    int stride, model;
};
static_assert(kHomFitRes > kFitCount && kFmFitRes > kFitCount && kEmFitRes >= 11 + 9, "a fit's result record");

template <class Start, class Fit>
int local_opt_loop(rsac_ctx *c, const Staged &st, const FitFamily &fam, int32_t max_rounds, uint32_t flags,
                   double *M_out, int32_t *counts_out, int32_t *steps_out, uint8_t *mask_out, hipStream_t s,
                   Start start, Fit fit) {
    const int P = st.P, R = fam.stride;
    const bool one = P == 1;
    int r = ensure_hyp_buffers(c, P, 1, false);
    if (r) return r;
    const HomArgs a = hom_args(c, st, 0, 0, 1, false);
    const int32_t max_n = st.max_n();
    const size_t N = (size_t)std::max<int64_t>(st.total, 1);
    HIPCHK(fam.masks.ensure(one ? 2 * N : N));
    uint8_t *cur = fam.masks.as<uint8_t>(), *other = one ? cur + N : cur;
    std::vector<double> models((size_t)kModelStride * P, 0.0);
    std::vector<int64_t> idx(P);
    auto masks_of = [&](const std::vector<double> &recs, const std::vector<uint8_t> &on, uint8_t *m) -> int {
        for (int p = 0; p < P; ++p) {
            memcpy(&models[(size_t)kModelStride * p], &recs[(size_t)R * p + fam.model], 9 * sizeof(double));
            models[(size_t)kModelStride * p + kValidSlot] = 1.0;
            idx[p] = on[p] ? p : -1;
        }
        HIPCHK(hipMemcpyAsync(c->models.p, models.data(), sizeof(double) * models.size(), hipMemcpyHostToDevice, s));
        if (!one) HIPCHK(hipMemcpyAsync(c->best.p, idx.data(), sizeof(int64_t) * P, hipMemcpyHostToDevice, s));
        HIPCHK(fam.launch_mask(a, P, max_n, one ? nullptr : c->best.as<int64_t>(), m, s, one ? idx[0] : -1));
        return RSAC_OK;
    };
    const double *res = nullptr;
    auto round = [&](const std::vector<double> &recs, const std::vector<uint8_t> &on, uint8_t *m) -> int {
        if (int e = masks_of(recs, on, m)) return e;
        return fit(m, recs.data(), on.data(), &res);
    };
    std::vector<double> rec((size_t)R * P, 0.0), next(rec);
    std::vector<uint8_t> model(P), live(P);
    std::vector<int32_t> count(P, 0), steps(P, 0);
    for (int p = 0; p < P; ++p) model[p] = start(p, &rec[(size_t)R * p]);
    r = round(rec, model, cur);
    if (r) return r;
    bool any_live = false;
    for (int p = 0; p < P; ++p) {
        const double *rp = res + (size_t)R * p;
        count[p] = model[p] ? (int32_t)rp[kFitCount] : 0;
        live[p] = model[p] && rp[kFitOk] != 0.0;
        memcpy(&next[(size_t)R * p], rp, R * sizeof(double));
        any_live = any_live || live[p];
    }
    while (any_live) {
        r = round(next, live, other);
        if (r) return r;
        any_live = false;
        for (int p = 0; p < P; ++p) {
            if (!live[p]) continue;
            const double *rp = res + (size_t)R * p;
            if (!((int32_t)rp[kFitCount] > count[p])) {  // accepted only when the count rises strictly
                live[p] = 0;
                continue;
            }
            memcpy(&rec[(size_t)R * p], &next[(size_t)R * p], R * sizeof(double));
            memcpy(&next[(size_t)R * p], rp, R * sizeof(double));
            count[p] = (int32_t)rp[kFitCount];
            ++steps[p];
            live[p] = steps[p] < max_rounds && rp[kFitOk] != 0.0;
            any_live = any_live || live[p];
            std::swap(cur, other);  // (one problem: `other` is `cur` otherwise)
        }
    }
    for (int p = 0; p < P; ++p) memcpy(M_out + 9 * (size_t)p, &rec[(size_t)R * p], 9 * sizeof(double));
    if (counts_out) memcpy(counts_out, count.data(), sizeof(int32_t) * P);
    if (steps_out) memcpy(steps_out, steps.data(), sizeof(int32_t) * P);
    if (mask_out) {  // the masks of the models returned
        const bool dev = (flags & RSAC_F_DEVICE_OUT) != 0;
        if (!one) {
            r = masks_of(rec, model, dev ? mask_out : cur);
            if (r) return r;
        }
        if ((one || !dev) && st.total > 0)
            HIPCHK(hipMemcpyAsync(mask_out, cur, (size_t)st.total, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return RSAC_OK;
}

// the staging of a fit or a local optimisation: the points of the P problems (offsets NULL: one problem
// of n points), then the offsets and the bound on the device
int stage_problems(rsac_ctx *c, const void *p1, const void *p2, const int64_t *offsets, int32_t P, int32_t n, double thr,
                   uint32_t flags, hipStream_t s, Staged &st) {
    if (int r = stage_points(c, p1, p2, 2, offsets, P, n, flags, s, st)) return r;
    return stage_tables(c, st, nullptr, thr, s);
}

// the start of a homography's or a fundamental matrix's record: row p of M_in; whether any element is
// non-zero (the batched call's "a model"; the single calls take every row for one, all zeros too)
bool model_row(const double *M_in, int p, double *rec) {
    memcpy(rec, M_in + 9 * (size_t)p, 9 * sizeof(double));
    bool any = false;
    for (int k = 0; k < 9; ++k) any = any || rec[k] != 0.0;
    return any;
}

// the flags rsac_fundamental_ransac and its batched form turn away, by name
int fm_ransac_flags(const char *what, uint32_t flags) {
    if ((flags & RSAC_F_MSAC) && (flags & (RSAC_F_LO | RSAC_F_ASYNC)))
        return fail(RSAC_EINVAL, "RSAC_F_MSAC cannot be combined with RSAC_F_LO or RSAC_F_ASYNC");
    if (flags & RSAC_F_SAMPLER_OPENCV)
        return fail(RSAC_EINVAL, "%s does not take RSAC_F_SAMPLER_OPENCV: Philox sampler only", what);
    if (flags & RSAC_F_LO)
        return fail(RSAC_EINVAL, "%s does not take RSAC_F_LO: rsac_fundamental_local_opt optimises the winner "
                                 "after the loop", what);
    if (flags & RSAC_F_EPNP) return fail(RSAC_EINVAL, "%s does not take RSAC_F_EPNP", what);
    return RSAC_OK;
}

// rsac_fundamental_ransac_batched: rsac_fundamental_ransac's sequence with P problems per launch --
// the pre-filter bounds, run_loop (every problem follows its own scan and bound), the masks, and
// under RSAC_F_REFINE one batched fit on the masks where finish_masks left them, behind the same
// synchronisation as the masks' copy-out.
int fm_batched_core(rsac_ctx *c, const void *pts1, const void *pts2, const int64_t *offsets, int32_t P,
                    int32_t max_iters, double thr, double conf, uint64_t seed, uint32_t flags, double *F_out,
                    int32_t *status_out, int32_t *ninl_out, uint8_t *mask_out, hipStream_t s) {
    const char *what = (flags & kFlagEm5) ? "rsac_essential_ransac_batched" : "rsac_fundamental_ransac_batched";
    if (P < 1 || P > kFmBatchMaxP || !offsets) return fail(RSAC_EINVAL, "%s: bad arguments", what);
    int r = fm_ransac_flags(what, flags);
    if (r) return r;
    if (flags & RSAC_F_ASYNC) return fail(RSAC_EINVAL, "%s does not take RSAC_F_ASYNC", what);
    const int sk = fm_sample_size(flags);
    for (int p = 0; p < P; ++p)
        if (offsets[p + 1] - offsets[p] < sk)
            return fail(RSAC_ETOOFEW, "the %d-point %s matrix needs >= %d correspondences (problem %d has %lld)", sk,
                        sk == 5 ? "essential" : "fundamental", sk, p, (long long)(offsets[p + 1] - offsets[p]));
    if ((flags & RSAC_F_DEVICE_OUT) && !mask_out) return fail(RSAC_EINVAL, "RSAC_F_DEVICE_OUT needs mask_out");
    const bool msac = (flags & RSAC_F_MSAC) != 0;
    const bool refit = (flags & RSAC_F_REFINE) != 0;  // the loop itself never sees the flag
    flags &= ~(uint32_t)RSAC_F_REFINE;
    if (msac) {
        r = check_msac_thr("RSAC_F_MSAC", thr);
        if (r) return r;
        flags |= RSAC_F_EXACT_ONLY;  // MSAC implies the exact path (k_fm_cost): no pre-filter, no f32 records
    }
    Staged st;
    r = stage_points(c, pts1, pts2, 2, offsets, P, 0, flags, s, st);
    if (r) return r;
    r = stage_tables(c, st, nullptr, thr, s);
    if (r) return r;
    const int64_t stride = (int64_t)std::max(max_iters, 1) * records_per_sample(Model::Fm, flags);  // run_loop's H
    r = ensure_hyp_buffers(c, P, stride, false);
    if (r) return r;
    HomArgs a = hom_args(c, st, seed, 0, stride, false);
    r = fm_prefilter(c, a, P, flags, s);
    if (r) return r;
    LoopOut lo;
    r = run_loop(c, Model::Fm, st, a, max_iters, conf, flags, s, lo);
    if (r) return r;
    r = finish_masks(c, Model::Fm, st, &a, lo, stride, mask_out, flags, s, refit);
    if (r) return r;
    if (refit) {  // finish_masks left the stream running: the winners' records, the fit, one synchronisation
        HIPCHK(hipMemcpyAsync(c->h_bestmodels.p, c->bestmodels.p, sizeof(double) * kModelStride * P,
                              hipMemcpyDeviceToHost, s));
        FmFitBatch fb;
        r = fm_fit_batch_plan(c, st, s, fb);
        if (r) return r;
        r = fm_fit_batch_enqueue(c, st, fb, device_mask_ptr(c, mask_out, flags), s);
        if (r) return r;
        HIPCHK(hipStreamSynchronize(s));
        finish_masks_host(c, st, mask_out, flags);
    }
    const double *bm = c->h_bestmodels.as<double>(), *fit = c->h_fmfit.as<double>();
    int any = 0;
    for (int p = 0; p < P; ++p) {
        const bool ok = lo.scan[p].best >= 0;
        any |= ok;
        if (F_out) {
            double *F = F_out + 9 * (size_t)p;
            if (!ok)
                memset(F, 0, 9 * sizeof(double));
            else if (refit && fit[(size_t)kFmFitRes * p + 9] != 0.0)  // a fit without a model: the minimal F stays
                memcpy(F, fit + (size_t)kFmFitRes * p, 9 * sizeof(double));
            else
                memcpy(F, bm + (size_t)kModelStride * p, 9 * sizeof(double));
        }
        if (status_out) status_out[p] = ok ? RSAC_OK : RSAC_NO_MODEL;
        if (ninl_out) ninl_out[p] = lo.scan[p].max_good;
    }
    if (msac) {  // rsac_last_costs
        c->last_costs.assign(P, -1);
        for (int p = 0; p < P; ++p)
            if (lo.scan[p].best >= 0) c->last_costs[p] = lo.best_cost[p];
    }
    if (c->timing) fill_stats(c->last_stats, lo);  // rsac_set_timing: the batched call's figures
    return any ? RSAC_OK : RSAC_NO_MODEL;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

const char *rsac_last_error(void) { return g_err.c_str(); }
int rsac_abi_version(void) { return RSAC_ABI_VERSION; }

int rsac_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rsac_create(int device, rsac_ctx **out) {
    if (!out) return fail(RSAC_EINVAL, "null out");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(RSAC_ENODEV, "no HIP device visible");
    if (device < 0 || device >= n) return fail(RSAC_EINVAL, "device %d out of range (%d devices)", device, n);
    HIPCHK(hipSetDevice(device));
    rsac_ctx *c = new rsac_ctx();
    c->device = device;
    // blocking stream: ordered with the legacy null stream, which is torch's default stream
    // (handle 0, indistinguishable from stream = NULL at the C-ABI), so device inputs written by
    // torch before a call, and device outputs read by torch after it, need no extra sync
    if (hipStreamCreateWithFlags(&c->stream, hipStreamDefault) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipEventCreate(&c->ev2) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_pts, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_small, hipEventDisableTiming) != hipSuccess) {
        rsac_destroy(c);
        return fail(RSAC_EHIP, "stream/event creation failed");
    }
    *out = c;
    return RSAC_OK;
}

void rsac_destroy(rsac_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    DevBuf *dev[] = {&c->pts,  &c->tables,     &c->models,  &c->status,  &c->counts,    &c->subsets,
                     &c->substatus, &c->best, &c->bestmodels, &c->mask, &c->bounds_ws,
                     &c->frame, &c->fconst,   &c->fmodels, &c->queue, &c->loc, &c->lo, &c->win, &c->geo,
                     &c->epnp, &c->epnp5, &c->direct, &c->lmscr, &c->setup_scr, &c->scanrec, &c->mxpts, &c->reproj,
                     &c->distbuf, &c->costs, &c->medians, &c->medkeys, &c->bound, &c->fmfit, &c->fmfit_mask, &c->em_kinv, &c->emfit};
    for (DevBuf *b : dev) b->release();
    PinBuf *pin[] = {&c->h_lmfail, &c->h_pts, &c->h_small, &c->h_counts, &c->h_status, &c->h_subsets,
                     &c->h_substatus, &c->h_best, &c->h_bestmodels, &c->h_mask, &c->h_scanrec, &c->h_lo,
                     &c->h_epnp, &c->h_rowinfo, &c->h_direct, &c->h_costs, &c->h_medians, &c->h_fmfit, &c->h_emfit};
    for (PinBuf *b : pin) b->release();
    c->lo_state_base = nullptr;
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->ev2) (void)hipEventDestroy(c->ev2);
    if (c->ev_pts) (void)hipEventDestroy(c->ev_pts);
    if (c->ev_small) (void)hipEventDestroy(c->ev_small);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int rsac_debug_set(rsac_ctx *c, int32_t key, int64_t value) {
    if (!c) return fail(RSAC_EINVAL, "null context");
    switch (key) {
    case RSAC_DBG_REFIT_MAX_BLOCKS:
        if (value < 0) return fail(RSAC_EINVAL, "bad block cap");
        c->dbg_refit_max_blocks = (int)std::min<int64_t>(value, kLmMaxBlocks);
        c->lm.max_blocks = pnp_refine_coresident(c->device);
        if (c->dbg_refit_max_blocks > 0) c->lm.max_blocks = std::min(c->lm.max_blocks, c->dbg_refit_max_blocks);
        return RSAC_OK;
    case RSAC_DBG_REFIT_DROP_BLOCK:
        c->lm.drop_block = value != 0;
        return RSAC_OK;
    case RSAC_DBG_MF_CELL_PTS:
        if (value < 0 || value > (1 << 30)) return fail(RSAC_EINVAL, "bad cell size");
        c->dbg_cell_pts = (int32_t)value;
        return RSAC_OK;
    case RSAC_DBG_SPEC_OVERFLOW:
        c->dbg_spec_overflow = value != 0;
        return RSAC_OK;
    case RSAC_DBG_BOUND:
        if (value < 0 || value > 2) return fail(RSAC_EINVAL, "bad bounded-scoring mode");
        c->dbg_bound = (int)value;
        return RSAC_OK;
    case RSAC_DBG_BOUND_SLAB:
        if (value < 0 || value > 2) return fail(RSAC_EINVAL, "bad slab mode");
        c->dbg_bound_slab = (int)value;
        return RSAC_OK;
    case RSAC_DBG_BOUND_COUNT:
        if (value < 0 || value > INT32_MAX) return fail(RSAC_EINVAL, "bad hypothesis index");
        c->dbg_bound_count = (int32_t)value;
        return RSAC_OK;
    case RSAC_DBG_BOUND_P2_MIN:
        if (value < 0 || value > (1 << 20)) return fail(RSAC_EINVAL, "bad share length");
        c->dbg_bound_p2_min = (int32_t)value;
        return RSAC_OK;
    case RSAC_DBG_LMEDS_KEYS:
        c->dbg_lmeds_keys = value;
        return RSAC_OK;
    case RSAC_DBG_HOM_FIT:
        if (value < 0 || value > 2) return fail(RSAC_EINVAL, "bad homography-refit mode");
        c->dbg_hom_fit = (int)value;
        return RSAC_OK;
    case RSAC_DBG_F64_SELFTEST:
    case RSAC_DBG_SLAB_SELFTEST: {
        if (value < 0 || value > (int64_t)1 << 30) return fail(RSAC_EINVAL, "bad self-test size");
        int r = check_device(c);
        if (r) return r;
        int *d = nullptr;
        HIPCHK(hipMalloc(&d, sizeof(int)));
        hipError_t e = hipMemsetAsync(d, 0, sizeof(int), c->stream);
        if (e == hipSuccess)
            e = key == RSAC_DBG_F64_SELFTEST ? launch_f64_selftest(value, d, c->stream)
                                             : launch_slab_selftest(value, d, c->stream);
        int h = -1;
        if (e == hipSuccess) e = hipMemcpyAsync(&h, d, sizeof(int), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        (void)hipFree(d);
        HIPCHK(e);
        (key == RSAC_DBG_F64_SELFTEST ? c->dbg_f64_selftest : c->dbg_slab_selftest) = h;
        return RSAC_OK;
    }
    default:
        return fail(RSAC_EINVAL, "unknown debug key %d", key);
    }
}

int rsac_debug_get(rsac_ctx *c, int32_t key, int64_t *value) {
    if (!c || !value) return fail(RSAC_EINVAL, "null argument");
    switch (key) {
    case RSAC_DBG_SPEC_FINISHES:
        *value = c->spec_finishes;
        return RSAC_OK;
    case RSAC_DBG_SPEC_REDOS:
        *value = c->spec_redos;
        return RSAC_OK;
    case RSAC_DBG_F64_SELFTEST:
        *value = c->dbg_f64_selftest;
        return RSAC_OK;
    case RSAC_DBG_SLAB_SELFTEST:
        *value = c->dbg_slab_selftest;
        return RSAC_OK;
    case RSAC_DBG_BOUND_SLAB:
        *value = c->dbg_bound_slab;
        return RSAC_OK;
    case RSAC_DBG_SETUP_REUSED:
        *value = c->setup_reused ? 1 : 0;
        return RSAC_OK;
    case RSAC_DBG_BOUND_HINTED:
        *value = c->bound_hinted ? 1 : 0;
        return RSAC_OK;
    case RSAC_DBG_BOUND_N1:
    case RSAC_DBG_BOUND_SURVIVORS: {
        if (!c->bound_last) {  // an unbounded call: every point in one pass
            *value = key == RSAC_DBG_BOUND_N1 ? c->bound_last_n : 0;
            return RSAC_OK;
        }
        int r = check_device(c);
        if (r) return r;
        int32_t plan[kBoundPlanWords];
        HIPCHK(hipMemcpy(plan, c->bound.as<int32_t>() + kBoundPlanStride * c->bound_rec, sizeof plan,
                         hipMemcpyDeviceToHost));
        *value = key == RSAC_DBG_BOUND_N1 ? plan[0] : plan[2];
        return RSAC_OK;
    }
    case RSAC_DBG_BOUND_SLAB_RAN: {
        *value = 0;
        if (!c->bound_last) return RSAC_OK;
        int r = check_device(c);
        if (r) return r;
        int32_t plan[kBoundPlanWords];
        HIPCHK(hipMemcpy(plan, c->bound.as<int32_t>() + kBoundPlanStride * c->bound_rec, sizeof plan,
                         hipMemcpyDeviceToHost));
        *value = pnp_bound_slab_ran(plan, c->bound_last_exact) ? 1 : 0;
        return RSAC_OK;
    }
    case RSAC_DBG_BOUND_COUNT: {
        if (!c->bound_last || c->dbg_bound_count >= c->bound_last_h)
            return fail(RSAC_EINVAL, "RSAC_DBG_BOUND_COUNT: no bounded call, or an index past its hypotheses");
        int r = check_device(c);
        if (r) return r;
        int32_t cnt = 0;
        HIPCHK(hipMemcpy(&cnt, c->counts.as<int32_t>() + c->dbg_bound_count, sizeof cnt, hipMemcpyDeviceToHost));
        *value = cnt;
        return RSAC_OK;
    }
    default:
        return fail(RSAC_EINVAL, "unknown debug key %d", key);
    }
}

int rsac_bound_layout(int32_t what, const int32_t *in, int32_t *out) {
    if (!in || !out) return fail(RSAC_EINVAL, "null argument");
    switch (what) {
    case 0: {  // in: group, row, half, accumulator, hypothesis of the tile
        if (in[0] < 0 || in[0] > 1 || in[1] < 0 || in[1] > 31 || in[2] < 0 || in[2] > 1 || in[3] < 0 || in[3] > 15 ||
            in[4] < 0 || in[4] > 31)
            return fail(RSAC_EINVAL, "rsac_bound_layout: index out of range");
        out[0] = slab_pack_row_hyp(in[0], in[1]);
        out[1] = slab_pack_row_comp(in[1]);
        out[2] = slab_pack_acc_hyp(in[0], in[2], in[3]);
        out[3] = slab_pack_acc_comp(in[3]);
        out[4] = slab_pack_slot(in[4]);
        out[5] = slab_pack_half(in[4]);
        return RSAC_OK;
    }
    case 1:
    case 2: {  // in: tiles, points, grid, shares per block, shortest share (what = 2: + share, position)
        int32_t k[4];
        pnp_bound_layout_consts(k);
        if (in[0] < 0 || in[1] < 0 || in[2] < 1) return fail(RSAC_EINVAL, "rsac_bound_layout: bad line");
        const BoundShares s = bound_shares(in[0], in[1], in[2], in[3] > 0 ? in[3] : k[0], in[4] > 0 ? in[4] : k[1]);
        if (what == 1) {
            out[0] = s.passes;
            out[1] = s.len;
            out[2] = s.n;
            return RSAC_OK;
        }
        const int64_t line = (int64_t)in[0] * s.passes;
        const int64_t lo = (int64_t)in[5] * s.len, hi = std::min<int64_t>(line, lo + s.len);
        if (in[5] < 0 || in[5] >= s.n || in[6] < lo || in[6] >= hi)
            return fail(RSAC_EINVAL, "rsac_bound_layout: position outside the share");
        int tile = 0, first = 0;
        out[2] = bound_share_seg(s, in[0], in[5], in[6], k[2], &tile, &first);
        out[0] = tile;
        out[1] = first;
        return RSAC_OK;
    }
    case 3:
        pnp_bound_layout_consts(out);
        return RSAC_OK;
    default:
        return fail(RSAC_EINVAL, "rsac_bound_layout: unknown map %d", what);
    }
}

int rsac_refit_blocks(rsac_ctx *c, int32_t n, int32_t *ranges, int32_t *blocks) {
    if (!c || n < 0) return fail(RSAC_EINVAL, "bad arguments");
    int r = check_device(c);
    if (r) return r;
    LmScratch *lm = lm_scratch(c, c->stream);
    if (!lm) return fail(RSAC_ENOMEM, "refit scratch");
    const int nb = lm_blocks(n);
    if (ranges) *ranges = nb;
    if (blocks) *blocks = nb > 1 ? std::min(nb, lm->max_blocks) : 1;
    return RSAC_OK;
}

int rsac_set_timing(rsac_ctx *c, int32_t on) {
    if (!c) return fail(RSAC_EINVAL, "null context");
    c->timing = on != 0;
    return RSAC_OK;
}

int rsac_last_stats(rsac_ctx *c, rsac_stats *out) {
    if (!c || !out) return fail(RSAC_EINVAL, "bad arguments");
    *out = c->last_stats;
    return RSAC_OK;
}

int rsac_set_round_size(rsac_ctx *c, int64_t hyps) {
    if (!c || hyps <= 0) return fail(RSAC_EINVAL, "bad round size");
    c->round_size = hyps;
    return RSAC_OK;
}

int rsac_pnp_ransac(rsac_ctx *c, const void *pts3d, const void *pts2d, int32_t n, const double K[9], int32_t n_iters,
                    double thr, double conf, uint64_t seed, uint32_t flags, double R_out[9], double t_out[3],
                    uint8_t *mask_out, rsac_stats *stats, void *stream) {
    if (n < 4) return fail(RSAC_ETOOFEW, "solvePnPRansac needs >= 4 correspondences (got %d)", n);
    int32_t status = 0, ninl = 0;
    return with_one_refit_block(c, [&] {
        return pnp_core(c, pts3d, pts2d, nullptr, 1, n, K, n_iters, thr, conf, seed, flags, R_out, t_out, &status,
                        &ninl, mask_out, stats, pick_stream(c, stream));
    });
}

int rsac_pnp_ransac_dist(rsac_ctx *c, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                         const double *dist, int32_t n_dist, int32_t n_iters, double thr, double conf, uint64_t seed,
                         uint32_t flags, double R_out[9], double t_out[3], uint8_t *mask_out, rsac_stats *stats,
                         void *stream) {
    DistK kd;
    bool active = false;
    if (int r = parse_dist_for("rsac_pnp_ransac_dist", dist, n_dist, flags, kd, active)) return r;
    if (!active)  // no distortion: the pinhole call, bit for bit
        return rsac_pnp_ransac(c, pts3d, pts2d, n, K, n_iters, thr, conf, seed, flags, R_out, t_out, mask_out, stats,
                               stream);
    if (flags & RSAC_F_LO)
        return fail(RSAC_EINVAL, "rsac_pnp_ransac_dist: RSAC_F_LO is not supported with lens distortion");
    if (n < 4) return fail(RSAC_ETOOFEW, "solvePnPRansac needs >= 4 correspondences (got %d)", n);
    int32_t status = 0, ninl = 0;
    return with_one_refit_block(c, [&] {
        return pnp_core(c, pts3d, pts2d, nullptr, 1, n, K, n_iters, thr, conf, seed, flags, R_out, t_out, &status,
                        &ninl, mask_out, stats, pick_stream(c, stream), nullptr, nullptr, &kd, n_dist);
    });
}

int rsac_pnp_ransac_first_round(rsac_ctx *c, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                                int32_t n_iters, double thr, double conf, uint64_t seed, uint32_t flags,
                                double R_out[9], double t_out[3], uint8_t *mask_out, rsac_scan_state *st_out,
                                rsac_stats *stats, void *stream) {
    if (n < 4) return fail(RSAC_ETOOFEW, "solvePnPRansac needs >= 4 correspondences (got %d)", n);
    if (!st_out) return fail(RSAC_EINVAL, "st_out required");
    int32_t status = 0, ninl = 0;
    return with_one_refit_block(c, [&] {
        return pnp_core(c, pts3d, pts2d, nullptr, 1, n, K, n_iters, thr, conf, seed, flags, R_out, t_out, &status,
                        &ninl, mask_out, stats, pick_stream(c, stream), st_out);
    });
}

int rsac_pnp_ransac_batched_rows(rsac_ctx *c, const void *pts3d, const void *pts2d, const int64_t *offsets, int32_t P,
                                 const double *K, int32_t n_iters, double thr, double conf, uint64_t seed,
                                 uint32_t flags, double *rows_out, uint8_t *mask_out, void *stream) {
    if (!offsets || !rows_out) return fail(RSAC_EINVAL, "offsets and rows_out required");
    return with_one_refit_block(c, [&] {
        return pnp_core(c, pts3d, pts2d, offsets, P, 0, K, n_iters, thr, conf, seed, flags, nullptr, nullptr,
                        nullptr, nullptr, mask_out, nullptr, pick_stream(c, stream), nullptr, rows_out);
    });
}

int rsac_pnp_ransac_batched(rsac_ctx *c, const void *pts3d, const void *pts2d, const int64_t *offsets, int32_t P,
                            const double *K, int32_t n_iters, double thr, double conf, uint64_t seed, uint32_t flags,
                            double *R_out, double *t_out, int32_t *status_out, int32_t *ninl_out, uint8_t *mask_out,
                            void *stream) {
    if (!offsets) return fail(RSAC_EINVAL, "offsets required");
    return with_one_refit_block(c, [&] {
        return pnp_core(c, pts3d, pts2d, offsets, P, 0, K, n_iters, thr, conf, seed, flags, R_out, t_out, status_out,
                        ninl_out, mask_out, nullptr, pick_stream(c, stream));
    });
}

int rsac_homography_ransac(rsac_ctx *c, const void *src, const void *dst, int32_t n, int32_t max_iters, double thr,
                           double conf, uint64_t seed, uint32_t flags, double H_out[9], uint8_t *mask_out,
                           rsac_stats *stats, void *stream) {
    if (n < 4) return fail(RSAC_ETOOFEW, "findHomography needs >= 4 correspondences (got %d)", n);
    int32_t status = 0, ninl = 0;
    return hom_core(c, src, dst, nullptr, 1, n, max_iters, thr, conf, seed, flags, H_out, &status, &ninl, mask_out,
                    stats, pick_stream(c, stream));
}

int rsac_homography_ransac_batched(rsac_ctx *c, const void *src, const void *dst, const int64_t *offsets, int32_t P,
                                   int32_t max_iters, double thr, double conf, uint64_t seed, uint32_t flags,
                                   double *H_out, int32_t *status_out, int32_t *ninl_out, uint8_t *mask_out,
                                   void *stream) {
    if (!offsets) return fail(RSAC_EINVAL, "offsets required");
    return hom_core(c, src, dst, offsets, P, 0, max_iters, thr, conf, seed, flags, H_out, status_out, ninl_out,
                    mask_out, nullptr, pick_stream(c, stream));
}

int rsac_location_search(rsac_ctx *c, const double *pos3d, const double *pixels, int32_t n, const double *locations,
                         int32_t L, double thr, int32_t max_iters, double conf, uint32_t flags, double *H_out,
                         double *err_out, int32_t *status_out, int32_t *ninl_out, uint8_t *mask_out,
                         int32_t *n_good_out, void *stream) {
    int r = check_device(c);
    if (r) return r;
    if ((r = reject_fm7("rsac_location_search", flags))) return r;
    if (!pos3d || !pixels || !locations || !err_out || n <= 0 || L <= 0)
        return fail(RSAC_EINVAL, "rsac_location_search: bad arguments");
    if (flags & (RSAC_F_DEVICE_IN | RSAC_F_DEVICE_SOA | RSAC_F_DEVICE_OUT))
        return fail(RSAC_EINVAL, "rsac_location_search takes host arrays");
    hipStream_t s = pick_stream(c, stream);
    // features noted on the image: pixel != (0, 0) (main_v1.py:304)
    std::vector<double> in;
    in.reserve((size_t)5 * n + 3 * L);
    int32_t ng = 0;
    for (int32_t i = 0; i < n; ++i)
        if (pixels[2 * i] != 0.0 || pixels[2 * i + 1] != 0.0) {
            in.insert(in.end(), pos3d + 3 * i, pos3d + 3 * i + 3);
            ++ng;
        }
    for (int32_t i = 0; i < n; ++i)
        if (pixels[2 * i] != 0.0 || pixels[2 * i + 1] != 0.0) in.insert(in.end(), pixels + 2 * i, pixels + 2 * i + 2);
    in.insert(in.end(), locations, locations + 3 * (size_t)L);
    if (n_good_out) *n_good_out = ng;
    if (ng < 4) return fail(RSAC_ETOOFEW, "findHomography needs >= 4 noted features (got %d)", ng);
    const size_t pairs = (size_t)L * ng;
    // device layout (f64): p3 [3 ng] px [2 ng] locs [3 L] src [2 L ng] dst [2 L ng] H [9 L] err [2 L], ok [L] i32
    const size_t nd = in.size() + 4 * pairs + 11 * (size_t)L;
    HIPCHK(c->loc.ensure(nd * sizeof(double) + sizeof(int32_t) * L));
    double *d_p3 = c->loc.as<double>(), *d_px = d_p3 + 3 * ng, *d_locs = d_px + 2 * ng, *d_src = d_locs + 3 * L;
    double *d_dst = d_src + 2 * pairs, *d_H = d_dst + 2 * pairs, *d_err = d_H + 9 * (size_t)L;
    int32_t *d_ok = (int32_t *)(d_err + 2 * (size_t)L);
    HIPCHK(hipMemcpyAsync(d_p3, in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(launch_loc_pos2(d_p3, d_px, ng, d_locs, L, d_src, d_dst, s));
    std::vector<int64_t> off((size_t)L + 1);
    for (int32_t l = 0; l <= L; ++l) off[l] = (int64_t)l * ng;
    std::vector<double> H((size_t)9 * L);
    std::vector<int32_t> st(L), ninl(L);
    std::vector<uint8_t> m(pairs);
    r = hom_core(c, d_src, d_dst, off.data(), L, 0, max_iters, thr, conf, 0, flags | RSAC_F_DEVICE_IN, H.data(),
                 st.data(), ninl.data(), m.data(), nullptr, s, true);
    if (r < 0) return r;
    // hom_core left the RANSAC-phase masks of every location in c->mask
    std::vector<int32_t> ok(L);
    for (int32_t l = 0; l < L; ++l) ok[l] = st[l] == RSAC_OK;
    HIPCHK(hipMemcpyAsync(d_H, H.data(), H.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_ok, ok.data(), sizeof(int32_t) * L, hipMemcpyHostToDevice, s));
    HIPCHK(launch_loc_score(d_src, d_dst, c->mask.as<uint8_t>(), d_H, d_ok, L, ng, thr <= 0 ? 3.0 : thr, d_err, s));
    HIPCHK(hipMemcpyAsync(err_out, d_err, sizeof(double) * 2 * L, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (H_out) memcpy(H_out, H.data(), H.size() * sizeof(double));
    if (status_out) memcpy(status_out, st.data(), sizeof(int32_t) * L);
    if (ninl_out) memcpy(ninl_out, ninl.data(), sizeof(int32_t) * L);
    if (mask_out) memcpy(mask_out, m.data(), pairs);
    return r;
}

int rsac_utm_convert(rsac_ctx *c, int inverse, const double *in, int64_t n, int32_t zone, int32_t south,
                     uint32_t flags, double *out, void *stream) {
    int r = check_device(c);
    if (r) return r;
    if ((r = reject_fm7("rsac_utm_convert", flags))) return r;
    if (!in || !out || n < 0 || zone < 1 || zone > 60) return fail(RSAC_EINVAL, "bad arguments");
    if (n == 0) return RSAC_OK;
    hipStream_t s = pick_stream(c, stream);
    const bool dev = (flags & RSAC_F_DEVICE_IN) != 0;
    const double *din = in;
    double *dout = out;
    if (!dev) {
        HIPCHK(c->geo.ensure(sizeof(double) * 4 * (size_t)n));
        double *b = c->geo.as<double>();
        HIPCHK(hipMemcpyAsync(b, in, sizeof(double) * 2 * n, hipMemcpyHostToDevice, s));
        din = b;
        dout = b + 2 * n;
    }
    HIPCHK(launch_utm(inverse != 0, din, n, zone, south != 0, dout, s));
    if (!dev) {
        HIPCHK(hipMemcpyAsync(out, dout, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return RSAC_OK;
}

int rsac_dem_ray_intersect(rsac_ctx *c, const double *origins, const double *dirs, int32_t n_rays, const double *dem,
                           int32_t ny, int32_t nx, double y0, double dy, double x0, double dx, int32_t zone,
                           int32_t south, double max_search_dist, double step, int32_t min_steps, uint32_t flags,
                           double *hits_out, int8_t *status_out, void *stream) {
    int r = check_device(c);
    if (r) return r;
    if ((r = reject_fm7("rsac_dem_ray_intersect", flags))) return r;
    if (!origins || !dirs || !dem || !hits_out || !status_out || n_rays < 0 || ny < 2 || nx < 2 || dy == 0.0 ||
        dx == 0.0 || !(step > 0.0) || zone < 1 || zone > 60)
        return fail(RSAC_EINVAL, "bad arguments");
    if (n_rays == 0) return RSAC_OK;
    // int(max_search_dist / step) of the reference's range()
    const double q = max_search_dist / step;
    const int32_t n_steps = q >= 2147483647.0 ? 2147483647 : (q > 0 ? (int32_t)q : 0);
    hipStream_t s = pick_stream(c, stream);
    const bool dev = (flags & RSAC_F_DEVICE_IN) != 0;
    const size_t cells = (size_t)ny * nx;
    const double *d_o = origins, *d_d = dirs, *d_dem = dem;
    double *d_hits = hits_out;
    int8_t *d_st = status_out;
    if (!dev) {
        HIPCHK(c->geo.ensure(sizeof(double) * (9 * (size_t)n_rays + cells) + (size_t)n_rays + 64));
        double *b = c->geo.as<double>();
        double *bo = b, *bd = b + 3 * (size_t)n_rays, *bh = bd + 3 * (size_t)n_rays, *bz = bh + 3 * (size_t)n_rays;
        int8_t *bs = (int8_t *)(bz + cells);
        HIPCHK(hipMemcpyAsync(bo, origins, sizeof(double) * 3 * n_rays, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(bd, dirs, sizeof(double) * 3 * n_rays, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(bz, dem, sizeof(double) * cells, hipMemcpyHostToDevice, s));
        d_o = bo; d_d = bd; d_dem = bz; d_hits = bh; d_st = bs;
    }
    HIPCHK(launch_dem_march(d_o, d_d, n_rays, d_dem, ny, nx, y0, dy, x0, dx, zone, south != 0, n_steps, step,
                            min_steps, d_hits, d_st, s));
    if (!dev) {
        HIPCHK(hipMemcpyAsync(hits_out, d_hits, sizeof(double) * 3 * n_rays, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(status_out, d_st, n_rays, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return RSAC_OK;
}

int rsac_pnp_winner(rsac_ctx *c, const double *pts3d, const double *pts2d, int32_t n, const double K[9], double thr,
                    uint64_t seed, const int64_t *key, double *model_out, uint8_t *mask_out, void *stream) {
    int r = check_device(c);
    if (r) return r;
    if (!pts3d || !pts2d || !K || !key || n < 4) return fail(RSAC_EINVAL, "bad arguments");
    hipStream_t s = pick_stream(c, stream);
    HIPCHK(c->win.ensure(sizeof(double) * (kModelStride + 8)));
    double *rec = c->win.as<double>();
    double *cam = rec + kModelStride;
    const double cm[4] = {K[0], K[4], K[2], K[5]};
    HIPCHK(c->h_small.ensure(64));
    HIPCHK(hipEventSynchronize(c->ev_small));
    double *hc = c->h_small.as<double>();
    memcpy(hc, cm, sizeof cm);
    hc[4] = (double)(float)(thr * thr);
    HIPCHK(hipMemcpyAsync(cam, hc, 5 * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(c->ev_small, s));
    HIPCHK(launch_pnp_winner(pts3d, pts2d, n, cam, seed, key, rec, model_out, mask_out, s));
    return RSAC_OK;
}

int rsac_pnp_local_opt(rsac_ctx *c, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                       const double model_in[12], double thr, uint32_t flags, double model_out[12], int32_t *count_out,
                       int32_t *steps_out, void *stream) {
    int r = check_device(c);
    if (r) return r;
    if ((r = reject_fm7("rsac_pnp_local_opt", flags))) return r;
    if (!K || !model_in || !model_out || n < 1) return fail(RSAC_EINVAL, "bad arguments");
    hipStream_t s = pick_stream(c, stream);
    Staged st;
    r = stage_points(c, pts3d, pts2d, 3, nullptr, 1, n, flags & (RSAC_F_DEVICE_IN | RSAC_F_DEVICE_SOA), s, st);
    if (r) return r;
    r = stage_tables(c, st, K, thr, s);
    if (r) return r;
    r = ensure_hyp_buffers(c, 1, 1, false);
    if (r) return r;
    PnpArgs a;
    r = pnp_args(c, st, flags | RSAC_F_EXACT_ONLY, 0, 1, 0, s, a);
    if (r) return r;
    double rec[kModelStride] = {0};
    memcpy(rec, model_in, 12 * sizeof(double));
    rec[kValidSlot] = 1.0;
    HIPCHK(hipMemcpyAsync(c->models.p, rec, sizeof rec, hipMemcpyHostToDevice, s));
    // the model's own count starts the chain (local_opt recounts it on the device)
    HIPCHK(c->lo.ensure(2 * sizeof(double) * kModelStride + 64 + 2 * (size_t)n));
    int32_t *cnt = (int32_t *)(c->lo.as<double>() + 2 * kModelStride);
    HIPCHK(hipMemsetAsync(cnt, 0, sizeof(int32_t), s));
    HIPCHK(launch_pnp_model_count(a, n, c->models.as<double>(), (uint8_t *)(cnt + 16), cnt, s));
    int32_t c0 = 0;
    HIPCHK(hipMemcpyAsync(&c0, cnt, sizeof c0, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ScanState sc;
    int32_t steps = 0;
    r = with_one_refit_block(c, [&] {
        // from the input model each time (a failed chain may have replaced the record)
        HIPCHK(hipMemcpyAsync(c->models.p, rec, sizeof rec, hipMemcpyHostToDevice, s));
        sc.reset(1 << 30);
        sc.best = 0;
        sc.max_good = c0;
        steps = 0;
        return local_opt(c, a, n, sc, 0.99, s, steps);
    });
    if (r) return r;
    HIPCHK(hipMemcpyAsync(rec, c->models.p, sizeof rec, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    memcpy(model_out, rec, 12 * sizeof(double));
    if (count_out) *count_out = sc.max_good;
    if (steps_out) *steps_out = steps;
    return RSAC_OK;
}

// LM on (R, t) from the given start over the masked points (NULL = all), on the device: one
// problem's k_pnp_refine, the bits of rsac_pnp_refine (host) and orc_pnp_refine.  Host f64 AoS.
static int refine_on_device(rsac_ctx *c, const double *pts3d, const double *pts2d, int32_t n, const double K[9],
                            const uint8_t *mask, double R[9], double t[3], hipStream_t s) {
    Staged st;
    int r = stage_points(c, pts3d, pts2d, 3, nullptr, 1, n, 0, s, st);
    if (r) return r;
    r = stage_tables(c, st, K, 1.0, s);
    if (r) return r;
    r = ensure_hyp_buffers(c, 1, 1, false);
    if (r) return r;
    PnpArgs a;
    r = pnp_args(c, st, RSAC_F_EXACT_ONLY, 0, 1, 0, s, a);
    if (r) return r;
    HIPCHK(c->h_bestmodels.ensure(sizeof(double) * kModelStride));
    HIPCHK(c->h_mask.ensure(std::max(n, 1)));
    double *hrec = c->h_bestmodels.as<double>();
    memset(hrec, 0, sizeof(double) * kModelStride);
    memcpy(hrec, R, 9 * sizeof(double));
    memcpy(hrec + 9, t, 3 * sizeof(double));
    hrec[kValidSlot] = 1.0;
    uint8_t *hm = c->h_mask.as<uint8_t>();
    if (mask)
        memcpy(hm, mask, n);
    else
        memset(hm, 1, n);
    HIPCHK(c->mask.ensure(std::max(n, 1)));
    HIPCHK(hipMemcpyAsync(c->bestmodels.p, hrec, sizeof(double) * kModelStride, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->mask.p, hm, n, hipMemcpyHostToDevice, s));
    HIPCHK(launch_pnp_refine(a, 1, c->mask.as<uint8_t>(), c->bestmodels.as<double>(), nullptr, s, lm_scratch(c, s),
                             st.off.data(), hrec));  // R, t also written to the pinned record
    HIPCHK(hipStreamSynchronize(s));
    if (int e = lm_check(c)) return e;
    memcpy(R, hrec, 9 * sizeof(double));
    memcpy(t, hrec + 9, 3 * sizeof(double));
    return RSAC_OK;
}

int rsac_pnp_refine_lm(rsac_ctx *c, const double *pts3d, const double *pts2d, int32_t n, const double K[9],
                       const uint8_t *mask, double R[9], double t[3], void *stream) {
    int r = check_device(c);
    if (r) return r;
    if (n < 3 || !pts3d || !pts2d || !K || !R || !t) return fail(RSAC_EINVAL, "bad arguments");
    const double R0[9] = {R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8]}, t0[3] = {t[0], t[1], t[2]};
    return with_one_refit_block(c, [&] {
        memcpy(R, R0, sizeof R0);
        memcpy(t, t0, sizeof t0);
        return refine_on_device(c, pts3d, pts2d, n, K, mask, R, t, pick_stream(c, stream));
    });
}

int rsac_pnp_reprojection_errors(rsac_ctx *c, const double *pts3d, const double *pts2d, int32_t n, const double K[9],
                                 const double R[9], const double t[3], uint32_t flags, double *proj_out,
                                 double *err_out, void *stream) {
    int r = check_device(c);
    if (r) return r;
    if ((r = reject_fm7("rsac_pnp_reprojection_errors", flags))) return r;
    if (n < 0 || !pts3d || !pts2d || !K || !R || !t) return fail(RSAC_EINVAL, "bad arguments");
    if (n == 0) return RSAC_OK;
    hipStream_t s = pick_stream(c, stream);
    PoseCam pc;
    memcpy(pc.R, R, sizeof pc.R);
    memcpy(pc.t, t, sizeof pc.t);
    pc.cam[0] = K[0]; pc.cam[1] = K[4]; pc.cam[2] = K[2]; pc.cam[3] = K[5];
    if (flags & RSAC_F_DEVICE_IN)  // device inputs and outputs: enqueue only
        return launch_pnp_reproj(pts3d, pts2d, n, pc, proj_out, err_out, s) == hipSuccess
                   ? RSAC_OK
                   : fail(RSAC_EHIP, "reprojection launch failed");
    const size_t N = (size_t)n;
    HIPCHK(c->reproj.ensure(sizeof(double) * 8 * N));
    double *d3 = c->reproj.as<double>(), *d2 = d3 + 3 * N, *dp = d2 + 2 * N, *de = dp + 2 * N;
    HIPCHK(hipMemcpyAsync(d3, pts3d, sizeof(double) * 3 * N, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d2, pts2d, sizeof(double) * 2 * N, hipMemcpyHostToDevice, s));
    HIPCHK(launch_pnp_reproj(d3, d2, n, pc, proj_out ? dp : nullptr, err_out ? de : nullptr, s));
    if (proj_out) HIPCHK(hipMemcpyAsync(proj_out, dp, sizeof(double) * 2 * N, hipMemcpyDeviceToHost, s));
    if (err_out) HIPCHK(hipMemcpyAsync(err_out, de, sizeof(double) * N, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RSAC_OK;
}

int rsac_pnp_reprojection_errors_dist(rsac_ctx *c, const double *pts3d, const double *pts2d, int32_t n,
                                      const double K[9], const double *dist, int32_t n_dist, const double R[9],
                                      const double t[3], uint32_t flags, double *proj_out, double *err_out,
                                      void *stream) {
    DistK kd;
    bool active = false;
    if (int r = parse_dist_for("rsac_pnp_reprojection_errors_dist", dist, n_dist, 0, kd, active)) return r;
    if (!active) return rsac_pnp_reprojection_errors(c, pts3d, pts2d, n, K, R, t, flags, proj_out, err_out, stream);
    int r = check_device(c);
    if (r) return r;
    if ((r = reject_fm7("rsac_pnp_reprojection_errors_dist", flags))) return r;
    if (n < 0 || !pts3d || !pts2d || !K || !R || !t) return fail(RSAC_EINVAL, "bad arguments");
    if (n == 0) return RSAC_OK;
    hipStream_t s = pick_stream(c, stream);
    PoseCam pc;
    memcpy(pc.R, R, sizeof pc.R);
    memcpy(pc.t, t, sizeof pc.t);
    pc.cam[0] = K[0]; pc.cam[1] = K[4]; pc.cam[2] = K[2]; pc.cam[3] = K[5];
    const bool rational = n_dist == 8;
    if (flags & RSAC_F_DEVICE_IN)  // device inputs and outputs: enqueue only
        return launch_pnp_reproj_dist(pts3d, pts2d, n, pc, kd, rational, proj_out, err_out, s) == hipSuccess
                   ? RSAC_OK
                   : fail(RSAC_EHIP, "reprojection launch failed");
    const size_t N = (size_t)n;
    HIPCHK(c->reproj.ensure(sizeof(double) * 8 * N));
    double *d3 = c->reproj.as<double>(), *d2 = d3 + 3 * N, *dp = d2 + 2 * N, *de = dp + 2 * N;
    HIPCHK(hipMemcpyAsync(d3, pts3d, sizeof(double) * 3 * N, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d2, pts2d, sizeof(double) * 2 * N, hipMemcpyHostToDevice, s));
    HIPCHK(launch_pnp_reproj_dist(d3, d2, n, pc, kd, rational, proj_out ? dp : nullptr, err_out ? de : nullptr, s));
    if (proj_out) HIPCHK(hipMemcpyAsync(proj_out, dp, sizeof(double) * 2 * N, hipMemcpyDeviceToHost, s));
    if (err_out) HIPCHK(hipMemcpyAsync(err_out, de, sizeof(double) * N, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RSAC_OK;
}

int rsac_pnp_orientation_sweep(rsac_ctx *c, const double *pts3d, const double *pts2d, int32_t n, const double *Ks,
                               int32_t n_k, int32_t n_iters, double thr, double conf, uint64_t seed, uint32_t flags,
                               int32_t min_inliers, int32_t *best_out, double *mean_err_out, double *models_out,
                               int32_t *status_out, int32_t *n_inliers_out, uint8_t *masks_out, double R_out[9],
                               double t_out[3], void *stream) {
    int r = check_device(c);
    if (r) return r;
    if ((r = reject_fm7("rsac_pnp_orientation_sweep", flags))) return r;
    if (n < 4) return fail(RSAC_ETOOFEW, "solvePnPRansac needs >= 4 correspondences (got %d)", n);
    if (n_k < 1 || !pts3d || !pts2d || !Ks || !best_out) return fail(RSAC_EINVAL, "bad arguments");
    // solvePnPRefineLM on the winner needs >= 3 inliers: a lower gate would fail only after the sweep
    if (min_inliers < 3) return fail(RSAC_EINVAL, "min_inliers must be >= 3 (got %d)", min_inliers);
    if (flags & (RSAC_F_DEVICE_IN | RSAC_F_DEVICE_SOA | RSAC_F_DEVICE_OUT | RSAC_F_LO | RSAC_F_ASYNC))
        return fail(RSAC_EINVAL, "the K sweep takes host arrays (no device, LO or async flags)");
    if (flags & RSAC_F_MSAC) return fail(RSAC_EINVAL, "RSAC_F_MSAC is not supported by rsac_pnp_orientation_sweep");
    hipStream_t s = pick_stream(c, stream);
    const size_t N = (size_t)n, P = (size_t)n_k;
    // 1. the loop over the intrinsics (testpro-K.py:58-75) as one batched call: problem k is the
    //    point set with K_k
    std::vector<double> p3(3 * N * P), p2(2 * N * P);
    std::vector<int64_t> off(P + 1);
    for (size_t k = 0; k < P; ++k) {
        memcpy(&p3[3 * N * k], pts3d, sizeof(double) * 3 * N);
        memcpy(&p2[2 * N * k], pts2d, sizeof(double) * 2 * N);
        off[k] = (int64_t)(N * k);
    }
    off[P] = (int64_t)(N * P);
    std::vector<double> R(9 * P), t(3 * P);
    std::vector<int32_t> status(P), ninl(P);
    std::vector<uint8_t> masks(N * P);
    r = rsac_pnp_ransac_batched(c, p3.data(), p2.data(), off.data(), n_k, Ks, n_iters, thr, conf, seed, flags, R.data(),
                                t.data(), status.data(), ninl.data(), masks.data(), stream);
    if (r < 0) return r;
    // 2. the gate (testpro-K.py:77) and each pose as projectPoints sees it: the shim returns
    //    rvec = Rodrigues(R), and projectPoints rotates by Rodrigues(rvec)
    std::vector<double> poses(12 * P, 0.0), cams(4 * P);
    std::vector<uint8_t> pass(P);
    for (size_t k = 0; k < P; ++k) {
        pass[k] = status[k] == RSAC_OK && ninl[k] >= min_inliers;
        double rv[3];
        rodrigues_m2v(&R[9 * k], rv);
        rodrigues_v2m(rv, &poses[12 * k]);
        memcpy(&poses[12 * k + 9], &t[3 * k], 3 * sizeof(double));
        const double *Kk = Ks + 9 * k;
        cams[4 * k] = Kk[0]; cams[4 * k + 1] = Kk[4]; cams[4 * k + 2] = Kk[2]; cams[4 * k + 3] = Kk[5];
    }
    // 3. the mean inlier reprojection error of every K on the device (testpro-K.py:80-82)
    HIPCHK(c->reproj.ensure(sizeof(double) * (5 * N + 16 * P + 2 * P) + N * P));
    double *d3 = c->reproj.as<double>(), *d2 = d3 + 3 * N, *dposes = d2 + 2 * N, *dcams = dposes + 12 * P,
           *dout = dcams + 4 * P;
    uint8_t *dmasks = (uint8_t *)(dout + 2 * P);
    HIPCHK(hipMemcpyAsync(d3, pts3d, sizeof(double) * 3 * N, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d2, pts2d, sizeof(double) * 2 * N, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dposes, poses.data(), sizeof(double) * 12 * P, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dcams, cams.data(), sizeof(double) * 4 * P, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dmasks, masks.data(), N * P, hipMemcpyHostToDevice, s));
    HIPCHK(launch_pnp_reproj_mean(d3, d2, n, n_k, dposes, dcams, dmasks, dout, s));
    std::vector<double> sums(2 * P);
    HIPCHK(hipMemcpyAsync(sums.data(), dout, sizeof(double) * 2 * P, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    // 4. the first K with the strictly smallest mean (testpro-K.py:90-97)
    int best = -1;
    double best_err = __builtin_inf();
    for (size_t k = 0; k < P; ++k) {
        const double mean = sums[2 * k] / sums[2 * k + 1];
        if (mean_err_out) mean_err_out[k] = pass[k] ? mean : __builtin_nan("");
        if (pass[k] && mean < best_err) {
            best_err = mean;
            best = (int)k;
        }
    }
    *best_out = best;
    for (size_t k = 0; k < P; ++k) {
        if (models_out) {
            memcpy(models_out + 12 * k, &R[9 * k], 9 * sizeof(double));
            memcpy(models_out + 12 * k + 9, &t[3 * k], 3 * sizeof(double));
        }
        if (status_out) status_out[k] = pass[k] ? RSAC_OK : RSAC_NO_MODEL;
        if (n_inliers_out) n_inliers_out[k] = ninl[k];
    }
    if (masks_out) memcpy(masks_out, masks.data(), N * P);
    if (best < 0) return RSAC_NO_MODEL;
    // 5. solvePnPRefineLM on the winner's inliers from its pose (testpro-K.py:122-125): the
    //    reference passes the inlier subset, in index order, and the rvec of step 2
    std::vector<double> s3, s2;
    for (size_t i = 0; i < N; ++i)
        if (masks[N * best + i]) {
            s3.insert(s3.end(), pts3d + 3 * i, pts3d + 3 * i + 3);
            s2.insert(s2.end(), pts2d + 2 * i, pts2d + 2 * i + 2);
        }
    double Rr[9], tr[3];
    memcpy(Rr, &poses[12 * best], sizeof Rr);
    memcpy(tr, &poses[12 * best + 9], sizeof tr);
    r = rsac_pnp_refine_lm(c, s3.data(), s2.data(), (int32_t)(s3.size() / 3), Ks + 9 * best, nullptr, Rr, tr, stream);
    if (r < 0) return r;
    if (R_out) memcpy(R_out, Rr, sizeof Rr);
    if (t_out) memcpy(t_out, tr, sizeof tr);
    return RSAC_OK;
}

static int score_poses_core(rsac_ctx *c, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                            const double *poses, int32_t n_poses, double thr, uint32_t flags, int32_t *counts_out,
                            void *stream, const DistK *dist, int32_t n_dist, int64_t *costs_out = nullptr) {
    int r = check_device(c);
    if (r) return r;
    if ((r = reject_fm7("the pose scorers", flags))) return r;
    if (dist || costs_out) flags |= RSAC_F_EXACT_ONLY;  // (the MSAC costs come with the all-f64 test)
    if (n_poses <= 0 || !poses || !counts_out || !K) return fail(RSAC_EINVAL, "bad arguments");
    if (costs_out) {
        r = check_msac_thr("rsac_score_poses_msac", thr);
        if (r) return r;
    }
    hipStream_t s = pick_stream(c, stream);
    Staged st;
    r = stage_points(c, pts3d, pts2d, 3, nullptr, 1, n, flags, s, st);
    if (r) return r;
    r = stage_tables(c, st, K, thr, s);
    if (r) return r;
    r = ensure_hyp_buffers(c, 1, n_poses, false);
    if (r) return r;
    std::vector<double> rec((size_t)n_poses * kModelStride, 0.0);
    for (int32_t h = 0; h < n_poses; ++h) {
        memcpy(&rec[(size_t)h * kModelStride], poses + 12 * h, 12 * sizeof(double));
        rec[(size_t)h * kModelStride + kValidSlot] = 1.0;
    }
    HIPCHK(hipMemcpyAsync(c->models.p, rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(c->status.p, 1, (size_t)n_poses, s));  // every pose valid (the scorers read status)
    PnpArgs a;
    r = pnp_args(c, st, flags, 0, n_poses, 0, s, a, nullptr, false, dist != nullptr);
    if (r) return r;
    if (dist) {
        r = dist_setup(c, st, K, *dist, n_dist, a, s);
        if (r) return r;
    }
    a.counts_out = nullptr;  // no solve kernel zeroes the counts here
    if (a.fmodels) HIPCHK(launch_pnp_fmodels(a, 1, n_poses, s));
    if (costs_out) {
        HIPCHK(c->costs.ensure(sizeof(int64_t) * (size_t)n_poses));
        HIPCHK(launch_pnp_cost(a, 1, 0, n_poses, c->counts.as<int32_t>(), c->costs.as<int64_t>(), s));
    } else {
        HIPCHK(launch_pnp_score(a, 1, 0, n_poses, c->counts.as<int32_t>(), s));
    }
    HIPCHK(hipStreamSynchronize(s));  // rec (host vector) must outlive the async copy
    if (costs_out)
        HIPCHK(hipMemcpyAsync(costs_out, c->costs.p, sizeof(int64_t) * n_poses, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(counts_out, c->counts.p, sizeof(int32_t) * n_poses, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RSAC_OK;
}

int rsac_score_poses(rsac_ctx *c, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                     const double *poses, int32_t n_poses, double thr, uint32_t flags, int32_t *counts_out,
                     void *stream) {
    return score_poses_core(c, pts3d, pts2d, n, K, poses, n_poses, thr, flags, counts_out, stream, nullptr, 0);
}

int rsac_score_poses_msac(rsac_ctx *c, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                          const double *poses, int32_t n_poses, double thr, uint32_t flags, int32_t *counts_out,
                          int64_t *costs_out, void *stream) {
    if (!costs_out) return fail(RSAC_EINVAL, "rsac_score_poses_msac: costs_out required");
    return score_poses_core(c, pts3d, pts2d, n, K, poses, n_poses, thr, flags, counts_out, stream, nullptr, 0,
                            costs_out);
}

int rsac_score_poses_dist(rsac_ctx *c, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                          const double *dist, int32_t n_dist, const double *poses, int32_t n_poses, double thr,
                          uint32_t flags, int32_t *counts_out, void *stream) {
    DistK kd;
    bool active = false;
    if (int r = parse_dist_for("rsac_score_poses_dist", dist, n_dist, flags, kd, active)) return r;
    return score_poses_core(c, pts3d, pts2d, n, K, poses, n_poses, thr, flags, counts_out, stream,
                            active ? &kd : nullptr, n_dist);
}

int rsac_pnp_evaluate_range(rsac_ctx *c, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                            int64_t hyp_begin, int64_t n_hyps, double thr, uint64_t seed, uint32_t flags,
                            int64_t *key_out, double model_out[12], uint8_t *mask_out, rsac_stats *stats,
                            void *stream) {
    int r = check_device(c);
    if (r) return r;
    if ((r = reject_fm7("rsac_pnp_evaluate_range", flags))) return r;
    if (n < 4) return fail(RSAC_ETOOFEW, "need >= 4 correspondences");
    if (n_hyps <= 0 || n_hyps > INT32_MAX || !K || !key_out) return fail(RSAC_EINVAL, "bad arguments");
    if ((flags & RSAC_F_ASYNC) && mask_out && !(flags & RSAC_F_DEVICE_OUT))
        return fail(RSAC_EINVAL, "RSAC_F_ASYNC needs a device mask (RSAC_F_DEVICE_OUT)");
    if (flags & RSAC_F_MSAC) return fail(RSAC_EINVAL, "RSAC_F_MSAC is not supported by rsac_pnp_evaluate_range");
    hipStream_t s = pick_stream(c, stream);
    // the previous call's set-up record (staging clears the context's; this call's replaces it at
    // its end) and this call's: RSAC_F_POINTS_UNCHANGED lets an equal one stand in for the launch
    const SetupRecord prev = c->setup_rec;
    const bool unchanged = (flags & RSAC_F_POINTS_UNCHANGED) != 0;
    flags &= ~RSAC_F_POINTS_UNCHANGED;
    c->setup_reused = false;
    SetupRecord made;
    made.p3 = pts3d;
    made.p2 = pts2d;
    made.n = n;
    made.cam[0] = K[0]; made.cam[1] = K[4]; made.cam[2] = K[2]; made.cam[3] = K[5];
    made.thr2 = (float)(thr * thr);
    made.flags = flags & kSetupFlags;
    made.stream = s;
    Staged st;
    // device f64 inputs: the f32 conversion is fused into the frame launch of pnp_args
    r = stage_points(c, pts3d, pts2d, 3, nullptr, 1, n, flags & ~RSAC_F_SAMPLER_OPENCV, s, st, true);
    if (r) return r;
    r = stage_tables(c, st, K, thr, s);
    if (r) return r;
    r = ensure_hyp_buffers(c, 1, n_hyps, false);
    if (r) return r;
    // the best key is reduced inside the scoring kernel; only 8 bytes + the
    // winner's record (+ its mask, computed on the device) leave the GPU
    unsigned long long *dkey = (unsigned long long *)c->best.p;
    PnpArgs a;
    r = pnp_args(c, st, flags, seed, n_hyps, hyp_begin, s, a, dkey, false, false, unchanged ? &prev : nullptr, &made);
    if (r) return r;
    const int32_t H = (int32_t)n_hyps;
    r = ensure_epnp5(c, a, 1, H);
    if (r) return r;
    // only the best key leaves this call: the bounded sequence where the problem allows it and its
    // size pays the extra launches (RSAC_DBG_BOUND overrides the size rule)
    HIPCHK(c->bound.ensure(64 + sizeof(int32_t) * (size_t)H));
    // two plan records alternate by bounded call (the one the previous call wrote holds the hint)
    static_assert(2 * kBoundPlanStride * sizeof(int32_t) <= 64, "the plan records lie before the list");
    const int rec_prev = c->bound_rec, rec_cur = rec_prev ^ 1;
    a.bound_plan = c->bound.as<int32_t>() + kBoundPlanStride * rec_cur;
    a.bound_list = c->bound.as<int32_t>() + 16;
    a.bound_exact = c->dbg_bound_slab;
    a.bound_p2_min = c->dbg_bound_p2_min;
    const bool bounded = c->dbg_bound != 2 && pnp_score_boundable(a, 1, H, c->dbg_bound == 1);
    // the hinted sequence: the same problem as the previous call of this context (the set-up record,
    // whatever the caller promises about the points' values: for an in-range problem a stale hint
    // only costs time, and the kernels ignore it for a problem outside the f16 range), which
    // ran the bounded sequence and left its record in this allocation
    const int32_t *hint = nullptr;
    if (bounded && pnp_bound_hint_built() && made.same(prev) && c->bound_last && c->bound_hint_gen == c->bound.gen) {
        hint = c->bound.as<int32_t>() + kBoundPlanStride * rec_prev;
        a.zero_word = pnp_bound_survivors_word(a.bound_plan);  // by the solve launch's first thread
    }
    c->bound_hinted = hint != nullptr;
    c->bound_last = bounded;
    c->bound_last_n = n;
    c->bound_last_h = H;
    c->bound_last_exact = a.bound_exact;
    if (bounded) {
        c->bound_rec = rec_cur;
        c->bound_hint_gen = c->bound.gen;
    }
    const auto score = [&](const PnpArgs &as) {
        return bounded ? launch_pnp_score_bounded(as, H, c->counts.as<int32_t>(), s, hint)
                       : launch_pnp_score(as, 1, 0, H, c->counts.as<int32_t>(), s);
    };
    const bool async = (flags & RSAC_F_ASYNC) != 0;
    // timing events only for a synchronous call that reports stats: each event record in the
    // stream costs a gap of several microseconds between the kernels around it
    const bool timed = stats != nullptr && !async;
    if (timed) HIPCHK(hipEventRecord(c->ev0, s));
    HIPCHK(launch_pnp_solve(a, 1, 0, H, s));
    if (timed) HIPCHK(hipEventRecord(c->ev1, s));
    if (timed) {  // score_ms = the scoring launches alone (ev1 -> ev2), then the key's reduction
        PnpArgs ak = a;
        ak.best_key = nullptr;
        HIPCHK(score(ak));
        HIPCHK(hipEventRecord(c->ev2, s));
        HIPCHK(launch_pnp_best_key(a, 0, H, c->counts.as<int32_t>(), s));
    } else {
        HIPCHK(score(a));
    }
    uint8_t *hmask_dev = nullptr;
    if (mask_out) {
        if (flags & RSAC_F_DEVICE_OUT) {
            hmask_dev = mask_out;
        } else {
            HIPCHK(c->mask.ensure(std::max(n, 1)));
            hmask_dev = c->mask.as<uint8_t>();
        }
    }
    HIPCHK(launch_pnp_key_finish(a, n, dkey, hmask_dev, c->bestmodels.as<double>(), async ? model_out : nullptr,
                                 async ? key_out : nullptr, s));
    c->setup_rec = made;  // (valid only for the device-f64 set-up: pnp_args)
    if (async) {
        // results stay on the device and nothing waits: the raw packed key (0 = no model) and
        // the winner's R, t were written to the caller's device buffers in stream order
        if (stats) memset(stats, 0, sizeof(*stats));
        return RSAC_OK;
    }
    HIPCHK(c->h_bestmodels.ensure(sizeof(double) * (kModelStride + 2)));
    double *hb = c->h_bestmodels.as<double>();
    HIPCHK(hipMemcpyAsync(hb, c->bestmodels.p, sizeof(double) * kModelStride, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hb + kModelStride, dkey, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if (mask_out && !(flags & RSAC_F_DEVICE_OUT)) {
        HIPCHK(c->h_mask.ensure(std::max(n, 1)));
        HIPCHK(hipMemcpyAsync(c->h_mask.p, hmask_dev, n, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (mask_out && !(flags & RSAC_F_DEVICE_OUT)) memcpy(mask_out, c->h_mask.p, n);
    unsigned long long key;
    memcpy(&key, hb + kModelStride, sizeof key);
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        add_times(c, stats->gpu_ms, stats->solve_ms, stats->score_ms);
        stats->hyps_scored = H;
        stats->rounds = 1;
    }
    if (key == 0) {
        *key_out = -1;
        if (stats) stats->best_hyp = -1;
        return RSAC_NO_MODEL;
    }
    *key_out = (int64_t)key;
    if (stats) {
        const uint64_t low = 0xFFFFFFFFull - (key & 0xFFFFFFFFull);
        stats->best_hyp = (int64_t)(((uint64_t)hyp_begin & ~0xFFFFFFFFull) | low);
        stats->n_inliers = (int32_t)(key >> 32);
    }
    if (model_out) memcpy(model_out, hb, 12 * sizeof(double));
    return RSAC_OK;
}

static int hypotheses_core(rsac_ctx *c, Model model, const void *a_pts, const void *b_pts, int32_t n, const double *K,
                           int64_t hyp_begin, int32_t H, double thr, uint64_t seed, uint32_t flags,
                           const int32_t *subsets, int32_t *counts_out, int8_t *status_out, double *models_out,
                           void *stream, int32_t *rows_out = nullptr, const DistK *dist = nullptr,
                           int32_t n_dist = 0, int64_t *costs_out = nullptr) {
    int r = check_device(c);
    if (r) return r;
    if (dist) flags |= RSAC_F_EXACT_ONLY;  // lens distortion: the all-f64 distorted test
    if (flags & RSAC_F_MSAC)
        return fail(RSAC_EINVAL, "RSAC_F_MSAC is not a flag of the hypothesis probes (rsac_pnp_hypotheses_msac, "
                                 "rsac_homography_hypotheses_msac and rsac_fundamental_hypotheses_msac return the "
                                 "costs)");
    if (costs_out && model == Model::PnP) {  // rsac_pnp_hypotheses_msac: the all-f64 test and the costs
        r = check_msac_thr("rsac_pnp_hypotheses_msac", thr);
        if (r) return r;
        flags |= RSAC_F_EXACT_ONLY;
    }
    if (costs_out && model == Model::Hom) {  // rsac_homography_hypotheses_msac (thr as given: no default here)
        r = check_msac_thr("rsac_homography_hypotheses_msac", thr);
        if (r) return r;
    }
    if (costs_out && model == Model::Fm) {  // rsac_fundamental_hypotheses_msac: the exact path (k_fm_cost)
        r = check_msac_thr("rsac_fundamental_hypotheses_msac", thr);
        if (r) return r;
        flags |= RSAC_F_EXACT_ONLY;
    }
    if (H <= 0 || (!rows_out && (!counts_out || !status_out))) return fail(RSAC_EINVAL, "bad arguments");
    if (model != Model::Fm)
        if (int e = reject_fm7("the PnP and homography hypothesis probes", flags)) return e;
    // RSAC_F_FM_7POINT: hyp_begin and the caller's H count samples, the outputs hold 3 rows for each
    const int rps = records_per_sample(model, flags);
    if ((int64_t)H * rps > INT32_MAX) return fail(RSAC_EINVAL, "too many hypotheses");
    H *= rps;
    if (model == Model::PnP && !K) return fail(RSAC_EINVAL, "K required");
    if (model == Model::Fm && subsets) return fail(RSAC_EINVAL, "the fundamental-matrix sampler is Philox only");
    hipStream_t s = pick_stream(c, stream);
    Staged st;
    r = stage_points(c, a_pts, b_pts, model == Model::PnP ? 3 : 2, nullptr, 1, n, flags, s, st);
    if (r) return r;
    r = stage_tables(c, st, K, thr, s);
    if (r) return r;
    r = ensure_hyp_buffers(c, 1, H, subsets != nullptr);
    if (r) return r;
    if (subsets) {  // (5 indices per subset for PnP's EPnP-5 kernel)
        r = upload_subsets(c, subsets, H, model == Model::PnP && (flags & RSAC_F_MINIMAL_EPNP5) ? 5 : 4, n, s);
        if (r) return r;
    }
    if (model == Model::PnP) {
        PnpArgs a;
        r = pnp_args(c, st, flags, seed, H, hyp_begin, s, a, nullptr, false, dist != nullptr);
        if (r) return r;
        if (dist) {
            r = dist_setup(c, st, K, *dist, n_dist, a, s);
            if (r) return r;
        }
        a.subsets = subsets ? c->subsets.as<int32_t>() : nullptr;
        a.sub_status = subsets ? c->substatus.as<int8_t>() : nullptr;
        r = ensure_epnp5(c, a, 1, H);
        if (r) return r;
        HIPCHK(launch_pnp_solve(a, 1, 0, H, s));
        if (costs_out) {
            HIPCHK(c->costs.ensure(sizeof(int64_t) * (size_t)H));
            HIPCHK(launch_pnp_cost(a, 1, 0, H, c->counts.as<int32_t>(), c->costs.as<int64_t>(), s));
        } else {
            HIPCHK(launch_pnp_score(a, 1, 0, H, c->counts.as<int32_t>(), s));
        }
    } else {
        HomArgs a = hom_args(c, st, seed, hyp_begin, H, subsets != nullptr);
        if (model == Model::Fm) {
            r = fm_prefilter(c, a, 1, flags, s);
            if (r) return r;
            HIPCHK(fm_solve(c, a, 1, 0, H, s, fm_sample_size(flags)));
            if (costs_out) {
                HIPCHK(c->costs.ensure(sizeof(int64_t) * (size_t)H));
                HIPCHK(launch_fm_cost(a, 1, 0, H, c->counts.as<int32_t>(), c->costs.as<int64_t>(), s));
            } else {
                HIPCHK(launch_fm_score(a, 1, 0, H, c->counts.as<int32_t>(), s));
            }
        } else {
            HIPCHK(launch_hom_solve(a, 1, 0, H, s));
            if (costs_out) {
                HIPCHK(c->costs.ensure(sizeof(int64_t) * (size_t)H));
                HIPCHK(launch_hom_cost(a, 1, 0, H, c->counts.as<int32_t>(), c->costs.as<int64_t>(), s));
            } else {
                HIPCHK(launch_hom_score(a, 1, 0, H, c->counts.as<int32_t>(), s));
            }
        }
    }
    if (flags & RSAC_F_DEVICE_OUT) {  // device outputs: enqueued, no wait
        if (rows_out) {
            HIPCHK(launch_pack_rows(c->status.as<int8_t>(), c->counts.as<int32_t>(), H, rows_out, s));
        } else {
            HIPCHK(hipMemcpyAsync(counts_out, c->counts.p, sizeof(int32_t) * H, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(status_out, c->status.p, H, hipMemcpyDeviceToDevice, s));
        }
        if (models_out)
            HIPCHK(hipMemcpyAsync(models_out, c->models.p, sizeof(double) * kModelStride * H,
                                  hipMemcpyDeviceToDevice, s));
        if (costs_out)
            HIPCHK(hipMemcpyAsync(costs_out, c->costs.p, sizeof(int64_t) * H, hipMemcpyDeviceToDevice, s));
        return RSAC_OK;
    }
    if (costs_out) HIPCHK(hipMemcpyAsync(costs_out, c->costs.p, sizeof(int64_t) * H, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(counts_out, c->counts.p, sizeof(int32_t) * H, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(status_out, c->status.p, H, hipMemcpyDeviceToHost, s));
    if (models_out)
        HIPCHK(hipMemcpyAsync(models_out, c->models.p, sizeof(double) * kModelStride * H, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    // PnP hypothesis records leave the validity slot to the status byte: filled in for the caller
    if (models_out && model == Model::PnP)
        for (int64_t h = 0; h < H; ++h) models_out[h * kModelStride + kValidSlot] = status_out[h] > 0 ? 1.0 : 0.0;
    return RSAC_OK;
}

int rsac_pnp_hypotheses(rsac_ctx *c, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                        int64_t hyp_begin, int32_t n_hyps, double thr, uint64_t seed, uint32_t flags,
                        const int32_t *subsets, int32_t *counts_out, int8_t *status_out, double *models_out,
                        void *stream) {
    return hypotheses_core(c, Model::PnP, pts3d, pts2d, n, K, hyp_begin, n_hyps, thr, seed, flags, subsets,
                           counts_out, status_out, models_out, stream);
}

int rsac_pnp_hypotheses_msac(rsac_ctx *c, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                             int64_t hyp_begin, int32_t n_hyps, double thr, uint64_t seed, uint32_t flags,
                             const int32_t *subsets, int32_t *counts_out, int8_t *status_out, double *models_out,
                             int64_t *costs_out, void *stream) {
    if (!costs_out) return fail(RSAC_EINVAL, "rsac_pnp_hypotheses_msac: costs_out required");
    return hypotheses_core(c, Model::PnP, pts3d, pts2d, n, K, hyp_begin, n_hyps, thr, seed, flags, subsets,
                           counts_out, status_out, models_out, stream, nullptr, nullptr, 0, costs_out);
}

int rsac_pnp_hypotheses_dist(rsac_ctx *c, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                             const double *dist, int32_t n_dist, int64_t hyp_begin, int32_t n_hyps, double thr,
                             uint64_t seed, uint32_t flags, const int32_t *subsets, int32_t *counts_out,
                             int8_t *status_out, double *models_out, void *stream) {
    DistK kd;
    bool active = false;
    if (int r = parse_dist_for("rsac_pnp_hypotheses_dist", dist, n_dist, flags, kd, active)) return r;
    if (!active)
        return rsac_pnp_hypotheses(c, pts3d, pts2d, n, K, hyp_begin, n_hyps, thr, seed, flags, subsets, counts_out,
                                   status_out, models_out, stream);
    return hypotheses_core(c, Model::PnP, pts3d, pts2d, n, K, hyp_begin, n_hyps, thr, seed, flags, subsets,
                           counts_out, status_out, models_out, stream, nullptr, &kd, n_dist);
}

int rsac_pnp_hypothesis_rows(rsac_ctx *c, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                             int64_t hyp_begin, int32_t n_hyps, double thr, uint64_t seed, uint32_t flags,
                             int32_t *rows_out, void *stream) {
    if (!rows_out) return fail(RSAC_EINVAL, "rows_out required");
    return hypotheses_core(c, Model::PnP, pts3d, pts2d, n, K, hyp_begin, n_hyps, thr, seed, flags | RSAC_F_DEVICE_OUT,
                           nullptr, nullptr, nullptr, nullptr, stream, rows_out);
}

int rsac_scan_device(rsac_ctx *c, rsac_scan_state *st, const int32_t *rows, int64_t count, int32_t n,
                     int32_t model_points, double confidence, int32_t stop_on_improve, int32_t *improved,
                     void *stream) {
    int r = check_device(c);
    if (r) return r;
    if (!st || count < 0 || count > INT32_MAX || n <= 0 || (count > 0 && !rows)) return fail(RSAC_EINVAL, "bad arguments");
    if (improved) *improved = 0;
    if (st->done || count == 0) return RSAC_OK;
    hipStream_t s = pick_stream(c, stream);
    const int32_t floor0 = std::max(st->max_good, model_points - 1);
    HIPCHK(c->h_scanrec.ensure(sizeof(ScanRecords)));
    ScanRecords *rec = c->h_scanrec.as<ScanRecords>();
    HIPCHK(launch_scan_rows(rows, (int32_t)count, floor0, rec, s));
    HIPCHK(hipStreamSynchronize(s));
    if (rec->nrec < 0) {  // more improvements than records: scan the copied rows exactly
        std::vector<int32_t> h(2 * (size_t)count), cn((size_t)count);
        std::vector<int8_t> sv((size_t)count);
        HIPCHK(hipMemcpyAsync(h.data(), rows, sizeof(int32_t) * 2 * count, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int64_t i = 0; i < count; ++i) {
            sv[i] = (int8_t)h[2 * i];
            cn[i] = h[2 * i + 1];
        }
        int32_t imp = 0;
        r = stop_on_improve ? rsac_scan_until_best(st, cn.data(), sv.data(), count, n, model_points, confidence, &imp)
                            : rsac_scan(st, cn.data(), sv.data(), count, n, model_points, confidence);
        if (improved) *improved = imp;
        return r;
    }
    // scan_step over the rows, replayed on the records (rsac_host.hip scan_records)
    ScanState sc;
    sc.niters = st->niters;
    sc.best = st->best;
    sc.max_good = st->max_good;
    sc.iter = st->iter;
    sc.done = st->done != 0;
    scan_records(sc, rec->idx, rec->cnt, rec->nrec, rec->first_neg, count, n, model_points, confidence,
                 stop_on_improve != 0);
    st->niters = sc.niters;
    st->best = sc.best;
    st->max_good = sc.max_good;
    st->iter = sc.iter;
    st->done = sc.done ? 1 : 0;
    if (improved) *improved = sc.improved ? 1 : 0;
    return RSAC_OK;
}

int rsac_homography_hypotheses(rsac_ctx *c, const void *src, const void *dst, int32_t n, int64_t hyp_begin,
                               int32_t n_hyps, double thr, uint64_t seed, uint32_t flags, const int32_t *subsets,
                               int32_t *counts_out, int8_t *status_out, double *models_out, void *stream) {
    return hypotheses_core(c, Model::Hom, src, dst, n, nullptr, hyp_begin, n_hyps, thr, seed, flags, subsets,
                           counts_out, status_out, models_out, stream);
}

int rsac_homography_hypotheses_msac(rsac_ctx *c, const void *src, const void *dst, int32_t n, int64_t hyp_begin,
                                    int32_t n_hyps, double thr, uint64_t seed, uint32_t flags, const int32_t *subsets,
                                    int32_t *counts_out, int8_t *status_out, double *models_out, int64_t *costs_out,
                                    void *stream) {
    if (!costs_out) return fail(RSAC_EINVAL, "rsac_homography_hypotheses_msac: costs_out required");
    return hypotheses_core(c, Model::Hom, src, dst, n, nullptr, hyp_begin, n_hyps, thr, seed, flags, subsets,
                           counts_out, status_out, models_out, stream, nullptr, nullptr, 0, costs_out);
}

int rsac_fundamental_hypotheses(rsac_ctx *c, const void *pts1, const void *pts2, int32_t n, int64_t hyp_begin,
                                int32_t n_hyps, double thr, uint64_t seed, uint32_t flags, int32_t *counts_out,
                                int8_t *status_out, double *models_out, void *stream) {
    if (int r = reject_em5("rsac_fundamental_hypotheses", flags)) return r;
    return hypotheses_core(c, Model::Fm, pts1, pts2, n, nullptr, hyp_begin, n_hyps, thr, seed, flags, nullptr,
                           counts_out, status_out, models_out, stream);
}

int rsac_fundamental_hypotheses_msac(rsac_ctx *c, const void *pts1, const void *pts2, int32_t n, int64_t hyp_begin,
                                     int32_t n_hyps, double thr, uint64_t seed, uint32_t flags, int32_t *counts_out,
                                     int8_t *status_out, double *models_out, int64_t *costs_out, void *stream) {
    if (!costs_out) return fail(RSAC_EINVAL, "rsac_fundamental_hypotheses_msac: costs_out required");
    if (int r = reject_em5("rsac_fundamental_hypotheses_msac", flags)) return r;
    return hypotheses_core(c, Model::Fm, pts1, pts2, n, nullptr, hyp_begin, n_hyps, thr, seed, flags, nullptr,
                           counts_out, status_out, models_out, stream, nullptr, nullptr, 0, costs_out);
}

// rsac_fundamental_ransac, and under kFlagEm5 (c->em_kinv uploaded) the loop of rsac_essential_ransac
static int fm_ransac_core(rsac_ctx *c, const void *pts1, const void *pts2, int32_t n, int32_t max_iters, double thr,
                          double conf, uint64_t seed, uint32_t flags, double F_out[9], uint8_t *mask_out,
                          rsac_stats *stats, void *stream) {
    int r = check_device(c);
    if (r) return r;
    const int sk = fm_sample_size(flags);
    if (n < sk)
        return fail(RSAC_ETOOFEW, "the %d-point %s matrix needs >= %d correspondences (got %d)", sk,
                    sk == 5 ? "essential" : "fundamental", sk, n);
    const bool msac = (flags & RSAC_F_MSAC) != 0;
    r = fm_ransac_flags((flags & kFlagEm5) ? "rsac_essential_ransac" : "rsac_fundamental_ransac", flags);
    if (r) return r;
    // RSAC_F_REFINE: the least-squares fit on the winner's mask after the loop; the loop itself
    // never sees the flag
    const bool refit = (flags & RSAC_F_REFINE) != 0;
    flags &= ~(uint32_t)RSAC_F_REFINE;
    if (msac) {
        r = check_msac_thr("RSAC_F_MSAC", thr);
        if (r) return r;
        flags |= RSAC_F_EXACT_ONLY;  // MSAC implies the exact path (k_fm_cost): no pre-filter, no f32 records
    }
    hipStream_t s = pick_stream(c, stream);
    Staged st;
    r = stage_points(c, pts1, pts2, 2, nullptr, 1, n, flags, s, st);
    if (r) return r;
    r = stage_tables(c, st, nullptr, thr, s);
    if (r) return r;
    const int64_t stride = (int64_t)std::max(max_iters, 1) * records_per_sample(Model::Fm, flags);  // run_loop's H
    r = ensure_hyp_buffers(c, 1, stride, false);
    if (r) return r;
    HomArgs a = hom_args(c, st, seed, 0, stride, false);
    r = fm_prefilter(c, a, 1, flags, s);
    if (r) return r;
    LoopOut lo;  // (its timing stays on: the call always times its rounds)
    r = run_loop(c, Model::Fm, st, a, max_iters, conf, flags, s, lo);
    if (r) return r;
    r = finish_masks(c, Model::Fm, st, &a, lo, stride, mask_out, flags, s);
    if (r) return r;
    const ScanState &sc = lo.scan[0];
    if (F_out) memcpy(F_out, c->h_bestmodels.as<double>(), 9 * sizeof(double));
    if (refit && sc.best >= 0) {  // the mask is read where finish_masks left it; it stays the RANSAC-phase mask
        double res[kFmFitRes];
        r = fm_fit_enqueue(c, st, device_mask_ptr(c, mask_out, flags), res, s);
        if (r) return r;
        HIPCHK(hipStreamSynchronize(s));
        if (F_out && res[9] != 0.0) memcpy(F_out, res, 9 * sizeof(double));  // no model: the minimal F stays
    }
    if (msac) c->last_costs.assign(1, sc.best >= 0 ? lo.best_cost[0] : -1);  // rsac_last_costs
    if (stats) fill_stats(*stats, lo);  // (c->last_stats is the PnP and homography drivers')
    return sc.best >= 0 ? RSAC_OK : RSAC_NO_MODEL;
}

int rsac_fundamental_ransac(rsac_ctx *c, const void *pts1, const void *pts2, int32_t n, int32_t max_iters,
                            double thr, double conf, uint64_t seed, uint32_t flags, double F_out[9],
                            uint8_t *mask_out, rsac_stats *stats, void *stream) {
    if (int r = reject_em5("rsac_fundamental_ransac", flags)) return r;
    return fm_ransac_core(c, pts1, pts2, n, max_iters, thr, conf, seed, flags, F_out, mask_out, stats, stream);
}

// ---------------------------------------------------------------------------
// Essential matrix
// ---------------------------------------------------------------------------
// Kinv1, Kinv2 of P problems (K2s null: K1s for both views) by em5_kinv -> c->em_kinv; the array the
// kernel reads.  hk (non-null): the same 18 P doubles for the caller.
static int em_upload_kinv(rsac_ctx *c, const char *what, const double *K1s, const double *K2s, int32_t P,
                          hipStream_t s, std::vector<double> *hk = nullptr) {
    if (!K1s) return fail(RSAC_EINVAL, "%s: K1 required", what);
    std::vector<double> kinv((size_t)18 * P);
    for (int p = 0; p < P; ++p) {
        const double *K1 = K1s + 9 * (size_t)p, *K2 = K2s ? K2s + 9 * (size_t)p : K1;
        if (!em5_kinv(K1, kinv.data() + 18 * (size_t)p) || !em5_kinv(K2, kinv.data() + 18 * (size_t)p + 9))
            return fail(RSAC_EINVAL, "%s: singular or non-finite intrinsics (problem %d)", what, p);
    }
    HIPCHK(c->em_kinv.ensure(sizeof(double) * kinv.size()));
    HIPCHK(hipMemcpyAsync(c->em_kinv.p, kinv.data(), sizeof(double) * kinv.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));  // kinv leaves scope
    if (hk) hk->swap(kinv);
    return RSAC_OK;
}

constexpr uint32_t kEmRansacFlags = RSAC_F_ADAPTIVE | RSAC_F_MSAC | RSAC_F_REFINE | RSAC_F_EXACT_ONLY |
                                    RSAC_F_DEVICE_IN | RSAC_F_DEVICE_SOA | RSAC_F_DEVICE_OUT;

int rsac_essential_from_fundamental(const double F[9], const double K1[9], const double K2[9], double E_out[9]) {
    if (!F || !K1 || !E_out) return fail(RSAC_EINVAL, "rsac_essential_from_fundamental: bad arguments");
    if (!em5_from_fundamental(F, K1, K2 ? K2 : K1, E_out)) {
        memset(E_out, 0, 9 * sizeof(double));
        return RSAC_NO_MODEL;
    }
    return RSAC_OK;
}

int rsac_essential_ransac(rsac_ctx *c, const void *pts1, const void *pts2, int32_t n, const double K1[9],
                          const double K2[9], int32_t max_iters, double thr, double conf, uint64_t seed,
                          uint32_t flags, double E_out[9], double F_out[9], uint8_t *mask_out, rsac_stats *stats,
                          void *stream) {
    int r = check_device(c);
    if (r) return r;
    if ((r = check_flags("rsac_essential_ransac", flags, kEmRansacFlags))) return r;
    if (!E_out) return fail(RSAC_EINVAL, "rsac_essential_ransac: E_out required");
    if (n < 5) return fail(RSAC_ETOOFEW, "the 5-point essential matrix needs >= 5 correspondences (got %d)", n);
    if ((r = em_upload_kinv(c, "rsac_essential_ransac", K1, K2, 1, pick_stream(c, stream)))) return r;
    double F[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    r = fm_ransac_core(c, pts1, pts2, n, max_iters, thr, conf, seed, flags | kFlagEm5, F, mask_out, stats, stream);
    memset(E_out, 0, 9 * sizeof(double));
    if (F_out) memcpy(F_out, F, sizeof F);
    if (r == RSAC_OK) (void)em5_from_fundamental(F, K1, K2 ? K2 : K1, E_out);
    return r;
}

int rsac_essential_ransac_batched(rsac_ctx *c, const void *pts1, const void *pts2, const int64_t *offsets,
                                  int32_t n_problems, const double *K1s, const double *K2s, int32_t max_iters,
                                  double thr, double conf, uint64_t seed, uint32_t flags, double *E_out, double *F_out,
                                  int32_t *status_out, int32_t *n_inliers_out, uint8_t *mask_out, void *stream) {
    const char *what = "rsac_essential_ransac_batched";
    int r = check_device(c);
    if (r) return r;
    if ((r = check_flags(what, flags, kEmRansacFlags))) return r;
    if (n_problems < 1 || n_problems > kFmBatchMaxP || !offsets || !E_out) return fail(RSAC_EINVAL, "%s: bad arguments", what);
    hipStream_t s = pick_stream(c, stream);
    if ((r = em_upload_kinv(c, what, K1s, K2s, n_problems, s))) return r;
    std::vector<double> F((size_t)9 * n_problems, 0.0);
    std::vector<int32_t> status(n_problems, RSAC_NO_MODEL);
    r = fm_batched_core(c, pts1, pts2, offsets, n_problems, max_iters, thr, conf, seed, flags | kFlagEm5, F.data(),
                        status.data(), n_inliers_out, mask_out, s);
    if (r < 0) return r;
    for (int p = 0; p < n_problems; ++p) {
        double *E = E_out + 9 * (size_t)p;
        memset(E, 0, 9 * sizeof(double));
        const double *K1 = K1s + 9 * (size_t)p;
        if (status[p] == RSAC_OK) (void)em5_from_fundamental(F.data() + 9 * (size_t)p, K1, K2s ? K2s + 9 * (size_t)p : K1, E);
        if (status_out) status_out[p] = status[p];
    }
    if (F_out) memcpy(F_out, F.data(), sizeof(double) * F.size());
    return r;
}

int rsac_essential_hypotheses(rsac_ctx *c, const void *pts1, const void *pts2, int32_t n, const double K1[9],
                              const double K2[9], int64_t hyp_begin, int32_t n_hyps, double thr, uint64_t seed,
                              uint32_t flags, int32_t *counts_out, int8_t *status_out, double *models_out,
                              int64_t *costs_out, void *stream) {
    int r = check_device(c);
    if (r) return r;
    if ((r = check_flags("rsac_essential_hypotheses", flags,
                         RSAC_F_EXACT_ONLY | RSAC_F_DEVICE_IN | RSAC_F_DEVICE_SOA | RSAC_F_DEVICE_OUT)))
        return r;
    if ((r = em_upload_kinv(c, "rsac_essential_hypotheses", K1, K2, 1, pick_stream(c, stream)))) return r;
    return hypotheses_core(c, Model::Fm, pts1, pts2, n, nullptr, hyp_begin, n_hyps, thr, seed, flags | kFlagEm5,
                           nullptr, counts_out, status_out, models_out, stream, nullptr, nullptr, 0, costs_out);
}

int rsac_essential_recover_pose(const double *pts1, const double *pts2, int32_t n, const double K1[9],
                                const double K2[9], const double E[9], const uint8_t *mask, double R_out[9],
                                double t_out[3], int32_t n_front_out[4]) {
    if (n < 0 || (n > 0 && (!pts1 || !pts2)) || !K1 || !E || !R_out || !t_out)
        return fail(RSAC_EINVAL, "rsac_essential_recover_pose: bad arguments");
    double k1[9], k2[9];
    if (!em5_kinv(K1, k1) || !em5_kinv(K2 ? K2 : K1, k2))
        return fail(RSAC_EINVAL, "rsac_essential_recover_pose: singular or non-finite intrinsics");
    for (int k = 0; k < 9; ++k)
        if (!dfinite(E[k])) return fail(RSAC_EINVAL, "rsac_essential_recover_pose: non-finite E");
    const int front = em5_recover_pose(pts1, pts2, n, k1, k2, E, mask, R_out, t_out, n_front_out);
    return front > 0 ? RSAC_OK : RSAC_NO_MODEL;
}

int rsac_poly_real_roots(const double *c, int32_t degree, double *roots_out) {
    if (!c || !roots_out || degree < 0 || degree > 10) return 0;
    double cc[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k <= degree; ++k) cc[k] = c[k];
    return poly10_real_roots(cc, roots_out);
}

int rsac_em_minimal5(const double *pts1, const double *pts2, const double K1[9], const double K2[9], double F_out[90],
                     double E_out[90], int32_t *n_models) {
    if (!pts1 || !pts2 || !K1 || !F_out || !n_models) return fail(RSAC_EINVAL, "rsac_em_minimal5: bad arguments");
    double k1[9], k2[9];
    if (!em5_kinv(K1, k1) || !em5_kinv(K2 ? K2 : K1, k2))
        return fail(RSAC_EINVAL, "rsac_em_minimal5: singular or non-finite intrinsics");
    float x1[5], y1[5], x2[5], y2[5];
    for (int i = 0; i < 5; ++i) {
        x1[i] = (float)pts1[2 * i]; y1[i] = (float)pts1[2 * i + 1];
        x2[i] = (float)pts2[2 * i]; y2[i] = (float)pts2[2 * i + 1];
    }
    double F[90], E[90];
    const int nm = em_minimal5(x1, y1, x2, y2, k1, k2, F, E);
    for (int k = 0; k < 90; ++k) {
        F_out[k] = k < 9 * nm ? F[k] : 0.0;
        if (E_out) E_out[k] = k < 9 * nm ? E[k] : 0.0;
    }
    *n_models = nm;
    return RSAC_OK;
}

static int pnp_mask_core(rsac_ctx *c, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                         const double model[12], double thr, uint32_t flags, uint8_t *mask_out, int32_t *count_out,
                         void *stream, const DistK *dist, int32_t n_dist) {
    int r = check_device(c);
    if (r) return r;
    if ((r = reject_fm7("rsac_pnp_mask", flags))) return r;
    if (!model || !K) return fail(RSAC_EINVAL, "bad arguments");
    hipStream_t s = pick_stream(c, stream);
    Staged st;
    r = stage_points(c, pts3d, pts2d, 3, nullptr, 1, n, flags, s, st);
    if (r) return r;
    r = stage_tables(c, st, K, thr, s);
    if (r) return r;
    r = ensure_hyp_buffers(c, 1, 1, false);
    if (r) return r;
    double rec[kModelStride] = {0};
    memcpy(rec, model, 12 * sizeof(double));
    rec[kValidSlot] = 1.0;
    HIPCHK(hipMemcpyAsync(c->models.p, rec, sizeof rec, hipMemcpyHostToDevice, s));
    int64_t zero = 0;
    HIPCHK(hipMemcpyAsync(c->best.p, &zero, sizeof zero, hipMemcpyHostToDevice, s));
    PnpArgs a{};
    a.X = st.d[0]; a.Y = st.d[1]; a.Z = st.d[2]; a.U = st.d[3]; a.V = st.d[4];
    a.offsets = c->d_off;
    a.max_n = st.max_n();
    a.cams = c->d_cams;
    a.thr2 = c->d_thr2;
    a.models = c->models.as<double>();
    uint8_t *dmask;
    if (flags & RSAC_F_DEVICE_OUT) {
        dmask = mask_out;
    } else {
        HIPCHK(c->mask.ensure(std::max(n, 1)));
        dmask = c->mask.as<uint8_t>();
    }
    if (dist) {  // lens distortion: mask and count in one launch (k_pnp_model_count_dist)
        r = dist_setup(c, st, K, *dist, n_dist, a, s);
        if (r) return r;
        int32_t cnt = 0;
        HIPCHK(hipMemsetAsync(c->counts.p, 0, sizeof(int32_t), s));
        HIPCHK(launch_pnp_model_count(a, n, c->models.as<double>(), dmask, c->counts.as<int32_t>(), s));
        HIPCHK(hipMemcpyAsync(&cnt, c->counts.p, sizeof cnt, hipMemcpyDeviceToHost, s));
        if (mask_out && !(flags & RSAC_F_DEVICE_OUT))
            HIPCHK(hipMemcpyAsync(mask_out, dmask, n, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (count_out) *count_out = cnt;
        return RSAC_OK;
    }
    HIPCHK(launch_pnp_mask(a, 1, n, c->best.as<int64_t>(), dmask, s));
    std::vector<uint8_t> hm(std::max(n, 1));
    HIPCHK(hipMemcpyAsync(hm.data(), dmask, n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (mask_out && !(flags & RSAC_F_DEVICE_OUT)) memcpy(mask_out, hm.data(), n);
    if (count_out) {
        int32_t k = 0;
        for (int i = 0; i < n; ++i) k += hm[i];
        *count_out = k;
    }
    return RSAC_OK;
}

int rsac_pnp_mask(rsac_ctx *c, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                  const double model[12], double thr, uint32_t flags, uint8_t *mask_out, int32_t *count_out,
                  void *stream) {
    return pnp_mask_core(c, pts3d, pts2d, n, K, model, thr, flags, mask_out, count_out, stream, nullptr, 0);
}

int rsac_pnp_mask_dist(rsac_ctx *c, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                       const double *dist, int32_t n_dist, const double model[12], double thr, uint32_t flags,
                       uint8_t *mask_out, int32_t *count_out, void *stream) {
    DistK kd;
    bool active = false;
    if (int r = parse_dist_for("rsac_pnp_mask_dist", dist, n_dist, flags, kd, active)) return r;
    return pnp_mask_core(c, pts3d, pts2d, n, K, model, thr, flags, mask_out, count_out, stream,
                         active ? &kd : nullptr, n_dist);
}

// lens distortion on the host (no GPU needed): rsac_math.h's undistort_point / pnp_reproj_err_dist,
// the source the kernels run
int rsac_undistort_points(const double *pts2d, int32_t n, const double K[9], const double *dist, int32_t n_dist,
                          double *norm_out, float *ideal_out) {
    if (n < 0 || (n > 0 && !pts2d) || !K) return fail(RSAC_EINVAL, "bad arguments");
    DistK kd;
    bool active = false;
    if (int r = parse_dist_for("rsac_undistort_points", dist, n_dist, 0, kd, active)) return r;
    const Cam k{K[0], K[4], K[2], K[5]};
    for (int32_t i = 0; i < n; ++i) {
        double x, y;
        undistort_point(k, kd.k, (double)(float)pts2d[2 * i], (double)(float)pts2d[2 * i + 1], x, y);
        if (norm_out) {
            norm_out[2 * i] = x;
            norm_out[2 * i + 1] = y;
        }
        if (ideal_out) ideal_pixel(k, x, y, ideal_out[2 * i], ideal_out[2 * i + 1]);
    }
    return RSAC_OK;
}

int rsac_undistort_points_device(rsac_ctx *c, const double *pts2d, int32_t n, const double K[9], const double *dist,
                                 int32_t n_dist, uint32_t flags, double *norm_out, float *ideal_out, void *stream) {
    int r = check_device(c);
    if (r) return r;
    if ((r = reject_fm7("rsac_undistort_points_device", flags))) return r;
    if (n < 0 || (n > 0 && !pts2d) || !K) return fail(RSAC_EINVAL, "bad arguments");
    if (flags & ~(uint32_t)RSAC_F_DEVICE_IN)
        return fail(RSAC_EINVAL, "rsac_undistort_points_device: RSAC_F_DEVICE_IN is the only flag");
    DistK kd;
    bool active = false;
    if ((r = parse_dist_for("rsac_undistort_points_device", dist, n_dist, 0, kd, active))) return r;
    if (n == 0) return RSAC_OK;
    hipStream_t s = pick_stream(c, stream);
    const double cam[4] = {K[0], K[4], K[2], K[5]};
    const size_t N = (size_t)n;
    if (flags & RSAC_F_DEVICE_IN)  // device input and outputs: enqueue only
        return launch_pnp_undistort(nullptr, nullptr, pts2d, n, cam, kd, nullptr, nullptr, ideal_out, norm_out,
                                    nullptr, s) == hipSuccess
                   ? RSAC_OK
                   : fail(RSAC_EHIP, "undistort launch failed");
    // host arrays: pts2d | norm | ideal in the scratch
    HIPCHK(c->reproj.ensure(sizeof(double) * 4 * N + sizeof(float) * 2 * N));
    double *d2 = c->reproj.as<double>(), *dn = d2 + 2 * N;
    float *di = (float *)(dn + 2 * N);
    HIPCHK(hipMemcpyAsync(d2, pts2d, sizeof(double) * 2 * N, hipMemcpyHostToDevice, s));
    HIPCHK(launch_pnp_undistort(nullptr, nullptr, d2, n, cam, kd, nullptr, nullptr, ideal_out ? di : nullptr,
                                norm_out ? dn : nullptr, nullptr, s));
    if (norm_out) HIPCHK(hipMemcpyAsync(norm_out, dn, sizeof(double) * 2 * N, hipMemcpyDeviceToHost, s));
    if (ideal_out) HIPCHK(hipMemcpyAsync(ideal_out, di, sizeof(float) * 2 * N, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RSAC_OK;
}

int rsac_project_points_dist(const double *pts3d, int32_t n, const double K[9], const double *dist, int32_t n_dist,
                             const double R[9], const double t[3], double *proj_out) {
    if (n < 0 || (n > 0 && !pts3d) || !K || !R || !t || !proj_out) return fail(RSAC_EINVAL, "bad arguments");
    DistK kd;
    bool active = false;
    if (int r = parse_dist_for("rsac_project_points_dist", dist, n_dist, 0, kd, active)) return r;
    const Cam k{K[0], K[4], K[2], K[5]};
    for (int32_t i = 0; i < n; ++i) {
        double pu, pv;
        if (active)
            (void)pnp_reproj_err_dist(n_dist == 8, R, t, k, kd.k, pts3d[3 * i], pts3d[3 * i + 1], pts3d[3 * i + 2], 0.0,
                                      0.0, pu, pv);
        else
            (void)pnp_reproj_err(R, t, k, pts3d[3 * i], pts3d[3 * i + 1], pts3d[3 * i + 2], 0.0, 0.0, pu, pv);
        proj_out[2 * i] = pu;
        proj_out[2 * i + 1] = pv;
    }
    return RSAC_OK;
}

int rsac_pnp_refine(const double *pts3d, const double *pts2d, int32_t n, const double K[9], const uint8_t *mask,
                    double R[9], double t[3], int32_t max_iter) {
    if (n < 3 || !pts3d || !pts2d || !K || !R || !t) return fail(RSAC_EINVAL, "bad arguments");
    std::vector<float> soa((size_t)5 * n);
    for (int32_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) soa[(size_t)k * n + i] = (float)pts3d[3 * i + k];
        soa[(size_t)3 * n + i] = (float)pts2d[2 * i];
        soa[(size_t)4 * n + i] = (float)pts2d[2 * i + 1];
    }
    std::vector<uint8_t> m(n, 1);
    if (mask) memcpy(m.data(), mask, n);
    const double cam[4] = {K[0], K[4], K[2], K[5]};
    const float *b = soa.data();
    return pnp_refine_lm(b, b + n, b + 2 * n, b + 3 * n, b + 4 * n, m.data(), n, cam, R, t, max_iter);
}

int rsac_pnp_epnp(const double *pts3d, const double *pts2d, int32_t n, const double K[9], const uint8_t *mask,
                  double R[9], double t[3]) {
    if (n < 4 || !pts3d || !pts2d || !K || !R || !t) return fail(RSAC_EINVAL, "bad arguments");
    std::vector<float> soa((size_t)5 * n);
    for (int32_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) soa[(size_t)k * n + i] = (float)pts3d[3 * i + k];
        soa[(size_t)3 * n + i] = (float)pts2d[2 * i];
        soa[(size_t)4 * n + i] = (float)pts2d[2 * i + 1];
    }
    std::vector<uint8_t> m(n, 1);
    if (mask) memcpy(m.data(), mask, n);
    const double cam[4] = {K[0], K[4], K[2], K[5]};
    const float *b = soa.data();
    return pnp_epnp_host(b, b + n, b + 2 * n, b + 3 * n, b + 4 * n, m.data(), n, cam, R, t) ? RSAC_OK : RSAC_NO_MODEL;
}

int rsac_pnp_epnp_minimal(const double *pts3d, const double *pts2d, const double K[9], double R[9], double t[3]) {
    if (!pts3d || !pts2d || !K || !R || !t) return fail(RSAC_EINVAL, "bad arguments");
    float X[5], Y[5], Z[5], U[5], V[5];
    for (int i = 0; i < 5; ++i) {
        X[i] = (float)pts3d[3 * i];
        Y[i] = (float)pts3d[3 * i + 1];
        Z[i] = (float)pts3d[3 * i + 2];
        U[i] = (float)pts2d[2 * i];
        V[i] = (float)pts2d[2 * i + 1];
    }
    cvq::epnp5_pose(X, Y, Z, U, V, Cam{K[0], K[4], K[2], K[5]}, R, t);
    return RSAC_OK;
}

int rsac_homography_fit(const double *src, const double *dst, int32_t n, const uint8_t *mask, double H_out[9]) {
    if (n < 4 || !src || !dst || !H_out) return fail(RSAC_ETOOFEW, "need >= 4 correspondences");
    std::vector<float> soa((size_t)4 * n);
    for (int32_t i = 0; i < n; ++i) {
        soa[i] = (float)src[2 * i];
        soa[(size_t)n + i] = (float)src[2 * i + 1];
        soa[(size_t)2 * n + i] = (float)dst[2 * i];
        soa[(size_t)3 * n + i] = (float)dst[2 * i + 1];
    }
    std::vector<uint8_t> m(n, 1);
    if (mask) memcpy(m.data(), mask, n);
    const float *b = soa.data();
    return hom_refine(b, b + n, b + 2 * n, b + 3 * n, m.data(), n, H_out) ? RSAC_OK : RSAC_NO_MODEL;
}

int rsac_homography_fit_device(rsac_ctx *c, const void *src, const void *dst, int32_t n, const uint8_t *mask,
                               uint32_t flags, double H_out[9], void *stream) {
    int r = check_device(c);
    if (r) return r;
    r = check_flags("rsac_homography_fit_device", flags, RSAC_F_DEVICE_IN | RSAC_F_DEVICE_SOA);
    if (r) return r;
    if (n < 4 || !src || !dst || !H_out) return fail(RSAC_ETOOFEW, "need >= 4 correspondences");
    memset(H_out, 0, 9 * sizeof(double));
    hipStream_t s = pick_stream(c, stream);
    Staged st;
    r = stage_points(c, src, dst, 2, nullptr, 1, n, flags, s, st);
    if (r) return r;
    const uint8_t *dmask = nullptr;
    r = fit_mask(c->homfit_mask, mask, n, flags, s, &dmask);
    if (r) return r;
    r = hom_fit_enqueue(c, st, dmask, s);
    if (r) return r;
    HIPCHK(hipStreamSynchronize(s));
    return unpack_fit_records(c->h_homfit.as<double>(), kHomFitRes, 1, H_out, nullptr) ? RSAC_OK : RSAC_NO_MODEL;
}

int rsac_homography_fit_batched_device(rsac_ctx *c, const void *src, const void *dst, const int64_t *offsets,
                                       int32_t n_problems, const uint8_t *masks, uint32_t flags, double *H_out,
                                       int32_t *status_out, void *stream) {
    int r = check_device(c);
    if (r) return r;
    r = check_flags("rsac_homography_fit_batched_device", flags, RSAC_F_DEVICE_IN | RSAC_F_DEVICE_SOA);
    if (r) return r;
    if (n_problems < 1 || !offsets || !H_out) return fail(RSAC_EINVAL, "rsac_homography_fit_batched_device: bad arguments");
    if (offsets[n_problems] > 0 && (!src || !dst))
        return fail(RSAC_EINVAL, "rsac_homography_fit_batched_device: bad arguments");
    hipStream_t s = pick_stream(c, stream);
    Staged st;
    r = stage_points(c, src, dst, 2, offsets, n_problems, 0, flags, s, st);
    if (r) return r;
    for (int p = 0; p < n_problems; ++p)
        if (st.off[p + 1] - st.off[p] > INT32_MAX) return fail(RSAC_EINVAL, "a problem exceeds 2^31 - 1 points");
    r = stage_tables(c, st, nullptr, 1.0, s);  // the offsets on the device
    if (r) return r;
    const uint8_t *dmask = nullptr;
    r = fit_mask(c->homfit_mask, masks, st.total, flags, s, &dmask);
    if (r) return r;
    // one problem takes the offsets too: its points start at 0
    const size_t b = sizeof(double) * kHomFitRes * (size_t)n_problems;
    HIPCHK(c->homfit.ensure(b));
    HIPCHK(c->h_homfit.ensure(b));
    HIPCHK(launch_hom_fit(st.d[0], st.d[1], st.d[2], st.d[3], c->d_off, n_problems, 0, dmask, c->homfit.as<double>(), s));
    HIPCHK(hipMemcpyAsync(c->h_homfit.p, c->homfit.p, b, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const bool any = unpack_fit_records(c->h_homfit.as<double>(), kHomFitRes, n_problems, H_out, status_out);
    return any ? RSAC_OK : RSAC_NO_MODEL;
}

int rsac_homography_local_opt(rsac_ctx *c, const void *src, const void *dst, int32_t n, const double H_in[9],
                              double thr, int32_t max_rounds, uint32_t flags, double H_out[9], int32_t *count_out,
                              int32_t *steps_out, uint8_t *mask_out, void *stream) {
    const bool have_args = n >= 1 && src && dst && H_in && H_out;
    if (int r = local_opt_checks(c, "rsac_homography_local_opt", have_args, thr, max_rounds, flags, mask_out)) return r;
    hipStream_t s = pick_stream(c, stream);
    Staged st;
    if (int r = stage_problems(c, src, dst, nullptr, 1, n, thr, flags, s, st)) return r;
    // k_hom_mask's mask, the fit's record in c->h_homfit; a fit of fewer than 4 masked points has no model
    return local_opt_loop(
        c, st, FitFamily{launch_hom_mask, c->homfit_mask, kHomFitRes, 0}, max_rounds, flags, H_out, count_out, steps_out,
        mask_out, s, [&](int p, double *rec) { model_row(H_in, p, rec); return true; },
        [&](const uint8_t *m, const double *, const uint8_t *, const double **res) -> int {
            if (int e = hom_fit_enqueue(c, st, m, s)) return e;
            HIPCHK(hipStreamSynchronize(s));
            *res = c->h_homfit.as<double>();
            return RSAC_OK;
        });
}

void rsac_rodrigues_v2m(const double r[3], double R[9]) { rodrigues_v2m(r, R); }
void rsac_rodrigues_m2v(const double R[9], double r[3]) { rodrigues_m2v(R, r); }
int rsac_update_num_iters(double p, double ep, int model_points, int max_iters) {
    return update_num_iters(p, ep, model_points, max_iters);
}

int rsac_scan_until_best(rsac_scan_state *st, const int32_t *counts, const int8_t *status, int64_t count, int32_t n,
                         int32_t model_points, double confidence, int32_t *improved) {
    if (!st || count < 0 || n <= 0 || (count > 0 && (!counts || !status)))
        return fail(RSAC_EINVAL, "rsac_scan_until_best: bad arguments");
    ScanState s;
    s.niters = st->niters; s.best = st->best; s.iter = st->iter; s.max_good = st->max_good; s.done = st->done != 0;
    scan_step(s, counts, status, count, n, model_points, confidence, true);
    *st = rsac_scan_state{s.niters, s.best, s.iter, s.max_good, s.done ? 1 : 0};
    if (improved) *improved = s.improved ? 1 : 0;
    return RSAC_OK;
}

int rsac_scan_raise(rsac_scan_state *st, int32_t count, int32_t n, int32_t model_points, double confidence) {
    if (!st || n <= 0) return fail(RSAC_EINVAL, "rsac_scan_raise: bad arguments");
    if (count > st->max_good) {  // as local_opt applies it
        st->max_good = count;
        st->niters = update_num_iters(confidence, (double)(n - count) / n, model_points, (int)st->niters);
        if (st->iter >= st->niters) st->done = 1;
    }
    return RSAC_OK;
}

int rsac_last_costs(rsac_ctx *c, int64_t *costs_out, int32_t n_problems) {
    if (!c || !costs_out || n_problems <= 0) return fail(RSAC_EINVAL, "rsac_last_costs: bad arguments");
    if ((size_t)n_problems != c->last_costs.size())
        return fail(RSAC_EINVAL, "rsac_last_costs: the context's last call was not an RSAC_F_MSAC call of %d problems",
                    n_problems);
    memcpy(costs_out, c->last_costs.data(), sizeof(int64_t) * (size_t)n_problems);
    return RSAC_OK;
}

int rsac_msac_shift(double thresh) { return msac_shift_host((float)(thresh * thresh)); }

int rsac_pnp_cost_host(const double *pts3d, const double *pts2d, int32_t n, const double K[9], const double model[12],
                       double thresh, int32_t *count_out, int64_t *cost_out) {
    if (n < 0 || (n > 0 && (!pts3d || !pts2d)) || !K || !model || !cost_out)
        return fail(RSAC_EINVAL, "rsac_pnp_cost_host: bad arguments");
    if (int r = check_msac_thr("rsac_pnp_cost_host", thresh)) return r;
    const float t2 = (float)(thresh * thresh);
    std::vector<float> soa((size_t)5 * std::max(n, 1));
    for (int32_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) soa[(size_t)k * n + i] = (float)pts3d[3 * i + k];
        soa[(size_t)3 * n + i] = (float)pts2d[2 * i];
        soa[(size_t)4 * n + i] = (float)pts2d[2 * i + 1];
    }
    const double cam[4] = {K[0], K[4], K[2], K[5]};
    const float *b = soa.data();
    *cost_out = pnp_cost_host(b, b + n, b + 2 * n, b + 3 * n, b + 4 * n, n, cam, model, model + 9, t2, count_out);
    return RSAC_OK;
}

// f64 AoS correspondences rounded to f32 SoA (sx, sy, dx, dy; n each), as the staging rounds them
static std::vector<float> hom_soa_f32(const double *src, const double *dst, int32_t n) {
    std::vector<float> soa((size_t)4 * std::max(n, 1));
    for (int32_t i = 0; i < n; ++i) {
        soa[i] = (float)src[2 * i];
        soa[(size_t)n + i] = (float)src[2 * i + 1];
        soa[(size_t)2 * n + i] = (float)dst[2 * i];
        soa[(size_t)3 * n + i] = (float)dst[2 * i + 1];
    }
    return soa;
}

int rsac_hom_cost_host(const double *src, const double *dst, int32_t n, const double H[9], double thresh,
                       int32_t *count_out, int64_t *cost_out) {
    if (n < 0 || (n > 0 && (!src || !dst)) || !H || !cost_out)
        return fail(RSAC_EINVAL, "rsac_hom_cost_host: bad arguments");
    if (int r = check_msac_thr("rsac_hom_cost_host", thresh)) return r;
    const float t2 = (float)(thresh * thresh);
    const std::vector<float> soa = hom_soa_f32(src, dst, n);
    const float *b = soa.data();
    *cost_out = hom_cost_host(b, b + n, b + 2 * n, b + 3 * n, n, H, t2, count_out);
    return RSAC_OK;
}

void rsac_scan_msac_init(rsac_scan_msac_state *st, int32_t max_iters) {
    if (!st) return;
    ScanState s;
    s.reset(max_iters);
    *st = rsac_scan_msac_state{s.niters, s.best, s.iter, s.max_good, 0, -1};
}

int rsac_scan_msac(rsac_scan_msac_state *st, const int32_t *counts, const int64_t *costs, const int8_t *status,
                   int64_t count, int32_t n, int32_t model_points, double confidence) {
    if (!st || count < 0 || n <= 0 || (count > 0 && (!counts || !costs || !status)))
        return fail(RSAC_EINVAL, "rsac_scan_msac: bad arguments");
    ScanState s;
    s.niters = st->niters; s.best = st->best; s.iter = st->iter; s.max_good = st->max_good; s.done = st->done != 0;
    int64_t bc = st->best_cost;
    scan_step_msac(s, bc, counts, costs, status, count, n, model_points, confidence);
    *st = rsac_scan_msac_state{s.niters, s.best, s.iter, s.max_good, s.done ? 1 : 0, bc};
    return RSAC_OK;
}

void rsac_scan_init(rsac_scan_state *st, int32_t max_iters) {
    if (!st) return;
    ScanState s;
    s.reset(max_iters);
    *st = rsac_scan_state{s.niters, s.best, s.iter, s.max_good, 0};
}

int rsac_scan(rsac_scan_state *st, const int32_t *counts, const int8_t *status, int64_t count, int32_t n,
              int32_t model_points, double confidence) {
    if (!st || count < 0 || n <= 0 || (count > 0 && (!counts || !status)))
        return fail(RSAC_EINVAL, "rsac_scan: bad arguments");
    ScanState s;
    s.niters = st->niters; s.best = st->best; s.iter = st->iter; s.max_good = st->max_good; s.done = st->done != 0;
    scan_step(s, counts, status, count, n, model_points, confidence);
    *st = rsac_scan_state{s.niters, s.best, s.iter, s.max_good, s.done ? 1 : 0};
    return RSAC_OK;
}

int rsac_homography_lmeds(rsac_ctx *c, const void *src, const void *dst, int32_t n, int32_t max_iters, double conf,
                          uint64_t seed, uint32_t flags, double H_out[9], uint8_t *mask_out, double *median_out,
                          rsac_stats *stats, void *stream) {
    if (n < 4) return fail(RSAC_ETOOFEW, "findHomography needs >= 4 correspondences (got %d)", n);
    int32_t status = 0, ninl = 0;
    return hom_lmeds_core(c, src, dst, nullptr, 1, n, max_iters, conf, seed, flags, H_out, &status, &ninl, median_out,
                          mask_out, stats, pick_stream(c, stream));
}

int rsac_homography_lmeds_batched(rsac_ctx *c, const void *src, const void *dst, const int64_t *offsets, int32_t P,
                                  int32_t max_iters, double conf, uint64_t seed, uint32_t flags, double *H_out,
                                  int32_t *status_out, int32_t *ninl_out, double *medians_out, uint8_t *mask_out,
                                  void *stream) {
    if (!offsets) return fail(RSAC_EINVAL, "offsets required");
    return hom_lmeds_core(c, src, dst, offsets, P, 0, max_iters, conf, seed, flags, H_out, status_out, ninl_out,
                          medians_out, mask_out, nullptr, pick_stream(c, stream));
}

int rsac_homography_medians(rsac_ctx *c, const void *src, const void *dst, int32_t n, int64_t hyp_begin, int32_t H,
                            uint64_t seed, uint32_t flags, const int32_t *subsets, double *medians_out,
                            int8_t *status_out, double *models_out, void *stream) {
    int r = check_device(c);
    if (r) return r;
    r = check_flags("rsac_homography_medians", flags, RSAC_F_DEVICE_IN | RSAC_F_DEVICE_SOA | RSAC_F_DEVICE_OUT);
    if (r) return r;
    if (H <= 0 || n < 0 || !medians_out || !status_out) return fail(RSAC_EINVAL, "bad arguments");
    hipStream_t s = pick_stream(c, stream);
    Staged st;
    r = stage_points(c, src, dst, 2, nullptr, 1, n, flags, s, st);
    if (r) return r;
    r = stage_tables(c, st, nullptr, 0.0, s);
    if (r) return r;
    r = ensure_hyp_buffers(c, 1, H, subsets != nullptr);
    if (r) return r;
    if (subsets) {
        r = upload_subsets(c, subsets, H, 4, n, s);
        if (r) return r;
    }
    HIPCHK(c->medians.ensure(sizeof(double) * (size_t)H));
    const HomArgs a = hom_args(c, st, seed, hyp_begin, H, subsets != nullptr);
    HIPCHK(launch_hom_solve(a, 1, 0, H, s));
    HIPCHK(launch_hom_median(a, 1, 0, H, c->medians.as<double>(), s));
    const hipMemcpyKind kind = (flags & RSAC_F_DEVICE_OUT) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHK(hipMemcpyAsync(medians_out, c->medians.p, sizeof(double) * H, kind, s));
    HIPCHK(hipMemcpyAsync(status_out, c->status.p, H, kind, s));
    if (models_out) HIPCHK(hipMemcpyAsync(models_out, c->models.p, sizeof(double) * kModelStride * H, kind, s));
    if (!(flags & RSAC_F_DEVICE_OUT)) HIPCHK(hipStreamSynchronize(s));  // device outputs: enqueued, no wait
    return RSAC_OK;
}

int rsac_hom_median_host(const double *src, const double *dst, int32_t n, const double H[9], double *median_out) {
    if (n < 1 || !src || !dst || !H || !median_out) return fail(RSAC_EINVAL, "rsac_hom_median_host: bad arguments");
    const std::vector<float> soa = hom_soa_f32(src, dst, n);
    const float *b = soa.data();
    *median_out = hom_median_host(b, b + n, b + 2 * n, b + 3 * n, n, H);
    return RSAC_OK;
}

int rsac_pnp_lmeds(rsac_ctx *c, const void *pts3d, const void *pts2d, int32_t n, const double K[9], int32_t max_iters,
                   double conf, uint64_t seed, uint32_t flags, double R_out[9], double t_out[3], uint8_t *mask_out,
                   double *median_out, rsac_stats *stats, void *stream) {
    if (n < 4) return fail(RSAC_ETOOFEW, "LMedS PnP needs >= 4 correspondences (got %d)", n);
    if (!c) return fail(RSAC_EINVAL, "null context");
    int32_t status = 0, ninl = 0;
    return with_one_refit_block(c, [&] {
        return pnp_lmeds_core(c, pts3d, pts2d, nullptr, 1, n, K, max_iters, conf, seed, flags, R_out, t_out, &status,
                              &ninl, median_out, mask_out, stats, pick_stream(c, stream));
    });
}

int rsac_pnp_lmeds_batched(rsac_ctx *c, const void *pts3d, const void *pts2d, const int64_t *offsets, int32_t P,
                           const double *K, int32_t max_iters, double conf, uint64_t seed, uint32_t flags,
                           double *R_out, double *t_out, int32_t *status_out, int32_t *ninl_out, double *medians_out,
                           uint8_t *mask_out, void *stream) {
    if (!c) return fail(RSAC_EINVAL, "null context");
    if (!offsets || P <= 0) return fail(RSAC_EINVAL, "offsets and a positive problem count required");
    for (int32_t p = 0; p < P; ++p)
        if (offsets[p + 1] - offsets[p] < 4)
            return fail(RSAC_ETOOFEW, "LMedS PnP needs >= 4 correspondences per problem (problem %d has %lld)", p,
                        (long long)(offsets[p + 1] - offsets[p]));
    return with_one_refit_block(c, [&] {
        return pnp_lmeds_core(c, pts3d, pts2d, offsets, P, 0, K, max_iters, conf, seed, flags, R_out, t_out,
                              status_out, ninl_out, medians_out, mask_out, nullptr, pick_stream(c, stream));
    });
}

int rsac_pnp_medians(rsac_ctx *c, const void *pts3d, const void *pts2d, int32_t n, const double K[9],
                     int64_t hyp_begin, int32_t H, uint64_t seed, uint32_t flags, const int32_t *subsets,
                     double *medians_out, int8_t *status_out, double *models_out, void *stream) {
    int r = check_device(c);
    if (r) return r;
    r = check_flags("rsac_pnp_medians", flags,
                    RSAC_F_MINIMAL_EPNP5 | RSAC_F_RVEC_ROUNDTRIP | RSAC_F_DEVICE_IN | RSAC_F_DEVICE_SOA |
                        RSAC_F_DEVICE_OUT);
    if (r) return r;
    if (H <= 0 || n < 0 || !K || !medians_out || !status_out) return fail(RSAC_EINVAL, "bad arguments");
    if (n < 4) return fail(RSAC_ETOOFEW, "rsac_pnp_medians needs >= 4 correspondences (got %d)", n);
    hipStream_t s = pick_stream(c, stream);
    flags |= RSAC_F_EXACT_ONLY;
    Staged st;
    r = stage_points(c, pts3d, pts2d, 3, nullptr, 1, n, flags, s, st);
    if (r) return r;
    r = stage_tables(c, st, K, 0.0, s);
    if (r) return r;
    r = ensure_hyp_buffers(c, 1, H, subsets != nullptr);
    if (r) return r;
    const int sk = (flags & RSAC_F_MINIMAL_EPNP5) ? 5 : 4;
    if (n < sk) return fail(RSAC_ETOOFEW, "rsac_pnp_medians: %d points, samples of %d", n, sk);
    if (subsets) {
        r = upload_subsets(c, subsets, H, sk, n, s);
        if (r) return r;
    }
    PnpArgs a;
    r = pnp_args(c, st, flags, seed, H, hyp_begin, s, a, nullptr, false, true);
    if (r) return r;
    a.subsets = subsets ? c->subsets.as<int32_t>() : nullptr;
    a.sub_status = subsets ? c->substatus.as<int8_t>() : nullptr;
    r = ensure_epnp5(c, a, 1, H);
    if (r) return r;
    HIPCHK(c->medians.ensure(sizeof(double) * (size_t)H));
    HIPCHK(launch_pnp_solve(a, 1, 0, H, s));
    r = pnp_median_launch(c, a, 1, H, s);
    if (r) return r;
    const bool dev_out = (flags & RSAC_F_DEVICE_OUT) != 0;
    const hipMemcpyKind kind = dev_out ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHK(hipMemcpyAsync(medians_out, c->medians.p, sizeof(double) * H, kind, s));
    HIPCHK(hipMemcpyAsync(status_out, c->status.p, H, kind, s));
    if (models_out) HIPCHK(hipMemcpyAsync(models_out, c->models.p, sizeof(double) * kModelStride * H, kind, s));
    if (dev_out) return RSAC_OK;  // device outputs: enqueued, no wait
    HIPCHK(hipStreamSynchronize(s));
    // PnP hypothesis records leave the validity slot to the status byte: filled in for the caller
    if (models_out)
        for (int64_t h = 0; h < H; ++h) models_out[h * kModelStride + kValidSlot] = status_out[h] > 0 ? 1.0 : 0.0;
    return RSAC_OK;
}

int rsac_pnp_median_host(const double *pts3d, const double *pts2d, int32_t n, const double K[9],
                         const double model[12], double *median_out) {
    if (n < 1 || !pts3d || !pts2d || !K || !model || !median_out)
        return fail(RSAC_EINVAL, "rsac_pnp_median_host: bad arguments");
    std::vector<float> soa((size_t)5 * n);
    for (int32_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) soa[(size_t)k * n + i] = (float)pts3d[3 * i + k];
        soa[(size_t)3 * n + i] = (float)pts2d[2 * i];
        soa[(size_t)4 * n + i] = (float)pts2d[2 * i + 1];
    }
    const double cam[4] = {K[0], K[4], K[2], K[5]};
    const float *b = soa.data();
    *median_out = pnp_median_host(b, b + n, b + 2 * n, b + 3 * n, b + 4 * n, n, cam, model, model + 9);
    return RSAC_OK;
}

int rsac_fundamental_lmeds(rsac_ctx *c, const void *pts1, const void *pts2, int32_t n, int32_t max_iters, double conf,
                           uint64_t seed, uint32_t flags, double F_out[9], uint8_t *mask_out, double *median_out,
                           rsac_stats *stats, void *stream) {
    return fm_lmeds_core(c, pts1, pts2, nullptr, 1, n, max_iters, conf, seed, flags, F_out, nullptr, nullptr,
                         median_out, mask_out, stats, pick_stream(c, stream));
}

int rsac_fundamental_lmeds_batched(rsac_ctx *c, const void *pts1, const void *pts2, const int64_t *offsets, int32_t P,
                                   int32_t max_iters, double conf, uint64_t seed, uint32_t flags, double *F_out,
                                   int32_t *status_out, int32_t *ninl_out, double *medians_out, uint8_t *mask_out,
                                   void *stream) {
    if (int r = check_device(c)) return r;
    if (!offsets) return fail(RSAC_EINVAL, "rsac_fundamental_lmeds_batched: offsets required");
    return fm_lmeds_core(c, pts1, pts2, offsets, P, 0, max_iters, conf, seed, flags, F_out, status_out, ninl_out,
                         medians_out, mask_out, nullptr, pick_stream(c, stream));
}

int rsac_fundamental_medians(rsac_ctx *c, const void *pts1, const void *pts2, int32_t n, int64_t hyp_begin, int32_t H,
                             uint64_t seed, uint32_t flags, double *medians_out, int8_t *status_out,
                             double *models_out, void *stream) {
    int r = check_device(c);
    if (r) return r;
    r = check_flags("rsac_fundamental_medians", flags,
                    RSAC_F_DEVICE_IN | RSAC_F_DEVICE_SOA | RSAC_F_DEVICE_OUT | RSAC_F_FM_7POINT);
    if (r) return r;
    if (H <= 0 || n < 0 || !medians_out || !status_out) return fail(RSAC_EINVAL, "bad arguments");
    // RSAC_F_FM_7POINT: hyp_begin and the caller's H count samples, the outputs hold 3 rows for each
    const int sk = fm_sample_size(flags);
    if ((int64_t)H * records_per_sample(Model::Fm, flags) > INT32_MAX) return fail(RSAC_EINVAL, "too many hypotheses");
    H *= records_per_sample(Model::Fm, flags);
    hipStream_t s = pick_stream(c, stream);
    Staged st;
    r = stage_points(c, pts1, pts2, 2, nullptr, 1, n, flags, s, st);
    if (r) return r;
    r = stage_tables(c, st, nullptr, 0.0, s);
    if (r) return r;
    r = ensure_hyp_buffers(c, 1, H, false);
    if (r) return r;
    HIPCHK(c->medians.ensure(sizeof(double) * (size_t)H));
    const HomArgs a = hom_args(c, st, seed, hyp_begin, H, false);
    HIPCHK(launch_fm_solve(a, 1, 0, H, s, sk));
    HIPCHK(launch_fm_median(a, 1, 0, H, c->medians.as<double>(), s));
    const hipMemcpyKind kind = (flags & RSAC_F_DEVICE_OUT) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHK(hipMemcpyAsync(medians_out, c->medians.p, sizeof(double) * H, kind, s));
    HIPCHK(hipMemcpyAsync(status_out, c->status.p, H, kind, s));
    if (models_out) HIPCHK(hipMemcpyAsync(models_out, c->models.p, sizeof(double) * kModelStride * H, kind, s));
    if (!(flags & RSAC_F_DEVICE_OUT)) HIPCHK(hipStreamSynchronize(s));  // device outputs: enqueued, no wait
    return RSAC_OK;
}

int rsac_fm_err_host(const double *pts1, const double *pts2, int32_t n, const double F[9], float *err_out) {
    if (n < 0 || (n > 0 && (!pts1 || !pts2 || !err_out)) || !F)
        return fail(RSAC_EINVAL, "rsac_fm_err_host: bad arguments");
    const std::vector<float> soa = hom_soa_f32(pts1, pts2, n);
    const float *b = soa.data();
    fm_err_host(b, b + n, b + 2 * n, b + 3 * n, n, F, err_out);
    return RSAC_OK;
}

int rsac_fm_cost_host(const double *pts1, const double *pts2, int32_t n, const double F[9], double thresh,
                      int32_t *count_out, int64_t *cost_out) {
    if (n < 0 || (n > 0 && (!pts1 || !pts2)) || !F || !cost_out)
        return fail(RSAC_EINVAL, "rsac_fm_cost_host: bad arguments");
    if (int r = check_msac_thr("rsac_fm_cost_host", thresh)) return r;
    const float t2 = (float)(thresh * thresh);
    const std::vector<float> soa = hom_soa_f32(pts1, pts2, n);
    const float *b = soa.data();
    *cost_out = fm_cost_host(b, b + n, b + 2 * n, b + 3 * n, n, F, t2, count_out);
    return RSAC_OK;
}

int rsac_fm_median_host(const double *pts1, const double *pts2, int32_t n, const double F[9], double *median_out) {
    if (n < 1 || !pts1 || !pts2 || !F || !median_out) return fail(RSAC_EINVAL, "rsac_fm_median_host: bad arguments");
    const std::vector<float> soa = hom_soa_f32(pts1, pts2, n);
    const float *b = soa.data();
    *median_out = fm_median_host(b, b + n, b + 2 * n, b + 3 * n, n, F);
    return RSAC_OK;
}

int rsac_cubic_real_roots(const double c[4], double roots_out[3]) {
    if (!c || !roots_out) return 0;
    return cubic_real_roots(c, roots_out);
}

int rsac_fm_minimal7(const double *pts1, const double *pts2, double F_out[27], int32_t *n_models) {
    if (!pts1 || !pts2 || !F_out || !n_models) return fail(RSAC_EINVAL, "rsac_fm_minimal7: bad arguments");
    float x1[7], y1[7], x2[7], y2[7];
    for (int i = 0; i < 7; ++i) {
        x1[i] = (float)pts1[2 * i]; y1[i] = (float)pts1[2 * i + 1];
        x2[i] = (float)pts2[2 * i]; y2[i] = (float)pts2[2 * i + 1];
    }
    double F[27];
    const int nm = fm_minimal7(x1, y1, x2, y2, F);
    for (int k = 0; k < 27; ++k) F_out[k] = k < 9 * nm ? F[k] : 0.0;
    *n_models = nm;
    return RSAC_OK;
}

int rsac_fundamental_fit(const double *pts1, const double *pts2, int32_t n, const uint8_t *mask, double F_out[9]) {
    if (n < 0 || (n > 0 && (!pts1 || !pts2)) || !F_out) return fail(RSAC_EINVAL, "rsac_fundamental_fit: bad arguments");
    const std::vector<float> soa = hom_soa_f32(pts1, pts2, n);
    const float *b = soa.data();
    if (fm_fit_host(b, b + n, b + 2 * n, b + 3 * n, mask, n, F_out)) return RSAC_OK;
    memset(F_out, 0, 9 * sizeof(double));
    return RSAC_NO_MODEL;
}

int rsac_fundamental_fit_device(rsac_ctx *c, const void *pts1, const void *pts2, int32_t n, const uint8_t *mask,
                                uint32_t flags, double F_out[9], void *stream) {
    int r = check_device(c);
    if (r) return r;
    r = check_flags("rsac_fundamental_fit_device", flags, RSAC_F_DEVICE_IN | RSAC_F_DEVICE_SOA);
    if (r) return r;
    if (n < 0 || (n > 0 && (!pts1 || !pts2)) || !F_out)
        return fail(RSAC_EINVAL, "rsac_fundamental_fit_device: bad arguments");
    memset(F_out, 0, 9 * sizeof(double));
    if (n < 8) return RSAC_NO_MODEL;
    hipStream_t s = pick_stream(c, stream);
    Staged st;
    r = stage_points(c, pts1, pts2, 2, nullptr, 1, n, flags, s, st);
    if (r) return r;
    const uint8_t *dmask = nullptr;
    r = fit_mask(c->fmfit_mask, mask, n, flags, s, &dmask);
    if (r) return r;
    double res[kFmFitRes];
    r = fm_fit_enqueue(c, st, dmask, res, s);
    if (r) return r;
    HIPCHK(hipStreamSynchronize(s));
    return unpack_fit_records(res, kFmFitRes, 1, F_out, nullptr) ? RSAC_OK : RSAC_NO_MODEL;
}

int rsac_fundamental_local_opt(rsac_ctx *c, const void *pts1, const void *pts2, int32_t n, const double F_in[9],
                               double thr, int32_t max_rounds, uint32_t flags, double F_out[9], int32_t *count_out,
                               int32_t *steps_out, uint8_t *mask_out, void *stream) {
    const bool have_args = n >= 1 && pts1 && pts2 && F_in && F_out;
    if (int r = local_opt_checks(c, "rsac_fundamental_local_opt", have_args, thr, max_rounds, flags, mask_out)) return r;
    hipStream_t s = pick_stream(c, stream);
    Staged st;
    if (int r = stage_problems(c, pts1, pts2, nullptr, 1, n, thr, flags, s, st)) return r;
    // k_fm_mask's mask (the count rule), the single fit's record straight to rec; a fit of fewer than 8
    // masked points has no model
    double rec[kFmFitRes];
    return local_opt_loop(
        c, st, FitFamily{launch_fm_mask, c->fmfit_mask, kFmFitRes, 0}, max_rounds, flags, F_out, count_out, steps_out,
        mask_out, s, [&](int p, double *r0) { model_row(F_in, p, r0); return true; },
        [&](const uint8_t *m, const double *, const uint8_t *, const double **res) -> int {
            if (int e = fm_fit_enqueue(c, st, m, rec, s)) return e;
            HIPCHK(hipStreamSynchronize(s));
            *res = rec;
            return RSAC_OK;
        });
}

int rsac_fundamental_ransac_batched(rsac_ctx *c, const void *pts1, const void *pts2, const int64_t *offsets,
                                    int32_t n_problems, int32_t max_iters, double thr, double conf, uint64_t seed,
                                    uint32_t flags, double *F_out, int32_t *status_out, int32_t *n_inliers_out,
                                    uint8_t *mask_out, void *stream) {
    if (int r = check_device(c)) return r;
    if (int r = reject_em5("rsac_fundamental_ransac_batched", flags)) return r;
    return fm_batched_core(c, pts1, pts2, offsets, n_problems, max_iters, thr, conf, seed, flags, F_out, status_out,
                           n_inliers_out, mask_out, pick_stream(c, stream));
}

// the staging both batched fit entry points share: points, offsets, the range plan
static int fm_batch_stage(rsac_ctx *c, const char *what, const void *pts1, const void *pts2, const int64_t *offsets,
                          int32_t P, double thr, uint32_t flags, hipStream_t s, Staged &st, FmFitBatch &fb) {
    if (int r = batch_checks(what, pts1, pts2, offsets, P, false)) return r;  // (the point limit: the plan's)
    if (int r = stage_problems(c, pts1, pts2, offsets, P, 0, thr, flags, s, st)) return r;
    return fm_fit_batch_plan(c, st, s, fb);
}

int rsac_fundamental_fit_batched_device(rsac_ctx *c, const void *pts1, const void *pts2, const int64_t *offsets,
                                        int32_t n_problems, const uint8_t *masks, uint32_t flags, double *F_out,
                                        int32_t *status_out, void *stream) {
    const char *what = "rsac_fundamental_fit_batched_device";
    int r = check_device(c);
    if (r) return r;
    r = check_flags(what, flags, RSAC_F_DEVICE_IN | RSAC_F_DEVICE_SOA);
    if (r) return r;
    if (!F_out) return fail(RSAC_EINVAL, "%s: bad arguments", what);
    hipStream_t s = pick_stream(c, stream);
    Staged st;
    FmFitBatch fb;
    r = fm_batch_stage(c, what, pts1, pts2, offsets, n_problems, 1.0, flags, s, st, fb);
    if (r) return r;
    const uint8_t *dmask = nullptr;
    r = fit_mask(c->fmfit_mask, masks, st.total, flags, s, &dmask);
    if (r) return r;
    r = fm_fit_batch_enqueue(c, st, fb, dmask, s);
    if (r) return r;
    HIPCHK(hipStreamSynchronize(s));
    const bool any = unpack_fit_records(c->h_fmfit.as<double>(), kFmFitRes, n_problems, F_out, status_out);
    return any ? RSAC_OK : RSAC_NO_MODEL;
}

int rsac_fundamental_local_opt_batched(rsac_ctx *c, const void *pts1, const void *pts2, const int64_t *offsets,
                                       int32_t n_problems, const double *F_in, double thr, int32_t max_rounds,
                                       uint32_t flags, double *F_out, int32_t *counts_out, int32_t *steps_out,
                                       uint8_t *mask_out, void *stream) {
    const char *what = "rsac_fundamental_local_opt_batched";
    const int P = n_problems;
    int r = local_opt_checks(c, what, F_in && F_out, thr, max_rounds, flags, mask_out);
    if (r) return r;
    hipStream_t s = pick_stream(c, stream);
    Staged st;
    FmFitBatch fb;
    r = fm_batch_stage(c, what, pts1, pts2, offsets, P, thr, flags, s, st, fb);
    if (r) return r;
    // k_fm_mask's masks, the batched fit (whose pass 1 counts each mask; a problem out of the round has a
    // zero mask, and the fit's blocks read the mask bytes alone), the records in c->h_fmfit
    return local_opt_loop(
        c, st, FitFamily{launch_fm_mask, c->fmfit_mask, kFmFitRes, 0}, max_rounds, flags, F_out, counts_out, steps_out,
        mask_out, s, [&](int p, double *rec) { return model_row(F_in, p, rec); },
        [&](const uint8_t *m, const double *, const uint8_t *, const double **res) -> int {
            if (int e = fm_fit_batch_enqueue(c, st, fb, m, s)) return e;
            HIPCHK(hipStreamSynchronize(s));
            *res = c->h_fmfit.as<double>();
            return RSAC_OK;
        });
}

double rsac_lmeds_sigma(double median, int32_t n, int32_t model_points) { return lmeds_sigma(median, n, model_points); }

int rsac_lmeds_num_iters(double confidence, int32_t model_points, int32_t max_iters) {
    return lmeds_num_iters(confidence, model_points, max_iters);
}

void rsac_scan_lmeds_init(rsac_scan_lmeds_state *st, int64_t n_iters) {
    if (!st) return;
    LmedsScan s;
    s.reset(n_iters);
    *st = rsac_scan_lmeds_state{s.niters, s.best, s.iter, 0, s.best_median};
}

int rsac_scan_lmeds(rsac_scan_lmeds_state *st, const int8_t *status, const double *medians, int64_t count) {
    if (!st || count < 0 || (count > 0 && (!status || !medians)))
        return fail(RSAC_EINVAL, "rsac_scan_lmeds: bad arguments");
    LmedsScan s;
    s.niters = st->niters; s.best = st->best; s.iter = st->iter; s.done = st->done != 0;
    s.best_median = st->best_median;
    scan_step_lmeds(s, status, medians, count);
    *st = rsac_scan_lmeds_state{s.niters, s.best, s.iter, s.done ? 1 : 0, s.best_median};
    return RSAC_OK;
}

// ---------------------------------------------------------------------------
// Essential matrix: calibrated refit and local optimisation
// ---------------------------------------------------------------------------
// Kinv1, Kinv2 of P problems (K2s null: K1s for both views) by em5_kinv -> kinv (18 P doubles)
static int em_fit_kinv(const char *what, const double *K1s, const double *K2s, int32_t P, std::vector<double> &kinv) {
    if (!K1s) return fail(RSAC_EINVAL, "%s: K1 required", what);
    kinv.resize((size_t)18 * P);
    for (int p = 0; p < P; ++p) {
        const double *K1 = K1s + 9 * (size_t)p, *K2 = K2s ? K2s + 9 * (size_t)p : K1;
        if (!em5_kinv(K1, kinv.data() + 18 * (size_t)p) || !em5_kinv(K2, kinv.data() + 18 * (size_t)p + 9))
            return fail(RSAC_EINVAL, "%s: singular or non-finite intrinsics (problem %d)", what, p);
    }
    return RSAC_OK;
}

// The batched refit (launch_em_refine) of the staged problems.  em_fit_plan lays c->emfit out as the
// inverse intrinsics, the start models, the result records and the `on` bytes, and uploads the
// intrinsics (once per call: every round of a local optimisation reuses them).  em_fit_enqueue
// uploads the start models (and `on`, NULL = every problem), refits over the device masks dmask
// (concatenated, NULL = all) and copies the records (kEmFitRes doubles per problem) to c->h_emfit --
// the caller synchronises before reading them.  Both after stage_tables (the offsets).  The uploads
// are from pageable memory, complete on return.
struct EmFitBatch {
    double *kinv = nullptr, *E = nullptr, *res = nullptr;
    uint8_t *on = nullptr;
};

static int em_fit_plan(rsac_ctx *c, int32_t P, const std::vector<double> &kinv, hipStream_t s, EmFitBatch &eb) {
    const size_t d = (size_t)(18 + 9 + kEmFitRes) * P;
    HIPCHK(c->emfit.ensure(sizeof(double) * d + (size_t)P));
    HIPCHK(c->h_emfit.ensure(sizeof(double) * kEmFitRes * (size_t)P));
    eb.kinv = c->emfit.as<double>();
    eb.E = eb.kinv + (size_t)18 * P;
    eb.res = eb.E + (size_t)9 * P;
    eb.on = (uint8_t *)(eb.res + (size_t)kEmFitRes * P);
    HIPCHK(hipMemcpyAsync(eb.kinv, kinv.data(), sizeof(double) * 18 * (size_t)P, hipMemcpyHostToDevice, s));
    return RSAC_OK;
}

static int em_fit_enqueue(rsac_ctx *c, const Staged &st, const EmFitBatch &eb, const uint8_t *dmask, const double *E_in,
                          const uint8_t *on, hipStream_t s) {
    const int P = st.P;
    HIPCHK(hipMemcpyAsync(eb.E, E_in, sizeof(double) * 9 * (size_t)P, hipMemcpyHostToDevice, s));
    if (on) HIPCHK(hipMemcpyAsync(eb.on, on, (size_t)P, hipMemcpyHostToDevice, s));
    HIPCHK(launch_em_refine(st.d[0], st.d[1], st.d[2], st.d[3], dmask, c->d_off, eb.kinv, eb.E, on ? eb.on : nullptr, P,
                            eb.res, s));
    HIPCHK(hipMemcpyAsync(c->h_emfit.p, eb.res, sizeof(double) * kEmFitRes * (size_t)P, hipMemcpyDeviceToHost, s));
    return RSAC_OK;
}

// one result record -> the caller's optional outputs (zeros without a model; the count always)
static int em_fit_unpack(const double *rec, double *E_out, double *F_out, double *cost_out, int32_t *count_out,
                         int32_t *steps_out) {
    const bool ok = rec[9] != 0.0;
    if (E_out) memcpy(E_out, rec, 9 * sizeof(double));
    if (F_out) memcpy(F_out, rec + 11, 9 * sizeof(double));
    if (cost_out) *cost_out = ok ? rec[20] : 0.0;
    if (count_out) *count_out = (int32_t)rec[10];
    if (steps_out) *steps_out = ok ? (int32_t)rec[21] : 0;
    return ok ? RSAC_OK : RSAC_NO_MODEL;
}

int rsac_essential_to_fundamental(const double E[9], const double K1[9], const double K2[9], double F_out[9]) {
    if (!E || !K1 || !F_out) return fail(RSAC_EINVAL, "rsac_essential_to_fundamental: bad arguments");
    std::vector<double> kinv;
    if (int r = em_fit_kinv("rsac_essential_to_fundamental", K1, K2, 1, kinv)) return r;
    if (!em_fit_F_of_E(E, kinv.data(), kinv.data() + 9, F_out)) {
        memset(F_out, 0, 9 * sizeof(double));
        return RSAC_NO_MODEL;
    }
    return RSAC_OK;
}

int rsac_essential_refine(const double *pts1, const double *pts2, int32_t n, const double K1[9], const double K2[9],
                          const uint8_t *mask, const double E_in[9], double E_out[9], double F_out[9], double *cost_out,
                          int32_t *count_out, int32_t *steps_out) {
    if (n < 0 || (n > 0 && (!pts1 || !pts2)) || !E_in || !E_out)
        return fail(RSAC_EINVAL, "rsac_essential_refine: bad arguments");
    std::vector<double> kinv;
    if (int r = em_fit_kinv("rsac_essential_refine", K1, K2, 1, kinv)) return r;
    const std::vector<float> soa = hom_soa_f32(pts1, pts2, n);
    const float *b = soa.data();
    double rec[kEmFitRes];
    em_refine_host(b, b + n, b + 2 * (size_t)n, b + 3 * (size_t)n, mask, n, kinv.data(), kinv.data() + 9, E_in, rec);
    return em_fit_unpack(rec, E_out, F_out, cost_out, count_out, steps_out);
}

int rsac_essential_refine_batched_device(rsac_ctx *c, const void *pts1, const void *pts2, const int64_t *offsets,
                                         int32_t n_problems, const double *K1s, const double *K2s, const uint8_t *masks,
                                         const double *E_in, uint32_t flags, double *E_out, double *F_out,
                                         double *cost_out, int32_t *count_out, int32_t *steps_out, int32_t *status_out,
                                         void *stream) {
    const char *what = "rsac_essential_refine_batched_device";
    const int P = n_problems;
    int r = check_device(c);
    if (r) return r;
    r = check_flags(what, flags, RSAC_F_DEVICE_IN | RSAC_F_DEVICE_SOA);
    if (r) return r;
    if (!E_in || !E_out) return fail(RSAC_EINVAL, "%s: bad arguments", what);
    if ((r = batch_checks(what, pts1, pts2, offsets, P, true))) return r;
    std::vector<double> kinv;
    if ((r = em_fit_kinv(what, K1s, K2s, P, kinv))) return r;
    hipStream_t s = pick_stream(c, stream);
    Staged st;
    r = stage_problems(c, pts1, pts2, offsets, P, 0, 1.0, flags, s, st);
    if (r) return r;
    EmFitBatch eb;
    r = em_fit_plan(c, P, kinv, s, eb);
    if (r) return r;
    const uint8_t *dmask = nullptr;
    r = fit_mask(c->fmfit_mask, masks, st.total, flags, s, &dmask);
    if (r) return r;
    r = em_fit_enqueue(c, st, eb, dmask, E_in, nullptr, s);
    if (r) return r;
    HIPCHK(hipStreamSynchronize(s));
    const double *res = c->h_emfit.as<double>();
    bool any = false;
    for (int p = 0; p < P; ++p) {
        const int code = em_fit_unpack(res + (size_t)kEmFitRes * p, E_out + 9 * (size_t)p, F_out ? F_out + 9 * (size_t)p : nullptr,
                                       cost_out ? cost_out + p : nullptr, count_out ? count_out + p : nullptr,
                                       steps_out ? steps_out + p : nullptr);
        any = any || code == RSAC_OK;
        if (status_out) status_out[p] = code;
    }
    return any ? RSAC_OK : RSAC_NO_MODEL;
}

int rsac_essential_refine_device(rsac_ctx *c, const void *pts1, const void *pts2, int32_t n, const double K1[9],
                                 const double K2[9], const uint8_t *mask, const double E_in[9], uint32_t flags,
                                 double E_out[9], double F_out[9], double *cost_out, int32_t *count_out,
                                 int32_t *steps_out, void *stream) {
    if (n < 0 || (n > 0 && (!pts1 || !pts2)) || !E_in || !E_out)
        return fail(RSAC_EINVAL, "rsac_essential_refine_device: bad arguments");
    const int64_t off[2] = {0, n};
    return rsac_essential_refine_batched_device(c, pts1, pts2, off, 1, K1, K2, mask, E_in, flags, E_out, F_out, cost_out,
                                                count_out, steps_out, nullptr, stream);
}

// The local optimisation with the calibrated refit in place of the fit: a problem's model is (E,
// F = Kinv2^T E Kinv1 at unit norm), one record; the count rule's mask (k_fm_mask) is F's, the refit
// starts from E on that mask and its record carries the mask's count and the next round's (E, F).
// A stopped problem's `on` byte is zero and its block leaves at once.
int rsac_essential_local_opt_batched(rsac_ctx *c, const void *pts1, const void *pts2, const int64_t *offsets,
                                     int32_t n_problems, const double *K1s, const double *K2s, const double *E_in,
                                     double thr, int32_t max_rounds, uint32_t flags, double *E_out, int32_t *counts_out,
                                     int32_t *steps_out, uint8_t *mask_out, void *stream) {
    const char *what = "rsac_essential_local_opt_batched";
    const int P = n_problems;
    int r = local_opt_checks(c, what, E_in && E_out, thr, max_rounds, flags, mask_out);
    if (r) return r;
    if ((r = batch_checks(what, pts1, pts2, offsets, P, true))) return r;
    std::vector<double> kinv;
    if ((r = em_fit_kinv(what, K1s, K2s, P, kinv))) return r;
    hipStream_t s = pick_stream(c, stream);
    Staged st;
    r = stage_problems(c, pts1, pts2, offsets, P, 0, thr, flags, s, st);
    if (r) return r;
    EmFitBatch eb;
    r = em_fit_plan(c, P, kinv, s, eb);
    if (r) return r;
    std::vector<double> E((size_t)9 * P);
    return local_opt_loop(
        c, st, FitFamily{launch_fm_mask, c->fmfit_mask, kEmFitRes, 11}, max_rounds, flags, E_out, counts_out, steps_out,
        mask_out, s,
        [&](int p, double *rec) {  // a row the refit cannot start from (zero, non-finite, rank < 2): no model, zeros
            EmFitPose pose;
            const double *Ep = E_in + 9 * (size_t)p, *kp = kinv.data() + 18 * (size_t)p;
            const bool ok = em_fit_start(Ep, pose) && em_fit_F_of_E(Ep, kp, kp + 9, rec + 11);
            if (ok) memcpy(rec, Ep, 9 * sizeof(double));
            else memset(rec + 11, 0, 9 * sizeof(double));
            return ok;
        },
        [&](const uint8_t *m, const double *recs, const uint8_t *on, const double **res) -> int {
            for (int p = 0; p < P; ++p) memcpy(&E[9 * (size_t)p], recs + (size_t)kEmFitRes * p, 9 * sizeof(double));
            if (int e = em_fit_enqueue(c, st, eb, m, E.data(), on, s)) return e;
            HIPCHK(hipStreamSynchronize(s));
            *res = c->h_emfit.as<double>();
            return RSAC_OK;
        });
}

int rsac_essential_local_opt(rsac_ctx *c, const void *pts1, const void *pts2, int32_t n, const double K1[9],
                             const double K2[9], const double E_in[9], double thr, int32_t max_rounds, uint32_t flags,
                             double E_out[9], int32_t *count_out, int32_t *steps_out, uint8_t *mask_out, void *stream) {
    if (n < 1 || !pts1 || !pts2 || !E_in || !E_out) return fail(RSAC_EINVAL, "rsac_essential_local_opt: bad arguments");
    const int64_t off[2] = {0, n};
    return rsac_essential_local_opt_batched(c, pts1, pts2, off, 1, K1, K2, E_in, thr, max_rounds, flags, E_out, count_out,
                                            steps_out, mask_out, stream);
}

}  // extern "C"
