// rsac_fm7.hip -- the 7-point fundamental-matrix solve on the device (k_fm_solve_g7).
// A source file of its own, as rsac_fmfit.hip is, so its code object stands beside
// rsac_kernels.hip's and leaves that one's kernels where they were.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rsac_fmrec.h"
#include "rsac_internal.h"
#include "rsac_math.h"

namespace rsac {

// fm_minimal7 (rsac_math.h) on 8 lanes, as fm_minimal8_g8 runs fm_minimal8: lane q < 7 holds point q
// and row q of the 7 x 9 system in registers, lane 7 holds a row of zeros that never takes part in
// the pivot search; a row swap is a lane exchange, a column swap selects over the row's 9
// registers, the pivot search is a group reduction.  The same operations in the same order as the
// host form, so the same bits.  After the elimination every lane holds g1, g2 and the cubic; lane
// r < 3 then bisects bracket r of cubic_plan and forms that root's model, and the models that
// survive fm7_model move down to the group's first lanes in root order.
// g: the group's first lane; q = lane - g.  Returns whether lane q (< 3) holds model q in F;
// false on every lane for a degenerate sample.  No runtime-indexed private arrays.
__device__ __forceinline__ bool fm_minimal7_g8(float x1, float y1, float x2, float y2, int g, int q, double *F) {
    const bool row = q < 7;
    // Hartley normalisation of both images (fm_norm7): the sums in point order on every lane
    double c[2][2], sc[2];
#pragma unroll
    for (int im = 0; im < 2; ++im) {
        const float xs = im ? x2 : x1, ys = im ? y2 : y1;
        double cx = 0.0, cy = 0.0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            cx = cx + (double)__shfl(xs, g + k);
            cy = cy + (double)__shfl(ys, g + k);
        }
        cx = cx / 7.0;
        cy = cy / 7.0;
        const double dx = (double)xs - cx, dy = (double)ys - cy;
        const double tq = dsqrt(dx * dx + dy * dy);
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < 7; ++k) d = d + __shfl(tq, g + k);
        d = d / 7.0;
        if (!(d > 1e-300)) return false;
        c[im][0] = cx;
        c[im][1] = cy;
        sc[im] = 1.4142135623730951 / d;
    }
    const double u1 = ((double)x1 - c[0][0]) * sc[0], v1 = ((double)y1 - c[0][1]) * sc[0];
    const double u2 = ((double)x2 - c[1][0]) * sc[1], v2 = ((double)y2 - c[1][1]) * sc[1];
    double A[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.0};
#pragma unroll
    for (int j = 0; j < 9; ++j) A[j] = row ? A[j] : 0.0;
    double amax = 0.0;
#pragma unroll
    for (int j = 0; j < 9; ++j) amax = dabs(A[j]) > amax ? dabs(A[j]) : amax;
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
        const double w = __shfl_xor(amax, o);
        amax = w > amax ? w : amax;
    }
    int perm[9] = {0, 1, 2, 3, 4, 5, 6, 7, 8};
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        // pivot: the first maximum of |A[i][j]|, r <= i < 7, j >= r, in row-major order
        const bool in = row && q >= r;
        double best = in ? -1.0 : -2.0;
        int pc = r;
#pragma unroll
        for (int j = r; j < 9; ++j)
            if (in && dabs(A[j]) > best) { best = dabs(A[j]); pc = j; }
        int pr = q;
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
            const double ob = __shfl_xor(best, o);
            const int opr = __shfl_xor(pr, o), opc = __shfl_xor(pc, o);
            if (ob > best || (ob == best && opr < pr)) { best = ob; pr = opr; pc = opc; }
        }
        if (!(best > 1e-12 * amax)) return false;
        if (pr != r) {  // group-uniform: rows r and pr trade lanes
            const int src = g + (q == r ? pr : q == pr ? r : q);
#pragma unroll
            for (int j = 0; j < 9; ++j) A[j] = __shfl(A[j], src);
        }
        if (pc != r) {
            double apc = A[r];
#pragma unroll
            for (int j = r + 1; j < 9; ++j) apc = j == pc ? A[j] : apc;
            const double ar = A[r];
#pragma unroll
            for (int j = r + 1; j < 9; ++j) A[j] = j == pc ? ar : A[j];
            A[r] = apc;
            int ppc = perm[r];
#pragma unroll
            for (int j = r + 1; j < 9; ++j) ppc = j == pc ? perm[j] : ppc;
            const int pr0 = perm[r];
#pragma unroll
            for (int j = r + 1; j < 9; ++j) perm[j] = j == pc ? pr0 : perm[j];
            perm[r] = ppc;
        }
        double prow[9];
#pragma unroll
        for (int j = r; j < 9; ++j) prow[j] = __shfl(A[j], g + r);
        const double ip = 1.0 / prow[r];
        if (q != r) {
            const double f = A[r] * ip;
            if (f != 0.0) {
#pragma unroll
                for (int j = r; j < 9; ++j) A[j] = A[j] - f * prow[j];
            }
        }
    }
    // g1[perm[r]] = -A[r][7] / A[r][r], g1[perm[7]] = 1, g1[perm[8]] = 0; g2 from column 8 likewise
    double arr = A[0];
#pragma unroll
    for (int j = 1; j < 7; ++j) arr = q == j ? A[j] : arr;
    const double val7 = -A[7] / arr, val8 = -A[8] / arr;
    double g1[9], g2[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        g1[k] = perm[7] == k ? 1.0 : 0.0;
        g2[k] = perm[8] == k ? 1.0 : 0.0;
    }
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        const double f7 = __shfl(val7, g + r), f8 = __shfl(val8, g + r);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            g1[k] = perm[r] == k ? f7 : g1[k];
            g2[k] = perm[r] == k ? f8 : g2[k];
        }
    }
    double cc[4];
    fm7_cubic(g1, g2, cc);
    const CubicPlan p = cubic_plan(cc);
    bool ok = false;
    if (q < p.n) {  // q < 3: this lane's root
        const double lo = q == 0 ? p.lo0 : q == 1 ? p.lo1 : p.lo2;
        const double hi = q == 0 ? p.hi0 : q == 1 ? p.hi1 : p.hi2;
        const bool neg = q == 0 ? p.neg0 : q == 1 ? p.neg1 : p.neg2;
        const double lambda = cubic_bisect(cc, lo, hi, neg);
        ok = fm7_model(g1, g2, lambda, c[0][0], c[0][1], sc[0], c[1][0], c[1][1], sc[1], F);
    }
    // the surviving models in root order on lanes 0 .. total - 1 (a dropped root closes the gap)
    const int ok0 = __shfl((int)ok, g), ok1 = __shfl((int)ok, g + 1), ok2 = __shfl((int)ok, g + 2);
    const int total = ok0 + ok1 + ok2;
    const int first = ok0 ? 0 : ok1 ? 1 : 2;
    const int second = (ok0 && ok1) ? 1 : 2;
    const int src = g + (q == 0 ? first : q == 1 ? second : q == 2 ? 2 : q);
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = __shfl(F[k], src);
    return q < total;
}

// 8 lanes per sample (fm_minimal7_g8), 32 samples per 256-thread block; lanes 0 .. 2 of a group
// write the sample's three records (model, status and, where a.fmodels is set, the f32 pre-filter
// record).  samp_begin, S: the launch's first sample and sample count, relative to the record
// buffers as the 8-point kernel's hyp_begin is; the Philox counter is a.rng_base + sample.
__global__ __launch_bounds__(256) void k_fm_solve_g7(HomArgs a, int64_t samp_begin, int32_t S) {
    const int prob = blockIdx.y;
    const int lane = threadIdx.x & 63, q = lane & 7, g = lane & ~7;
    const int sl = blockIdx.x * 32 + (threadIdx.x >> 3);
    const bool live = sl < S;  // group-uniform; dead groups still reach every shuffle
    const int64_t sg = samp_begin + (live ? sl : 0);
    const int64_t p0 = a.offsets[prob];
    const int n = (int)(a.offsets[prob + 1] - p0);
    int8_t st = -1;
    double F[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool go = false;
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
    if (n >= 7) {
        Philox rng;
        rng.init(a.seed, 0u, (uint64_t)(a.rng_base + sg));
        int32_t idx[7];
        if (rng.subset<7>(n, idx) == 0) {
            int my = idx[0];  // lane 7 reads point idx[0] too; its row is zeroed
#pragma unroll
            for (int j = 1; j < 7; ++j) my = q == j ? idx[j] : my;
            const int64_t i = p0 + my;
            x1 = a.SX[i]; y1 = a.SY[i]; x2 = a.DX[i]; y2 = a.DY[i];
            go = true;
        }
    }
    if (go) {  // group-uniform (the subset is the group's)
        st = fm_minimal7_g8(x1, y1, x2, y2, g, q, F) ? 1 : 0;
        if (st == 0)
#pragma unroll
            for (int k = 0; k < 9; ++k) F[k] = 0.0;
    }
    if (!live || q >= kFm7Records) return;
    const int64_t rec = (int64_t)prob * a.hyp_stride + kFm7Records * sg + q;
    double *m = a.models + rec * kModelStride;
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = F[k];
    m[kValidSlot] = st > 0 ? 1.0 : 0.0;
    a.status[rec] = st;
    if (a.fmodels) fm_write_record(F, st > 0, a.fbounds, prob, (double)a.thr2[prob], a.fmodels + rec * kFModelStride);
}

hipError_t launch_fm_solve_g7(const HomArgs &a, int32_t P, int64_t hyp_begin, int32_t H, hipStream_t s) {
    if (hyp_begin % kFm7Records != 0 || H % kFm7Records != 0 || H <= 0) return hipErrorInvalidValue;
    const int32_t S = H / kFm7Records;
    hipLaunchKernelGGL(k_fm_solve_g7, dim3((S + 31) / 32, P), dim3(256), 0, s, a, hyp_begin / kFm7Records, S);
    return hipGetLastError();
}

}  // namespace rsac
