// rsac_em5.hip -- the five-point essential-matrix solve on the device (k_em_solve_g5).
// A source file of its own, as rsac_fm7.hip is, so its code object stands beside
// rsac_kernels.hip's and leaves that one's kernels where they were.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rsac_em5.h"
#include "rsac_fmrec.h"
#include "rsac_internal.h"
#include "rsac_math.h"

namespace rsac {

// the source lane (relative to the group) of rank q among the set bits of m: the q-th set bit, or
// q itself when m has no more than q bits (that lane's value is then unused)
__device__ __forceinline__ int em5_nth_bit(uint32_t m, int q) {
    int cnt = 0, src = q;
#pragma unroll
    for (int b = 0; b < 11; ++b) {
        const bool on = (m >> b) & 1u;
        src = (on && cnt == q) ? b : src;
        cnt += on ? 1 : 0;
    }
    return src;
}

// poly10_level on a group: lane q takes interval q of the np + 1 that the np roots of D_(d-1)
// (root j on lane j) cut from [-B, B]; the roots found move down to the group's first lanes in
// ascending order.  Every lane of the group reaches the shuffles.
template <int D>
__device__ __forceinline__ void poly10_level_g16(const double *cc, double B, int g, int q, double &root, int &np) {
    double dc[D + 1];
    poly10_deriv<D>(cc, dc);
    const double left = __shfl(root, g + (q > 0 ? q - 1 : 0));
    const double lo = q == 0 ? -B : left, hi = q == np ? B : root;
    bool has = false;
    double r = 0.0;
    if (q <= np) {
        const bool nlo = poly_eval<D>(dc, lo) < 0.0, nhi = poly_eval<D>(dc, hi) < 0.0;
        has = nlo != nhi;
        if (has) r = poly_bisect<D>(dc, lo, hi, nlo);
    }
    const uint32_t m = (uint32_t)(__ballot(has) >> g) & 0xFFFFu;
    root = __shfl(r, g + em5_nth_bit(m, q));
    np = __popc(m);
}

// em_minimal5 (rsac_em5.h) on 16 lanes: lane q < 5 holds point q and row q of the 5 x 9 system,
// lanes 5 .. 15 rows of zeros that never take part in the pivot search; after the elimination every
// lane holds X, Y, Z, W.  Lane r < 10 then builds row r of the 10 x 20 constraint matrix in
// registers; a row swap is a lane exchange, the pivot search a group reduction, there are no column
// swaps.  Rows 4 .. 9 are broadcast, every lane forms B(z) and the degree-10 polynomial, the levels
// of poly10_real_roots run with one interval per lane, and lane r finishes root r (em5_model).  The
// same operations in the same order as the host form, so the same bits.
// g: the group's first lane; q = lane - g.  Returns whether lane q (< 10) holds model q in F; false
// on every lane for a degenerate sample.  No runtime-indexed private arrays.
__device__ __forceinline__ bool em_minimal5_g16(float x1, float y1, float x2, float y2, const double *Kinv1,
                                                const double *Kinv2, int g, int q, double *F) {
    const bool row = q < 5;
    double q1[3], q2[3];
    em5_ray(Kinv1, x1, y1, q1);
    em5_ray(Kinv2, x2, y2, q2);
    double A[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) A[3 * a + b] = row ? q2[a] * q1[b] : 0.0;
    double amax = 0.0;
#pragma unroll
    for (int j = 0; j < 9; ++j) amax = dabs(A[j]) > amax ? dabs(A[j]) : amax;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        const double w = __shfl_xor(amax, o);
        amax = w > amax ? w : amax;
    }
    int perm[9] = {0, 1, 2, 3, 4, 5, 6, 7, 8};
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        // pivot: the first maximum of |A[i][j]|, r <= i < 5, j >= r, in row-major order
        const bool in = row && q >= r;
        double best = in ? -1.0 : -2.0;
        int pc = r;
#pragma unroll
        for (int j = r; j < 9; ++j)
            if (in && dabs(A[j]) > best) { best = dabs(A[j]); pc = j; }
        int pr = q;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
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
    // N[t][perm[r]] = -A[r][5 + t] / A[r][r], N[t][perm[5 + u]] = (t == u)
    double arr = A[0];
#pragma unroll
    for (int j = 1; j < 5; ++j) arr = q == j ? A[j] : arr;
    double val[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) val[t] = -A[5 + t] / arr;
    double N[4][9];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int k = 0; k < 9; ++k) N[t][k] = perm[5 + t] == k ? 1.0 : 0.0;
#pragma unroll
    for (int r = 0; r < 5; ++r)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const double f = __shfl(val[t], g + r);
#pragma unroll
            for (int k = 0; k < 9; ++k) N[t][k] = perm[r] == k ? f : N[t][k];
        }
    // the 10 x 20 constraint matrix, row q on lane q (lanes 10 .. 15 hold a copy of row 0 that
    // never takes part in the pivot search)
    const bool crow = q < 10;
    double M[20];
    em5_row(N, crow ? q : 0, M);
#pragma unroll
    for (int c = 0; c < 10; ++c) {
        const bool in = crow && q >= c;
        double best = in ? dabs(M[c]) : -2.0;
        if (in && !(best > -1.0)) best = -1.0;  // a NaN entry never wins, as on the host
        int pr = q;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const double ob = __shfl_xor(best, o);
            const int opr = __shfl_xor(pr, o);
            if (ob > best || (ob == best && opr < pr)) { best = ob; pr = opr; }
        }
        if (!(best > 0.0)) return false;
        if (pr != c) {
            const int src = g + (q == c ? pr : q == pr ? c : q);
#pragma unroll
            for (int j = 0; j < 20; ++j) M[j] = __shfl(M[j], src);
        }
        double prow[20];
#pragma unroll
        for (int j = c; j < 20; ++j) prow[j] = __shfl(M[j], g + c);
        const double ip = 1.0 / prow[c];
        if (q != c) {
            const double f = M[c] * ip;
            if (f != 0.0) {
#pragma unroll
                for (int j = c; j < 20; ++j) M[j] = M[j] - f * prow[j];
            }
        }
    }
    double diag = M[0];
#pragma unroll
    for (int j = 1; j < 10; ++j) diag = q == j ? M[j] : diag;
    double T[6][10];
#pragma unroll
    for (int j = 0; j < 10; ++j) {
        const double tj = M[10 + j] / diag;
#pragma unroll
        for (int t = 0; t < 6; ++t) T[t][j] = __shfl(tj, g + 4 + t);
    }
    double B[3][3][5], c[11];
    em5_poly(T, B, c);
    double cc[11], bound;
    const int deg = poly10_plan(c, cc, bound);
    double root = 0.0;
    int nr = 0;
    // group-uniform (every lane holds the same polynomial): a polynomial without roots skips the levels
    if (deg >= 1) {
        poly10_level_g16<1>(cc, bound, g, q, root, nr);
        poly10_level_g16<2>(cc, bound, g, q, root, nr);
        poly10_level_g16<3>(cc, bound, g, q, root, nr);
        poly10_level_g16<4>(cc, bound, g, q, root, nr);
        poly10_level_g16<5>(cc, bound, g, q, root, nr);
        poly10_level_g16<6>(cc, bound, g, q, root, nr);
        poly10_level_g16<7>(cc, bound, g, q, root, nr);
        poly10_level_g16<8>(cc, bound, g, q, root, nr);
        poly10_level_g16<9>(cc, bound, g, q, root, nr);
        poly10_level_g16<10>(cc, bound, g, q, root, nr);
    }
    // the intrinsics are read again here (the pointers pass through an empty asm, so the loads are
    // not merged with those of the rays): 36 wave-uniform registers need not live across the solve
    asm volatile("" : "+s"(Kinv1), "+s"(Kinv2));
    bool ok = false;
    if (q < nr) ok = em5_model(N, B, root, Kinv1, Kinv2, F, nullptr);
    // the surviving models in root order on lanes 0 .. total - 1 (a dropped root closes the gap)
    const uint32_t m = (uint32_t)(__ballot(ok) >> g) & 0xFFFFu;
    const int src = g + em5_nth_bit(m, q);
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = __shfl(F[k], src);
    return q < __popc(m);
}

// 16 lanes per sample (em_minimal5_g16), 16 samples per 256-thread block; lanes 0 .. 9 of a group
// write the sample's ten records (model, status and, where a.fmodels is set, the f32 pre-filter
// record).  samp_begin, S: the launch's first sample and sample count, relative to the record
// buffers; the Philox counter is a.rng_base + sample.  kinv: 18 doubles per problem, Kinv1 then
// Kinv2 (row-major).
__global__ __launch_bounds__(256) void k_em_solve_g5(HomArgs a, const double *__restrict__ kinv, int64_t samp_begin,
                                                     int32_t S) {
    const int prob = blockIdx.y;
    const int lane = threadIdx.x & 63, q = lane & 15, g = lane & ~15;
    const int sl = blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool live = sl < S;  // group-uniform; dead groups still reach every shuffle
    const int64_t sg = samp_begin + (live ? sl : 0);
    const int64_t p0 = a.offsets[prob];
    const int n = (int)(a.offsets[prob + 1] - p0);
    int8_t st = -1;
    double F[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool go = false;
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
    if (n >= 5) {
        Philox rng;
        rng.init(a.seed, 0u, (uint64_t)(a.rng_base + sg));
        int32_t idx[5];
        if (rng.subset<5>(n, idx) == 0) {
            int my = idx[0];  // lanes 5 .. 15 read point idx[0] too; their rows are zeroed
#pragma unroll
            for (int j = 1; j < 5; ++j) my = q == j ? idx[j] : my;
            const int64_t i = p0 + my;
            x1 = a.SX[i]; y1 = a.SY[i]; x2 = a.DX[i]; y2 = a.DY[i];
            go = true;
        }
    }
    if (go) {  // group-uniform (the subset is the group's)
        const double *K1 = kinv + (size_t)prob * 18, *K2 = K1 + 9;
        st = em_minimal5_g16(x1, y1, x2, y2, K1, K2, g, q, F) ? 1 : 0;
        if (st == 0)
#pragma unroll
            for (int k = 0; k < 9; ++k) F[k] = 0.0;
    }
    if (!live || q >= kEm5Records) return;
    const int64_t rec = (int64_t)prob * a.hyp_stride + kEm5Records * sg + q;
    double *m = a.models + rec * kModelStride;
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = F[k];
    m[kValidSlot] = st > 0 ? 1.0 : 0.0;
    a.status[rec] = st;
    if (a.fmodels) fm_write_record(F, st > 0, a.fbounds, prob, (double)a.thr2[prob], a.fmodels + rec * kFModelStride);
}

hipError_t launch_em_solve_g5(const HomArgs &a, const double *kinv, int32_t P, int64_t hyp_begin, int32_t H,
                              hipStream_t s) {
    if (hyp_begin % kEm5Records != 0 || H % kEm5Records != 0 || H <= 0 || !kinv) return hipErrorInvalidValue;
    const int32_t S = H / kEm5Records;
    hipLaunchKernelGGL(k_em_solve_g5, dim3((S + 15) / 16, P), dim3(256), 0, s, a, kinv, hyp_begin / kEm5Records, S);
    return hipGetLastError();
}

}  // namespace rsac
