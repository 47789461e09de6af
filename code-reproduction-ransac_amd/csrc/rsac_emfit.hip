// rsac_emfit.hip -- the calibrated refit of essential matrices on the device (k_em_refine; DESIGN.md
// §25).  A source file of its own, as rsac_homfit.hip, rsac_fmfit.hip and rsac_em5.hip are, so its
// code object stands beside rsac_kernels.hip's and leaves that one's kernels where they were.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rsac_emfit.h"
#include "rsac_internal.h"
#include "rsac_math.h"

namespace rsac {

// em_refine_host (rsac_emfit.h) with one 512-thread block per problem and the whole LM in one launch.
// Problem p is the points offsets[p] .. offsets[p + 1] and the mask bytes at the same positions
// (NULL = all); kinv: Kinv1 then Kinv2, 18 doubles per problem; E_in: 9 per problem; on (may be
// NULL): a zero byte names a problem that takes no part -- its block leaves at once and writes
// nothing.  res: kEmFitRes doubles per problem.
//
// Thread t is slot t of fm_fit's summation order: per range of 4096 points it adds its masked points
// r * 4096 + t + 512 j, j = 0 .. 7, in that order from +0 into 22 register accumulators, the wave
// runs the 64-lane tree, the 8 wave sums go through LDS and are added left to right, and the range
// sums are added left to right into tot -- the host's additions in the host's order.  Thread 0 runs
// em_fit_begin / em_fit_step / em_fit_finish on the state in LDS and publishes the next pass's
// matrices there.  The pass and range loops have block-uniform trip counts, so every thread reaches
// every barrier and shuffle; a slot past the problem's n neither loads nor adds.  No atomics, no
// waits, nothing shared between blocks.
__global__ __launch_bounds__(kLmThreads) void k_em_refine(const float *__restrict__ X1, const float *__restrict__ Y1,
                                                          const float *__restrict__ X2, const float *__restrict__ Y2,
                                                          const uint8_t *__restrict__ mask,
                                                          const int64_t *__restrict__ offsets,
                                                          const double *__restrict__ kinv, const double *__restrict__ E_in,
                                                          const uint8_t *__restrict__ on, double *__restrict__ res) {
    constexpr int NV = kEmFitSums;
    constexpr int PER = kFmFitRange / kLmThreads;
    __shared__ EmFitState st;
    __shared__ double mats[kEmFitMats];
    __shared__ double wsum[kLmThreads / 64][NV];
    __shared__ double tot[NV];
    __shared__ double kin[18];
    const int prob = blockIdx.x;
    if (on && !on[prob]) return;  // block-uniform, before any barrier
    const int64_t p0 = offsets[prob];
    const int n = (int)(offsets[prob + 1] - p0);
    const int nr = fm_fit_ranges(n);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double *rec = res + (size_t)prob * kEmFitRes;
    if (tid < 18) kin[tid] = kinv[(size_t)18 * prob + tid];
    __syncthreads();
    if (tid == 0) em_fit_begin(st, E_in + (size_t)9 * prob, kin, kin + 9, mats);
    __syncthreads();
    bool ok = st.ok != 0;  // block-uniform
    for (int pass = 0; ok && pass <= kEmFitPasses; ++pass) {
        for (int r = 0; r < nr; ++r) {
            double a[NV];
#pragma unroll
            for (int q = 0; q < NV; ++q) a[q] = 0.0;
            const int64_t base = (int64_t)r * kFmFitRange + tid;  // within the problem
#pragma unroll 1
            for (int j = 0; j < PER; ++j) {
                const int64_t i = base + (int64_t)j * kLmThreads;
                if (i < n) {  // read only where i < n
                    const int64_t q = p0 + i;
                    if (!mask || mask[q]) em_fit_acc((double)X1[q], (double)Y1[q], (double)X2[q], (double)Y2[q], mats, a);
                }
            }
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                double v = a[q];
                for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
                if (lane == 0) wsum[wave][q] = v;
            }
            __syncthreads();
            if (tid < NV) {
                double t = wsum[0][tid];
                for (int w = 1; w < kLmThreads / 64; ++w) t = t + wsum[w][tid];
                tot[tid] = r == 0 ? t : tot[tid] + t;
            }
            __syncthreads();  // tot is whole; wsum may be rewritten
        }
        if (tid == 0) em_fit_step(st, pass, tot, kin, kin + 9, mats);
        __syncthreads();
        ok = st.ok != 0;
    }
    if (tid == 0) em_fit_finish(st, kin, kin + 9, rec);
}

hipError_t launch_em_refine(const float *x1, const float *y1, const float *x2, const float *y2, const uint8_t *mask,
                            const int64_t *offsets, const double *kinv, const double *E_in, const uint8_t *on,
                            int32_t P, double *res, hipStream_t s) {
    hipLaunchKernelGGL(k_em_refine, dim3(P), dim3(kLmThreads), 0, s, x1, y1, x2, y2, mask, offsets, kinv, E_in, on, res);
    return hipGetLastError();
}

}  // namespace rsac
