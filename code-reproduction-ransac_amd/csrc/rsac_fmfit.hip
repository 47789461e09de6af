// rsac_fmfit.hip -- the batched least-squares fundamental matrix on the device (k_fm_fit_sums_b,
// k_fm_fit_finish_b; DESIGN.md "Batched fundamental matrix").  A source file of its own, as
// rsac_homfit.hip is, so its code object stands beside rsac_kernels.hip's and leaves that one's
// kernels where they were: the headline kernels and the one-problem fit keep their code, their
// registers and their addresses.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rsac_internal.h"
#include "rsac_math.h"

namespace rsac {

// ---------------------------------------------------------------------------
// The twins of k_fm_fit_sums<PASS> and k_fm_fit_finish (rsac_kernels.hip) with a problem per grid
// row; the summation order is fm_fit's (rsac_math.h), defined over point indices within the
// problem.  Block (r, p) of k_fm_fit_sums_b sums range r of problem p -- points offsets[p] ..
// offsets[p + 1]; thread t is slot t and takes the problem's points r * 4096 + t + 512 j, j = 0 .. 7,
// in that order; the 64-lane tree per wave, the 8 wave sums left to right through LDS -- into row
// rbase[p] + r, rbase[p] being the ranges of the problems before p.  A block past its problem's last
// range leaves before any barrier.  Pass 2's blocks each re-add their own problem's
// fm_fit_ranges(n_p) rows of pass 1 left to right for the centroids.  k_fm_fit_finish_b: one wave per
// problem adds that problem's rows left to right, one lane runs the solve with the 9 x 9 arrays in
// LDS.  Every operation a problem sees is the one-problem kernels' in their order: the same bits.
// Kernel boundaries are the only ordering between blocks: no atomics, no waits.
// ---------------------------------------------------------------------------
template <int PASS>
__global__ __launch_bounds__(kLmThreads) void k_fm_fit_sums_b(const float *__restrict__ X1, const float *__restrict__ Y1,
                                                              const float *__restrict__ X2, const float *__restrict__ Y2,
                                                              const uint8_t *__restrict__ mask,
                                                              const int64_t *__restrict__ offsets,
                                                              const int32_t *__restrict__ rbase,
                                                              const double *__restrict__ rows1, double *__restrict__ rows) {
    constexpr int NV = PASS == 1 ? kFmFitS1 : kFmFitS2;
    constexpr int PER = kFmFitRange / kLmThreads;
    __shared__ double wsum[kLmThreads / 64][NV];
    __shared__ double tot1[kFmFitS1];
    const int prob = blockIdx.y;
    const int64_t p0 = offsets[prob];
    const int n = (int)(offsets[prob + 1] - p0);
    const int nr = fm_fit_ranges(n);
    if ((int)blockIdx.x >= nr) return;  // block-uniform, before any barrier
    const size_t row0 = (size_t)rbase[prob];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double cen[4] = {0.0, 0.0, 0.0, 0.0};
    bool live = true;
    if (PASS == 2) {
        if (tid < kFmFitS1) {
            const double *r1 = rows1 + row0 * kFmFitS1;
            double t = r1[tid];
            for (int r = 1; r < nr; ++r) t = t + r1[r * kFmFitS1 + tid];
            tot1[tid] = t;
        }
        __syncthreads();
        live = fm_fit_centroids(tot1, cen);  // block-uniform; fewer than 8 points: the finish reports no model
    }
    double a[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) a[q] = 0.0;
    const int64_t base = (int64_t)blockIdx.x * kFmFitRange + tid;  // within the problem
    float x1[PER], y1[PER], x2[PER], y2[PER];
    bool on[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int64_t i = base + (int64_t)j * kLmThreads;
        const int64_t q = p0 + i;  // read only where i < n
        on[j] = live && i < n && (!mask || mask[q]);
        x1[j] = on[j] ? X1[q] : 0.f;
        y1[j] = on[j] ? Y1[q] : 0.f;
        x2[j] = on[j] ? X2[q] : 0.f;
        y2[j] = on[j] ? Y2[q] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < PER; ++j)
        if (on[j]) {
            if (PASS == 1)
                fm_fit_acc1((double)x1[j], (double)y1[j], (double)x2[j], (double)y2[j], a);
            else
                fm_fit_acc2((double)x1[j], (double)y1[j], (double)x2[j], (double)y2[j], cen[0], cen[1], cen[2],
                            cen[3], a);
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
        rows[(row0 + blockIdx.x) * NV + tid] = t;
    }
}

// jacobi_eig<9> (rsac_math.h) by one wave, A, V, d in LDS: rsac_kernels.hip's jacobi_eig9_wave, copied
// so that file stays as it was.  The three element loops of a rotation run on lanes 0 .. 8 (lane k
// takes index k; V's columns go with A's), every lane forms the sweep test and the rotation from the
// same LDS values, so all branches are wave-uniform.  Each element sees the host loop's operations
// in the host loop's order: the same bits.  Barriers: after the parameters are read, between the
// column and the row phase (lane q reads what lane p wrote), and after the row phase.
static __device__ void fm_jacobi_eig9_wave(double *A, double *V, double *d, int lane) {
    constexpr int N = 9;
    for (int i = lane; i < N * N; i += 64) V[i] = (i / N == i % N) ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < N; ++p) {
            diag = diag + A[p * N + p] * A[p * N + p];
            for (int q = p + 1; q < N; ++q) off = off + A[p * N + q] * A[p * N + q];
        }
        if (!(off > 1e-32 * diag)) break;
        for (int p = 0; p < N - 1; ++p)
            for (int q = p + 1; q < N; ++q) {
                double c, sn;
                const bool rot = jrr_rotation(sweep, A[p * N + p], A[q * N + q], A[p * N + q], c, sn);
                __syncthreads();
                if (!rot) continue;
                const int k = lane;
                if (k < N) {
                    const double akp = A[k * N + p], akq = A[k * N + q];
                    A[k * N + p] = jrr_lo(c, sn, akp, akq);
                    A[k * N + q] = jrr_hi(c, sn, akp, akq);
                    const double vkp = V[k * N + p], vkq = V[k * N + q];
                    V[k * N + p] = jrr_lo(c, sn, vkp, vkq);
                    V[k * N + q] = jrr_hi(c, sn, vkp, vkq);
                }
                __syncthreads();
                if (k < N) {
                    const double apk = A[p * N + k], aqk = A[q * N + k];
                    A[p * N + k] = jrr_lo(c, sn, apk, aqk);
                    A[q * N + k] = jrr_hi(c, sn, apk, aqk);
                }
                __syncthreads();
            }
    }
    if (lane < N) d[lane] = A[lane * N + lane];
    __syncthreads();
}

__global__ __launch_bounds__(64) void k_fm_fit_finish_b(const double *__restrict__ rows1, const double *__restrict__ rows2,
                                                        const int64_t *__restrict__ offsets,
                                                        const int32_t *__restrict__ rbase, double *__restrict__ resall) {
    __shared__ double tot[kFmFitS1 + kFmFitS2];
    __shared__ double A[81], V[81], d[9], F[9], par[8];  // par: the centroids, the scales, ok
    const int prob = blockIdx.x;
    const int nr = fm_fit_ranges((int)(offsets[prob + 1] - offsets[prob]));
    const size_t row0 = (size_t)rbase[prob];
    double *res = resall + (size_t)prob * kFmFitRes;
    const int tid = threadIdx.x;
    if (tid < kFmFitS1 + kFmFitS2) {
        const bool one = tid < kFmFitS1;
        const double *rows = one ? rows1 + row0 * kFmFitS1 + tid : rows2 + row0 * kFmFitS2 + (tid - kFmFitS1);
        const int nv = one ? kFmFitS1 : kFmFitS2;
        double t = rows[0];
        for (int r = 1; r < nr; ++r) t = t + rows[(size_t)r * nv];
        tot[tid] = t;
    }
    __syncthreads();
    if (tid == 0) {
        double sc1 = 0.0, sc2 = 0.0;
        const bool ok = fm_fit_centroids(tot, par) && fm_fit_matrix(tot[0], tot + kFmFitS1, A, sc1, sc2);
        par[4] = sc1;
        par[5] = sc2;
        par[6] = ok ? 1.0 : 0.0;
    }
    __syncthreads();
    bool ok = par[6] != 0.0;  // block-uniform
    if (ok) fm_jacobi_eig9_wave(A, V, d, tid);
    if (tid != 0) return;
    ok = ok && fm_fit_model(V, d, par, par[4], par[5], F);
    for (int k = 0; k < 9; ++k) res[k] = ok ? F[k] : 0.0;
    res[9] = ok ? 1.0 : 0.0;
    res[10] = tot[0];
}

hipError_t launch_fm_fit_batched(const float *x1, const float *y1, const float *x2, const float *y2,
                                 const uint8_t *mask, const int64_t *offsets, const int32_t *rbase, int32_t P,
                                 int32_t max_ranges, int32_t total_ranges, double *scr, double *res, hipStream_t s) {
    double *rows1 = scr, *rows2 = scr + (size_t)total_ranges * kFmFitS1;
    const dim3 g(max_ranges, P);
    hipLaunchKernelGGL(k_fm_fit_sums_b<1>, g, dim3(kLmThreads), 0, s, x1, y1, x2, y2, mask, offsets, rbase, nullptr, rows1);
    hipLaunchKernelGGL(k_fm_fit_sums_b<2>, g, dim3(kLmThreads), 0, s, x1, y1, x2, y2, mask, offsets, rbase, rows1, rows2);
    hipLaunchKernelGGL(k_fm_fit_finish_b, dim3(P), dim3(64), 0, s, rows1, rows2, offsets, rbase, res);
    return hipGetLastError();
}

}  // namespace rsac
