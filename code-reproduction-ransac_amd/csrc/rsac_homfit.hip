// rsac_homfit.hip -- the homography refit on the device (k_hom_fit).  A source file
// of its own, so its code object stands beside rsac_kernels.hip's and leaves that one's kernels
// where they were: the headline kernels keep their addresses.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rsac_internal.h"
#include "rsac_math.h"

namespace rsac {

// ---------------------------------------------------------------------------
// Homography refit (hom_refine of rsac_host.hip, from the pieces of rsac_math.h), one wave per
// problem.  Every sum is one lane's sequential chain over the masked points in ascending index,
// the host's order: a chunk of 64 consecutive points is staged through LDS (each lane forms one
// point's terms once), then every lane walks the chunk's masked points in index order and adds its
// own term -- the 8 x 8 A = J^T J is exactly the 64 lanes, lane (a, b); v[a], S and max|r| ride
// along in every lane; LtL's 45 upper entries take lanes 0 .. 44; the centroid and deviation sums
// lanes 0 .. 3.  The Jacobi solves keep A and V in LDS and spread a rotation's three element loops
// over lanes; every lane forms the sweep test, the rotation and the LM schedule from the same LDS
// values, so every branch is wave-uniform.  All loops carry the host's bounds (60 sweeps, 10 LM
// iterations); no atomics, no waits, no hand-off between blocks.
// ---------------------------------------------------------------------------
constexpr int kHomStage = 19;  // doubles per staged point (18 used: an odd stride keeps the lanes' reads apart)

// one pass over the problem's points: term(row, i) stages point i's terms (lane = slot), then
// acc(row) runs for the chunk's masked points in index order on every lane -> the masked count
template <class Term, class Acc>
__device__ __forceinline__ int hom_fit_pass(const uint8_t *__restrict__ mask, int n, int lane, double *stage, Term term,
                                            Acc acc) {
    int m = 0;
    for (int64_t base = 0; base < n; base += 64) {
        const int64_t i = base + lane;
        const bool on = i < n && (!mask || mask[i]);
        if (on) term(stage + lane * kHomStage, i);
        unsigned long long bal = __ballot(on);
        m += __popcll(bal);
        __syncthreads();
        for (; bal; bal &= bal - 1) acc(stage + (__ffsll((long long)bal) - 1) * kHomStage);
        __syncthreads();
    }
    return m;
}

// jacobi_sym (rsac_host.hip) by one wave, A (destroyed: the eigenvalues on its diagonal) and V in
// LDS: lane k < N takes index k of the three element loops (V's columns go with A's), each element
// sees the host loop's operations in the host loop's order.  Barriers: after the parameters are
// read, between the column and the row phase (lane q reads what lane p wrote), after the row phase.
template <int N>
__device__ void hom_jacobi_wave(double *A, double *V, int lane) {
    double frob = 0;
    for (int i = 0; i < N * N; ++i) frob += A[i] * A[i];
    for (int i = lane; i < N * N; i += 64) V[i] = (i / N == i % N) ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0;
        for (int i = 0; i < N; ++i)
            for (int j = i + 1; j < N; ++j) off += A[i * N + j] * A[i * N + j];
        if (hom_jacobi_done(off, frob)) break;
        for (int p = 0; p < N; ++p)
            for (int q = p + 1; q < N; ++q) {
                const double apq = A[p * N + q], app = A[p * N + p], aqq = A[q * N + q];
                __syncthreads();
                if (hom_jacobi_skip(apq)) continue;
                double c, s;
                hom_jacobi_rot(app, aqq, apq, c, s);
                const int k = lane;
                if (k < N) {
                    const double akp = A[k * N + p], akq = A[k * N + q];
                    A[k * N + p] = hom_jacobi_lo(c, s, akp, akq);
                    A[k * N + q] = hom_jacobi_hi(c, s, akp, akq);
                    const double vkp = V[k * N + p], vkq = V[k * N + q];
                    V[k * N + p] = hom_jacobi_lo(c, s, vkp, vkq);
                    V[k * N + q] = hom_jacobi_hi(c, s, vkp, vkq);
                }
                __syncthreads();
                if (k < N) {
                    const double apk = A[p * N + k], aqk = A[q * N + k];
                    A[p * N + k] = hom_jacobi_lo(c, s, apk, aqk);
                    A[q * N + k] = hom_jacobi_hi(c, s, apk, aqk);
                }
                __syncthreads();
            }
    }
}

// offsets NULL: one problem of n1 points at index 0.  mask: over the concatenated points, NULL = all.
// res: kHomFitRes doubles per problem (H or zeros, ok, the masked count).
__global__ __launch_bounds__(64) void k_hom_fit(const float *__restrict__ SX, const float *__restrict__ SY,
                                                const float *__restrict__ DX, const float *__restrict__ DY,
                                                const int64_t *__restrict__ offsets, int32_t n1,
                                                const uint8_t *__restrict__ mask, double *__restrict__ res) {
    __shared__ double stage[64 * kHomStage];
    __shared__ double A9[81], V9[81];
    __shared__ double A[64], W[64], V[64];
    __shared__ double x[9], xd[9], v[8], D[8], d[8], par[9];
    const int lane = threadIdx.x, prob = blockIdx.x;
    const int64_t p0 = offsets ? offsets[prob] : 0;
    const int n = offsets ? (int)(offsets[prob + 1] - p0) : n1;
    const float *sx = SX + p0, *sy = SY + p0, *dx = DX + p0, *dy = DY + p0;
    const uint8_t *mk = mask ? mask + p0 : nullptr;
    double *out = res + (size_t)prob * kHomFitRes;

    // the masked centroids: lane 0 .. 3 sums dx, dy, sx, sy
    const int comp = lane & 3;
    double acc = 0;
    auto coords = [&](double *row, int64_t i) {
        row[0] = dx[i]; row[1] = dy[i]; row[2] = sx[i]; row[3] = sy[i];
    };
    const int m = hom_fit_pass(mk, n, lane, stage, coords, [&](const double *row) { acc += row[comp]; });
    if (m < 4) {  // block-uniform: the ballots' count
        if (lane < kHomFitRes) out[lane] = lane == 10 ? (double)m : 0.0;
        return;
    }
    acc /= m;
    if (lane < 4) par[lane] = acc;
    __syncthreads();
    const double cmx = par[0], cmy = par[1], cMx = par[2], cMy = par[3];
    // the mean absolute deviations
    const double cen = acc;
    acc = 0;
    hom_fit_pass(mk, n, lane, stage, coords, [&](const double *row) { acc += fabs(row[comp] - cen); });
    if (lane < 4) par[4 + lane] = acc;
    __syncthreads();
    double smx = par[4], smy = par[5], sMx = par[6], sMy = par[7];
    if (!hom_fit_scales_ok(smx, smy, sMx, sMy)) {
        if (lane < kHomFitRes) out[lane] = lane == 10 ? (double)m : 0.0;
        return;
    }
    smx = m / smx; smy = m / smy; sMx = m / sMx; sMy = m / sMy;
    // LtL's upper triangle: lane e < 45 is entry (lj, lk)
    int lj = 0, lk = 0;
    {
        int e = lane < 45 ? lane : 0;
        for (int j = 0; j < 9; ++j) {
            if (e < 9 - j) {
                lj = j;
                lk = j + e;
                break;
            }
            e -= 9 - j;
        }
    }
    acc = 0;
    hom_fit_pass(
        mk, n, lane, stage,
        [&](double *row, int64_t i) {
            const double px = (dx[i] - cmx) * smx, py = (dy[i] - cmy) * smy;
            const double pX = (sx[i] - cMx) * sMx, pY = (sy[i] - cMy) * sMy;
            hom_fit_lrows(px, py, pX, pY, row, row + 9);
        },
        [&](const double *row) { acc += hom_fit_lterm(row, row + 9, lj, lk); });
    if (lane < 45) {
        A9[lj * 9 + lk] = acc;
        A9[lk * 9 + lj] = acc;
    }
    __syncthreads();
    hom_jacobi_wave<9>(A9, V9, lane);
    if (lane == 0) {
        int mi = 0;
        for (int i = 1; i < 9; ++i)
            if (A9[i * 9 + i] < A9[mi * 9 + mi]) mi = i;
        double hv[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) hv[k] = V9[k * 9 + mi];
        hom_fit_denorm(hv, cmx, cmy, cMx, cMy, smx, smy, sMx, sMy, x);
    }
    __syncthreads();

    // hom_lm: lane (la, lb) carries A[la][lb]; v[la], S and max|r| ride along in every lane
    const int la = lane >> 3, lb = lane & 7;
    double S = 0, rinf = 0;
    auto normal_eqs = [&]() {  // r, J at x -> A, v (LDS), S, rinf
        double h[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = x[k];
        double aA = 0, av = 0, aS = 0, ar = 0;
        hom_fit_pass(
            mk, n, lane, stage,
            [&](double *row, int64_t i) { hom_fit_point(h, sx[i], sy[i], dx[i], dy[i], row[16], row[17], row, row + 8); },
            [&](const double *row) {
                const double rx = row[16], ry = row[17];
                av += row[la] * rx;
                aA += row[la] * row[lb];
                av += row[8 + la] * ry;
                aA += row[8 + la] * row[8 + lb];
                aS += rx * rx;
                aS += ry * ry;
                ar = fmax(ar, fabs(rx));
                ar = fmax(ar, fabs(ry));
            });
        A[lane] = aA;
        if (lb == 0) v[la] = av;
        S = aS;
        rinf = ar;
        __syncthreads();
    };
    auto eig8 = [&](bool damp, double lam) {  // W = A (damp: + lam * diag(D)), decomposed and clipped
        W[lane] = damp && la == lb ? A[lane] + lam * D[la] : A[lane];
        __syncthreads();
        hom_jacobi_wave<8>(W, V, lane);
        if (lane == 0) hom_eig8_clip(W);
        __syncthreads();
    };
    __syncthreads();
    normal_eqs();
    if (lane < 8) D[lane] = A[lane * 8 + lane];
    __syncthreads();
    double lambda = 1, lc = 0.75;
    int iter = 0;
    for (;;) {
        eig8(true, lambda);
        if (lane == 0) {
            hom_eig8_solve(W, V, v, d);
            for (int a = 0; a < 8; ++a) xd[a] = x[a] - d[a];
        }
        __syncthreads();
        double Sd = 0;
        {
            double h[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) h[k] = xd[k];
            hom_fit_pass(
                mk, n, lane, stage,
                [&](double *row, int64_t i) {
                    hom_fit_point(h, sx[i], sy[i], dx[i], dy[i], row[0], row[1], nullptr, nullptr);
                },
                [&](const double *row) {
                    Sd += row[0] * row[0];
                    Sd += row[1] * row[1];
                });
        }
        const double R = hom_lm_gain(A, v, d, S, Sd);
        if (R > 0.75) {
            lambda *= 0.5;
            if (lambda < lc) lambda = 0;
        } else if (R < 0.25) {
            double nu = hom_lm_nu(v, d, S, Sd);
            if (lambda == 0) {
                eig8(false, 0.0);
                if (lane == 0) par[8] = hom_eig8_maxdiag(W, V);
                __syncthreads();
                lambda = lc = 1. / par[8];
                nu *= 0.5;
            }
            lambda *= nu;
        }
        const double dinf = hom_lm_dinf(d);
        __syncthreads();  // A, v and d are read: the accepted step may rewrite A and v
        if (Sd < S) {
            if (lane < 8) x[lane] = xd[lane];
            __syncthreads();
            normal_eqs();
        }
        iter++;
        if (!hom_lm_go_on(iter, kHomLmIters, dinf, rinf)) break;
    }
    if (lane < 8) out[lane] = x[lane];
    if (lane == 8) out[8] = 1.0;
    if (lane == 9) out[9] = 1.0;
    if (lane == 10) out[10] = (double)m;
    if (lane == 11) out[11] = (double)iter;
}

hipError_t launch_hom_fit(const float *sx, const float *sy, const float *dx, const float *dy, const int64_t *offsets,
                          int32_t P, int32_t n1, const uint8_t *mask, double *res, hipStream_t s) {
    if (P < 1) return hipSuccess;
    hipLaunchKernelGGL(k_hom_fit, dim3(P), dim3(64), 0, s, sx, sy, dx, dy, offsets, n1, mask, res);
    return hipGetLastError();
}

}  // namespace rsac
