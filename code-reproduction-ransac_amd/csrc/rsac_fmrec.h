// rsac_fmrec.h -- the f32 Sampson pre-filter's record of one fundamental matrix (fm_frame,
// fm_write_record), shared by the solve kernels that write it: k_fm_solve_g8 (rsac_kernels.hip) and
// k_fm_solve_g7 (rsac_fm7.hip).  The error model is described at "Float32 Sampson pre-filter" in
// rsac_kernels.hip, where the scoring kernels that read the records live.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include "rsac_internal.h"

namespace rsac {

struct FmFrame {
    float c[4];      // x1 y1 x2 y2 centres
    float is;        // 1 / s
    double s;        // power of 2
    double hb[4];    // bounds of |x^| per coordinate
    double pb[4];    // bounds of |x| (pixel frame)
};

// the ordered-int encoding of k_fm_bounds' minima and maxima back to the float
__device__ __forceinline__ float fm_ord2f(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7FFFFFFF); }

// ws: per problem 4 ordered-int minima then 4 maxima (k_fm_bounds); identical in every kernel
__device__ __forceinline__ FmFrame fm_frame(const int *ws, int prob) {
    FmFrame f;
    double half = 0;
    for (int k = 0; k < 4; ++k) {
        const float lo = fm_ord2f(ws[8 * prob + k]), hi = fm_ord2f(ws[8 * prob + 4 + k]);
        f.c[k] = (lo <= hi) ? (lo + hi) * 0.5f : 0.f;  // empty problem: lo = +inf, hi = -inf
        f.pb[k] = fmax(fabs((double)lo), fabs((double)hi));
        half = fmax(half, fmax((double)hi - f.c[k], (double)f.c[k] - lo));
    }
    int e = 0;
    (void)frexp(half > 0 && half < 1e30 ? half : 1.0, &e);
    f.s = ldexp(1.0, e);  // >= half
    f.is = (float)(1.0 / f.s);
    for (int k = 0; k < 4; ++k) {
        const float lo = fm_ord2f(ws[8 * prob + k]), hi = fm_ord2f(ws[8 * prob + 4 + k]);
        f.hb[k] = fmax((double)hi - f.c[k], (double)f.c[k] - lo) * (1.0 + 1.2e-7) / f.s;
    }
    return f;
}

__device__ __forceinline__ void fm_write_record(const double *F, bool valid, const int *ws, int prob, double T,
                                                float *rec) {
    const FmFrame fr = fm_frame(ws, prob);
    bool finite = valid;
    for (int q = 0; q < 9; ++q) finite = finite && isfinite(F[q]);
    if (!valid || !finite || !(fr.hb[0] == fr.hb[0]) || !(fr.pb[0] < 1e30) || !(fr.pb[1] < 1e30) || !(fr.pb[2] < 1e30) ||
        !(fr.pb[3] < 1e30)) {
#pragma unroll
        for (int q = 0; q < kFModelStride; ++q) rec[q] = 0.f;
        if (!valid) {
            rec[10] = 1.f;   // lo = -1: never an inlier
            rec[12] = -1.f;  // hi = -1 < r^2 = 0: an outlier
        } else {
            rec[9] = rec[11] = __builtin_nanf("");  // every pair undecided: the f64 test decides
        }
        return;
    }
    const double s = fr.s;
    // F^ = T2^T F T1
    double G[9];  // F T1
    for (int i = 0; i < 3; ++i) {
        G[3 * i] = F[3 * i] * s;
        G[3 * i + 1] = F[3 * i + 1] * s;
        G[3 * i + 2] = F[3 * i] * fr.c[0] + F[3 * i + 1] * fr.c[1] + F[3 * i + 2];
    }
    double Fh[9];
    for (int j = 0; j < 3; ++j) {
        Fh[j] = s * G[j];
        Fh[3 + j] = s * G[3 + j];
        Fh[6 + j] = fr.c[2] * G[j] + fr.c[3] * G[3 + j] + G[6 + j];
    }
    // r^2 <= T^ den is homogeneous in F^: a power of two (exact) puts its largest entry in [0.5, 1),
    // so that r32, den32 and the band stay in f32's normal range whatever the scale of the
    // coordinates.  Unscaled, F^ ~ s^2 F reaches 1e19 under one far point of 1e12 (den32 = inf
    // beside a finite r^2 reads as a decided inlier) and 1e-18 for coordinates of 1e-9 (r^2, A den
    // and beta all denormal, beta rounded to 0).  ke also scales the pixel-frame terms below.
    double fmx = 0;
    for (int q = 0; q < 9; ++q) fmx = fmax(fmx, fabs(Fh[q]));
    int ke = 0;
    (void)frexp(fmx > 0 && fmx < 1e300 ? fmx : 1.0, &ke);
    for (int q = 0; q < 9; ++q) Fh[q] = ldexp(Fh[q], -ke);
    const double X1 = fr.hb[0], Y1 = fr.hb[1], X2 = fr.hb[2], Y2 = fr.hb[3];
    const double Ar = fabs(Fh[0]) * X1 + fabs(Fh[1]) * Y1 + fabs(Fh[2]);
    const double Br = fabs(Fh[3]) * X1 + fabs(Fh[4]) * Y1 + fabs(Fh[5]);
    const double Cr = fabs(Fh[6]) * X1 + fabs(Fh[7]) * Y1 + fabs(Fh[8]);
    const double A2 = fabs(Fh[0]) * X2 + fabs(Fh[3]) * Y2 + fabs(Fh[6]);
    const double B2 = fabs(Fh[1]) * X2 + fabs(Fh[4]) * Y2 + fabs(Fh[7]);
    // den32 <= Ar^2 + Br^2 + A2^2 + B2^2 must stay finite in f32 (an infinite den beside a finite
    // r^2 reads as a decided inlier): past the scaling above only the bounds of |x^| can break
    // this.  Such a record leaves every pair to the f64 test.
    if (!(Ar * Ar + Br * Br + A2 * A2 + B2 * B2 < 1e38)) {
#pragma unroll
        for (int q = 0; q < kFModelStride; ++q) rec[q] = 0.f;
        rec[9] = rec[11] = __builtin_nanf("");
        return;
    }
    // pixel-frame sums (the f64 kernel's rounding, ~1e-16 relative of these)
    const double P1 = fr.pb[0], Q1 = fr.pb[1], P2 = fr.pb[2], Q2 = fr.pb[3];
    const double Ap = fmax(fmax(fabs(F[0]) * P1 + fabs(F[1]) * Q1 + fabs(F[2]), fabs(F[3]) * P1 + fabs(F[4]) * Q1 + fabs(F[5])),
                           fmax(fabs(F[0]) * P2 + fabs(F[3]) * Q2 + fabs(F[6]), fabs(F[1]) * P2 + fabs(F[4]) * Q2 + fabs(F[7])));
    const double Rp = P2 * (fabs(F[0]) * P1 + fabs(F[1]) * Q1 + fabs(F[2])) +
                      Q2 * (fabs(F[3]) * P1 + fabs(F[4]) * Q1 + fabs(F[5])) + fabs(F[6]) * P1 + fabs(F[7]) * Q1 + fabs(F[8]);
    constexpr double u = 5.9604644775390625e-08;
    const double e = 4.1 * u * fmax(fmax(Ar, Br), fmax(fmax(A2, B2), Cr)) + 1e-15 * (fmax(fmax(Ar, Br), fmax(A2, B2)) + ldexp(s * Ap, -ke));
    const double er = 7.5 * u * (X2 * Ar + Y2 * Br + Cr) + 1e-15 * ldexp(Rp, -ke);
    const double Th = T / (s * s);
    // eta: any value in (0, 1) keeps the band sound; it trades the band's relative width 2 eta against
    // beta ~ (e_r^2 + 4 T^ e^2) / eta.  1e-3 while the error terms are small beside T^ den; where
    // they are not (rho > 1e-4: a far point moves the frame's centre and the f32 x^ resolve the image
    // coarsely), sqrt(rho / 2), which keeps both near sqrt(2 rho).  den is taken at the corner of the
    // box of x^ where it is smallest, image by image (a far point leaves the image at one end).
    double dmin = 0;
    for (int im = 0; im < 2; ++im) {
        const double X = im ? X2 : X1, Y = im ? Y2 : Y1;
        const double pa0 = Fh[0], pa1 = im ? Fh[3] : Fh[1], pa2 = im ? Fh[6] : Fh[2];
        const double pb0 = im ? Fh[1] : Fh[3], pb1 = Fh[4], pb2 = im ? Fh[7] : Fh[5];
        double part = 0;
        for (int c = 0; c < 4; ++c) {
            const double sx = (c & 2) ? 1.0 : -1.0, sy = (c & 1) ? 1.0 : -1.0;
            const double pa = pa0 * (sx * X) + pa1 * (sy * Y) + pa2, pb = pb0 * (sx * X) + pb1 * (sy * Y) + pb2;
            const double d = pa * pa + pb * pb;
            part = c ? fmin(part, d) : d;
        }
        dmin = im ? dmin + part : part;
    }
    const double rho = (er * er + 4.0 * Th * e * e) / (Th * dmin);
    const double eta = rho > 1e-4 ? fmin(0.5, sqrt(0.5 * rho)) : 1e-3;
    const double Alo = Th * (1.0 - 6.0 * u) / ((1.0 + eta) * (1.0 + eta)) * (1.0 - 1e-6);
    const double b1 = (1.0 + 1.0 / eta) * (er * er + 4.0 * Th * e * e) / (1.0 + eta) * (1.0 + 1e-6);
    const double Chi = Th * (1.0 + 6.0 * u) / ((1.0 - eta) * (1.0 - eta)) * (1.0 + 1e-6);
    const double b2 = (er * er / eta + 4.0 * Th * e * e * (1.0 + 1.0 / eta) / (1.0 - eta)) / (1.0 - eta) * (1.0 + 1e-6);
#pragma unroll
    for (int q = 0; q < 9; ++q) rec[q] = (float)Fh[q];
    // A rounded down, the others up (float conversion rounds to nearest: nudge by 2^-23)
    rec[9] = (float)(Alo * (1.0 - 1.2e-7));
    rec[10] = (float)(b1 * (1.0 + 1.2e-7));
    rec[11] = (float)(Chi * (1.0 + 1.2e-7));
    rec[12] = (float)(b2 * (1.0 + 1.2e-7));
    rec[13] = rec[14] = rec[15] = 0.f;
}

}  // namespace rsac
