// rsac_emfit.h -- the calibrated refit of an essential matrix: Levenberg-Marquardt
// on the Sampson residuals of the masked points over the five parameters of (R, t), |t| = 1.  One
// source for the host (em_refine_host, the export rsac_essential_refine) and for k_em_refine
// (rsac_emfit.hip).  Only IEEE + - * /, sqrt and fma, no libm, -ffp-contract=off: both sides return
// the same bits.
//
//   start    em_fit_start: svd3 of E_in, U and V^T made proper, R = U W V^T, t = u3 / |u3| (the first
//            of em5_recover_pose's candidates; the four parameterise +-E and share the minimiser).
//            A non-finite E_in or one with w1 <= kEmFitRank w0: no model.
//   pass     em_fit_matrices: F = Kinv2^T [t]x R Kinv1 and the five directions D_k = Kinv2^T dE_k Kinv1,
//            dE_k = [t]x [e_k]x R (k < 3), [b1]x R, [b2]x R; e = the axis of t's smallest |component|
//            (the first on ties), b1 = (t x e) / |t x e|, b2 = t x b1.
//            em_fit_acc: per masked point the residual r = c / sqrt g and its five derivatives, into the
//            kEmFitSums = 22 sums: count, sum r^2, J^T r (5), J^T J (15, em_fit_idx), each one
//            acc = fma(u, v, acc) in fm_fit's summation order (rsac_math.h, fm_fit_reduce_host).
//   step     em_fit_step after every pass: pass 0 takes the sums as the state's (fewer than 5 masked
//            points or a non-finite sum r^2: no model); a later pass is accepted iff its sum r^2 is
//            strictly lower (state and sums replaced, lambda / 10), else lambda * 10.  Then, but for
//            the last pass, the next trial: (A + lambda diag A) d = -J^T r by em_fit_solve5,
//            R' = Q(d_w) R, t' = (t + d3 b1 + d4 b2) / |.|; a failed or non-finite solve makes the
//            state its own trial, which the next pass rejects.  kEmFitPasses trial passes follow
//            pass 0 whatever the data: the trip count is fixed.
//   finish   em_fit_finish: E = [t]x R / sqrt 2 signed as em5_from_fundamental signs it, F = Kinv2^T E
//            Kinv1 at unit norm, the cost, the count, the accepted steps.
//
// The state lives in LDS on the device (one lane runs start, matrices, step and finish), on the
// stack on the host; its arrays are indexed at run time only there, never in registers.
#pragma once
#include "rsac_em5.h"
#include "rsac_math.h"

namespace rsac {

constexpr int kEmFitPasses = 10;       // trial passes after the initial one
constexpr int kEmFitSums = 22;         // count, sum r^2, J^T r (5), J^T J (15)
constexpr int kEmFitMats = 54;         // F (9), then D_0 .. D_4 (9 each)
constexpr int kEmFitRes = 24;          // the result record: E 9, ok, count, F 9, cost, steps, 2 spare
constexpr double kEmFitRank = 1e-8;    // w1 <= kEmFitRank w0: E_in has rank < 2
constexpr double kEmFitLambda = 1e-3;  // the first damping
// the J^T J sum of (k, l), k <= l, within the 22 sums
RSAC_HD constexpr int em_fit_idx(int k, int l) { return 7 + k * 5 - k * (k - 1) / 2 + (l - k); }

struct EmFitPose {
    double R[9], t[3], b1[3], b2[3];
};
struct EmFitState {
    EmFitPose cur, tri;
    double sums[kEmFitSums];  // the sums at cur
    double lam;
    double M[30], x[5];       // em_fit_solve5's 5 x 6 system and its solution
    int32_t steps, ok;
};

// [v]x M (3 x 3 row-major)
RSAC_HD void em_fit_cross_mul(const double *v, const double *M, double *out) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        out[j] = v[1] * M[6 + j] - v[2] * M[3 + j];
        out[3 + j] = v[2] * M[j] - v[0] * M[6 + j];
        out[6 + j] = v[0] * M[3 + j] - v[1] * M[j];
    }
}

// Kinv2^T E Kinv1, the sums left to right (em5_model's product)
RSAC_HD void em_fit_to_pixels(const double *E, const double *Kinv1, const double *Kinv2, double *F) {
    double tmp[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) tmp[3 * i + j] = Kinv2[i] * E[j] + Kinv2[3 + i] * E[3 + j] + Kinv2[6 + i] * E[6 + j];
    mat3mul(tmp, Kinv1, F);
}

// F = Kinv2^T E Kinv1 at unit Frobenius norm; false for a zero or non-finite product
RSAC_HD bool em_fit_F_of_E(const double *E, const double *Kinv1, const double *Kinv2, double *F) {
    em_fit_to_pixels(E, Kinv1, Kinv2, F);
    double nrm = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) nrm = nrm + F[k] * F[k];
    if (!(nrm > 1e-300) || !dfinite(nrm)) return false;
    const double in = 1.0 / dsqrt(nrm);
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = F[k] * in;
    return true;
}

// the start pose of E_in -> p.R, p.t; false: no model
RSAC_HD bool em_fit_start(const double *E, EmFitPose &p) {
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) fin = fin && dfinite(E[k]);
    if (!fin) return false;
    double w[3], ut[3][3], vt[3][3];
    cvq::svd3(E, w, ut, vt);
    if (!(w[1] > kEmFitRank * w[0])) return false;
    double U[9], Vt[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            U[3 * i + j] = ut[j][i];
            Vt[3 * i + j] = vt[i][j];
        }
    if (det3_rows(U, U + 3, U + 6) < 0.0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) U[k] = -U[k];
    }
    if (det3_rows(Vt, Vt + 3, Vt + 6) < 0.0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) Vt[k] = -Vt[k];
    }
    const double W[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1};
    double tmp[9], R[9];
    mat3mul(U, W, tmp);
    mat3mul(tmp, Vt, R);
    const double tn = dsqrt(U[2] * U[2] + U[5] * U[5] + U[8] * U[8]);
    const double t0 = U[2] / tn, t1 = U[5] / tn, t2 = U[8] / tn;
    fin = dfinite(t0) && dfinite(t1) && dfinite(t2);
#pragma unroll
    for (int k = 0; k < 9; ++k) fin = fin && dfinite(R[k]);
    if (!fin) return false;
#pragma unroll
    for (int k = 0; k < 9; ++k) p.R[k] = R[k];
    p.t[0] = t0;
    p.t[1] = t1;
    p.t[2] = t2;
    return true;
}

// the tangent basis of p.t into p.b1, p.b2, and F, D_0 .. D_4 of the pose -> mats[kEmFitMats]
RSAC_HD void em_fit_matrices(EmFitPose &p, const double *Kinv1, const double *Kinv2, double *mats) {
    const double t0 = p.t[0], t1 = p.t[1], t2 = p.t[2];
    const double a0 = dabs(t0), a1 = dabs(t1), a2 = dabs(t2);
    const int ax = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);
    // t x e_ax
    const double c0 = ax == 0 ? 0.0 : ax == 1 ? -t2 : t1;
    const double c1 = ax == 0 ? t2 : ax == 1 ? 0.0 : -t0;
    const double c2 = ax == 0 ? -t1 : ax == 1 ? t0 : 0.0;
    const double cn = dsqrt(c0 * c0 + c1 * c1 + c2 * c2);
    const double b1[3] = {c0 / cn, c1 / cn, c2 / cn};
    const double b2[3] = {t1 * b1[2] - t2 * b1[1], t2 * b1[0] - t0 * b1[2], t0 * b1[1] - t1 * b1[0]};
    const double t[3] = {t0, t1, t2};
    double R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = p.R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p.b1[k] = b1[k];
        p.b2[k] = b2[k];
    }
    double E[9], G[9], out[9];
    em_fit_cross_mul(t, R, E);
    em_fit_to_pixels(E, Kinv1, Kinv2, out);
#pragma unroll
    for (int k = 0; k < 9; ++k) mats[k] = out[k];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double e[3] = {a == 0 ? 1.0 : 0.0, a == 1 ? 1.0 : 0.0, a == 2 ? 1.0 : 0.0};
        em_fit_cross_mul(e, R, G);
        em_fit_cross_mul(t, G, E);
        em_fit_to_pixels(E, Kinv1, Kinv2, out);
#pragma unroll
        for (int k = 0; k < 9; ++k) mats[9 * (1 + a) + k] = out[k];
    }
    em_fit_cross_mul(b1, R, E);
    em_fit_to_pixels(E, Kinv1, Kinv2, out);
#pragma unroll
    for (int k = 0; k < 9; ++k) mats[36 + k] = out[k];
    em_fit_cross_mul(b2, R, E);
    em_fit_to_pixels(E, Kinv1, Kinv2, out);
#pragma unroll
    for (int k = 0; k < 9; ++k) mats[45 + k] = out[k];
}

// one masked point (x, y) -> (u, v) into the 22 sums a; m: F, then the five D_k
RSAC_HD void em_fit_acc(double x, double y, double u, double v, const double *m, double *a) {
    const double a0 = m[0] * x + m[1] * y + m[2], a1 = m[3] * x + m[4] * y + m[5], a2 = m[6] * x + m[7] * y + m[8];
    const double c = u * a0 + v * a1 + a2;
    const double b0 = m[0] * u + m[3] * v + m[6], b1 = m[1] * u + m[4] * v + m[7];
    const double g = a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1;
    const double sg = dsqrt(g);
    const double r = c / sg;
    const double w = c / (g * sg);  // J_k = dc_k / sqrt g - (dg_k / 2) c / (g sqrt g)
    double J[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double *d = m + 9 * (1 + k);
        const double d0 = d[0] * x + d[1] * y + d[2], d1 = d[3] * x + d[4] * y + d[5], d2 = d[6] * x + d[7] * y + d[8];
        const double dc = u * d0 + v * d1 + d2;
        const double e0 = d[0] * u + d[3] * v + d[6], e1 = d[1] * u + d[4] * v + d[7];
        const double hg = a0 * d0 + a1 * d1 + b0 * e0 + b1 * e1;
        J[k] = dc / sg - hg * w;
    }
    a[0] = a[0] + 1.0;
    a[1] = dfma(r, r, a[1]);
#pragma unroll
    for (int k = 0; k < 5; ++k) a[2 + k] = dfma(J[k], r, a[2 + k]);
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
        for (int l = k; l < 5; ++l) a[em_fit_idx(k, l)] = dfma(J[k], J[l], a[em_fit_idx(k, l)]);
}

// M (5 x 6, row-major: the matrix, then the right-hand side) -> x by Gaussian elimination.  Column
// c = 0 .. 4: the pivot is the first row i >= c of the largest |M[i][c]|; a pivot that is not > 0
// (zero or NaN) fails; the rows c and pivot swap; every row i > c, in order, takes f = M[i][c] /
// M[c][c] and M[i][j] = M[i][j] - f M[c][j] for j = c + 1 .. 5 in order.  Back-substitution from
// row 4 up: s = M[i][5], s = s - M[i][j] x[j] for j = i + 1 .. 4 in order, x[i] = s / M[i][i].
// false for a failed pivot or a non-finite x.  M is indexed at run time: LDS or host memory.
RSAC_HD bool em_fit_solve5(double *M, double *x) {
    for (int c = 0; c < 5; ++c) {
        int pr = c;
        double best = dabs(M[6 * c + c]);
        for (int i = c + 1; i < 5; ++i)
            if (dabs(M[6 * i + c]) > best) { best = dabs(M[6 * i + c]); pr = i; }
        if (!(best > 0.0)) return false;
        if (pr != c)
            for (int j = 0; j < 6; ++j) { const double tmp = M[6 * c + j]; M[6 * c + j] = M[6 * pr + j]; M[6 * pr + j] = tmp; }
        for (int i = c + 1; i < 5; ++i) {
            const double f = M[6 * i + c] / M[6 * c + c];
            for (int j = c + 1; j < 6; ++j) M[6 * i + j] = M[6 * i + j] - f * M[6 * c + j];
        }
    }
    bool fin = true;
    for (int i = 4; i >= 0; --i) {
        double s = M[6 * i + 5];
        for (int j = i + 1; j < 5; ++j) s = s - M[6 * i + j] * x[j];
        x[i] = s / M[6 * i + i];
        fin = fin && dfinite(x[i]);
    }
    return fin;
}

// the trial pose st.tri of the step d from st.cur: R' = Q(d_w) R, Q the rotation of the quaternion
// (1, d_w / 2) normalised; t' = (t + d3 b1 + d4 b2) / |.|.  false for a non-finite result.
RSAC_HD bool em_fit_trial(EmFitState &st, const double *d) {
    const double vx = 0.5 * d[0], vy = 0.5 * d[1], vz = 0.5 * d[2];
    const double nq = dsqrt(1.0 + (vx * vx + vy * vy + vz * vz));
    const double qw = 1.0 / nq, qx = vx / nq, qy = vy / nq, qz = vz / nq;
    const double Q[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy),
                         2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx),
                         2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)};
    double R[9], Rn[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = st.cur.R[k];
    mat3mul(Q, R, Rn);
    const double s0 = st.cur.t[0] + d[3] * st.cur.b1[0] + d[4] * st.cur.b2[0];
    const double s1 = st.cur.t[1] + d[3] * st.cur.b1[1] + d[4] * st.cur.b2[1];
    const double s2 = st.cur.t[2] + d[3] * st.cur.b1[2] + d[4] * st.cur.b2[2];
    const double sn = dsqrt(s0 * s0 + s1 * s1 + s2 * s2);
    const double t0 = s0 / sn, t1 = s1 / sn, t2 = s2 / sn;
    bool fin = dfinite(t0) && dfinite(t1) && dfinite(t2);
#pragma unroll
    for (int k = 0; k < 9; ++k) fin = fin && dfinite(Rn[k]);
    if (!fin) return false;
#pragma unroll
    for (int k = 0; k < 9; ++k) st.tri.R[k] = Rn[k];
    st.tri.t[0] = t0;
    st.tri.t[1] = t1;
    st.tri.t[2] = t2;
    return true;
}

// E_in -> the state at pass 0 and its matrices; false (st.ok = 0): no model, no pass runs
RSAC_HD bool em_fit_begin(EmFitState &st, const double *E_in, const double *Kinv1, const double *Kinv2, double *mats) {
    st.steps = 0;
    st.lam = kEmFitLambda;
    for (int q = 0; q < kEmFitSums; ++q) st.sums[q] = 0.0;
    st.ok = em_fit_start(E_in, st.cur) ? 1 : 0;
    if (!st.ok) return false;
    em_fit_matrices(st.cur, Kinv1, Kinv2, mats);
    return true;
}

// after pass `pass` (0 .. kEmFitPasses) left its sums in tot: the acceptance, then the next trial's
// matrices into mats.  Returns st.ok.
RSAC_HD bool em_fit_step(EmFitState &st, int pass, const double *tot, const double *Kinv1, const double *Kinv2,
                         double *mats) {
    if (pass == 0) {
        for (int q = 0; q < kEmFitSums; ++q) st.sums[q] = tot[q];
        if (!(tot[0] >= 5.0) || !dfinite(tot[1])) {
            st.ok = 0;
            return false;
        }
    } else if (tot[1] < st.sums[1]) {
        st.cur = st.tri;
        for (int q = 0; q < kEmFitSums; ++q) st.sums[q] = tot[q];
        st.lam = st.lam / 10.0;
        st.steps = st.steps + 1;
    } else {
        st.lam = st.lam * 10.0;
    }
    if (pass == kEmFitPasses) return true;
    for (int k = 0; k < 5; ++k) {
        for (int l = 0; l < 5; ++l) st.M[6 * k + l] = st.sums[k <= l ? em_fit_idx(k, l) : em_fit_idx(l, k)];
        st.M[6 * k + k] = st.M[6 * k + k] + st.lam * st.M[6 * k + k];
        st.M[6 * k + 5] = -st.sums[2 + k];
    }
    bool have = em_fit_solve5(st.M, st.x);
    if (have) {
        const double d[5] = {st.x[0], st.x[1], st.x[2], st.x[3], st.x[4]};
        have = em_fit_trial(st, d);
    }
    if (!have) st.tri = st.cur;  // its own trial: the next pass cannot be strictly lower
    em_fit_matrices(st.tri, Kinv1, Kinv2, mats);
    return true;
}

// the result record (kEmFitRes doubles)
RSAC_HD void em_fit_finish(EmFitState &st, const double *Kinv1, const double *Kinv2, double *rec) {
    for (int k = 0; k < kEmFitRes; ++k) rec[k] = 0.0;
    rec[10] = st.sums[0];
    if (!st.ok) return;
    double t[3], R[9], E[9], F[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = st.cur.t[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = st.cur.R[k];
    em_fit_cross_mul(t, R, E);
    double big = -1.0, sign = 1.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        E[k] = E[k] * 0.70710678118654752;
        if (dabs(E[k]) > big) { big = dabs(E[k]); sign = E[k] < 0.0 ? -1.0 : 1.0; }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = sign * E[k];
    if (!em_fit_F_of_E(E, Kinv1, Kinv2, F)) {
        st.ok = 0;
        return;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        rec[k] = E[k];
        rec[11 + k] = F[k];
    }
    rec[9] = 1.0;
    rec[20] = st.sums[1];
    rec[21] = (double)st.steps;
}

// the refit on the host over f32 SoA points -> rec[kEmFitRes]; returns whether there is a model
inline bool em_refine_host(const float *x1, const float *y1, const float *x2, const float *y2, const uint8_t *mask, int n,
                           const double *Kinv1, const double *Kinv2, const double *E_in, double *rec) {
    EmFitState st;
    double mats[kEmFitMats], tot[kEmFitSums];
    if (em_fit_begin(st, E_in, Kinv1, Kinv2, mats)) {
        double *part = new double[(size_t)kLmThreads * kEmFitSums];
        for (int pass = 0; pass <= kEmFitPasses; ++pass) {
            fm_fit_reduce_host(n, mask, kEmFitSums, part, tot, [&](int64_t i, double *a) {
                em_fit_acc((double)x1[i], (double)y1[i], (double)x2[i], (double)y2[i], mats, a);
            });
            if (!em_fit_step(st, pass, tot, Kinv1, Kinv2, mats)) break;
        }
        delete[] part;
    }
    em_fit_finish(st, Kinv1, Kinv2, rec);
    return st.ok != 0;
}

}  // namespace rsac
