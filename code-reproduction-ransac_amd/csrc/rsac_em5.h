// rsac_em5.h -- the five-point essential-matrix solver: one source for the host
// (em_minimal5, the exports rsac_em_minimal5 / rsac_poly_real_roots) and for k_em_solve_g5
// (rsac_em5.hip), which runs the same stages on 16 lanes per sample.  Only IEEE + - * /, sqrt and
// fma, no libm, -ffp-contract=off: both sides return the same bits.
//
// Stages (Nister's construction):
//   1. rays q = Kinv (x, y, 1) in f64 from f32 pixels; rows q2 (x) q1 of a 5 x 9 system; its
//      four-dimensional null space X, Y, Z, W by fm_minimal8's full-pivot Gauss-Jordan (first maximum
//      in row-major order, 1e-12 amax pivot floor; a failed pivot: no models).
//   2. E = x X + y Y + z Z + W; the ten cubic constraints over the 20 monomials of degree <= 3 in
//      Nister's column order (em5_c3): rows 0 .. 8 the entries of 2 E E^T E - tr(E E^T) E, row 9 det E.
//   3. Gauss-Jordan on the first ten columns with row pivoting (first maximum of the column; a zero
//      or NaN pivot: no models); rows 4 .. 9 give the 3 x 3 polynomial matrix B(z) acting on
//      (x, y, 1), and det B(z) is the degree-10 polynomial.
//   4. its real roots in ascending order (poly10 below).
//   5. per root z: (x, y, 1) from the largest cross product of two rows of B(z), kEm5Polish
//      Gauss-Newton steps on the ten constraints in (x, y, z) (em5_polish), E, then
//      F = Kinv2^T E Kinv1 at unit Frobenius norm; a non-finite or zero-norm model is dropped and
//      the rest close up in root order.
#pragma once
#include <string.h>

#include "rsac_math.h"

namespace rsac {

constexpr int kEm5Records = 10;  // hypothesis records a five-point sample owns

// ---------------------------------------------------------------------------
// Real roots of a polynomial of degree <= 10.
// p(x) = sum c[k] x^k.  The effective degree is the highest k whose coefficient is non-zero and
// whose Cauchy bound B = 1 + max_{j<k} |c_j| / |c_k| is finite; higher coefficients are dropped
// (never divided by).  Degree < 1: no roots.  All real roots of p and of its derivatives lie in
// [-B, B] (Gauss-Lucas).  Level d = 1 .. 10 takes D_d = p^(10 - d) (degree d): the roots of D_(d-1)
// in ascending order and +-B cut [-B, B] into intervals on each of which D_d is monotonic; an
// interval holds a root iff D_d is negative at exactly one of its ends, found by bisection
// (poly_bisect, cubic_bisect's rule).  A root of even multiplicity that is not an exact zero at an
// end is not found; an exact zero at an end counts as the interval ends say.
// ---------------------------------------------------------------------------
// n (n - 1) .. (n - m + 1)
RSAC_HD constexpr double em5_ffac(int n, int m) {
    double f = 1.0;
    for (int i = 0; i < m; ++i) f = f * (double)(n - i);
    return f;
}

// the coefficients of D_d = p^(10 - d) -> dc[0 .. d]
template <int D>
RSAC_HD void poly10_deriv(const double *c, double *dc) {
#pragma unroll
    for (int k = 0; k <= D; ++k) dc[k] = c[k + 10 - D] * em5_ffac(k + 10 - D, 10 - D);
}

template <int D>
RSAC_HD double poly_eval(const double *dc, double x) {
    double v = dc[D];
#pragma unroll
    for (int k = D - 1; k >= 0; --k) v = dfma(v, x, dc[k]);
    return v;
}

constexpr int kPolyBisect = 200;
template <int D>
RSAC_HD double poly_bisect(const double *dc, double lo, double hi, bool neg_lo) {
    for (int it = 0; it < kPolyBisect; ++it) {
        const double mid = 0.5 * lo + 0.5 * hi;
        if (mid == lo || mid == hi) break;
        const double v = poly_eval<D>(dc, mid);
        if (v == 0.0) return mid;
        if ((v < 0.0) == neg_lo) lo = mid; else hi = mid;
    }
    return 0.5 * lo + 0.5 * hi;
}

// the effective polynomial -> cc[0 .. 10] (dropped coefficients zeroed) and its bound B; returns
// the effective degree (0: no roots)
RSAC_HD int poly10_plan(const double *c, double *cc, double &B) {
    double pm[11];  // pm[k] = max |c_j|, j < k
    pm[0] = 0.0;
#pragma unroll
    for (int k = 0; k < 10; ++k) pm[k + 1] = dabs(c[k]) > pm[k] ? dabs(c[k]) : pm[k];
#pragma unroll
    for (int k = 0; k <= 10; ++k) cc[k] = c[k];
    int deg = 10;
    B = 0.0;
#pragma unroll
    for (int k = 10; k >= 1; --k) {
        if (deg == k) {
            double b = 0.0;
            bool ok = cc[k] != 0.0;
            if (ok) {
                b = 1.0 + pm[k] / dabs(cc[k]);
                ok = dfinite(b);
            }
            if (ok) B = b;
            else { cc[k] = 0.0; deg = k - 1; }
        }
    }
    return deg;
}

// one level on the host: the roots of D_d between the np ascending roots `prev` of D_(d-1) -> out
template <int D>
inline int poly10_level(const double *cc, double B, const double *prev, int np, double *out) {
    double dc[D + 1];
    poly10_deriv<D>(cc, dc);
    int n = 0;
    for (int j = 0; j <= np; ++j) {
        const double lo = j == 0 ? -B : prev[j - 1], hi = j == np ? B : prev[j];
        const bool nlo = poly_eval<D>(dc, lo) < 0.0, nhi = poly_eval<D>(dc, hi) < 0.0;
        if (nlo != nhi) out[n++] = poly_bisect<D>(dc, lo, hi, nlo);
    }
    return n;
}

// the real roots of c[0] + .. + c[10] x^10 in ascending order -> roots[0 .. n); n <= 10
inline int poly10_real_roots(const double *c, double *roots) {
    double cc[11], B;
    if (poly10_plan(c, cc, B) < 1) return 0;
    double a[10], b[10];
    int n = poly10_level<1>(cc, B, a, 0, b);
    n = poly10_level<2>(cc, B, b, n, a);
    n = poly10_level<3>(cc, B, a, n, b);
    n = poly10_level<4>(cc, B, b, n, a);
    n = poly10_level<5>(cc, B, a, n, b);
    n = poly10_level<6>(cc, B, b, n, a);
    n = poly10_level<7>(cc, B, a, n, b);
    n = poly10_level<8>(cc, B, b, n, a);
    n = poly10_level<9>(cc, B, a, n, b);
    n = poly10_level<10>(cc, B, b, n, roots);
    return n;
}

// ---------------------------------------------------------------------------
// Polynomials in (x, y, z): variables 0 = x, 1 = y, 2 = z, 3 = 1.
// linear: l[v]; quadratic: q[em5_q2(a, b)], a <= b; cubic: c[em5_c3(a, b, c)], a <= b <= c, in
// Nister's column order x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1.
// ---------------------------------------------------------------------------
RSAC_HD constexpr int em5_q2(int a, int b) { return a * 4 - a * (a - 1) / 2 + (b - a); }
RSAC_HD constexpr int em5_c3(int a, int b, int c) {
    switch (a * 16 + b * 4 + c) {
        case 0: return 0;    // x x x
        case 21: return 1;   // y y y
        case 1: return 2;    // x x y
        case 5: return 3;    // x y y
        case 2: return 4;    // x x z
        case 3: return 5;    // x x 1
        case 22: return 6;   // y y z
        case 23: return 7;   // y y 1
        case 6: return 8;    // x y z
        case 7: return 9;    // x y 1
        case 10: return 10;  // x z z
        case 11: return 11;  // x z 1
        case 15: return 12;  // x 1 1
        case 26: return 13;  // y z z
        case 27: return 14;  // y z 1
        case 31: return 15;  // y 1 1
        case 42: return 16;  // z z z
        case 43: return 17;  // z z 1
        case 47: return 18;  // z 1 1
        default: return 19;  // 1 1 1
    }
}
// the cubic monomial of quadratic monomial k times variable v
RSAC_HD constexpr int em5_qa(int k) { return k < 4 ? 0 : k < 7 ? 1 : k < 9 ? 2 : 3; }
RSAC_HD constexpr int em5_qb(int k) { return k < 4 ? k : k < 7 ? k - 3 : k < 9 ? k - 5 : 3; }
RSAC_HD constexpr int em5_qv(int k, int v) {
    const int a = em5_qa(k), b = em5_qb(k);
    return v <= a ? em5_c3(v, a, b) : v <= b ? em5_c3(a, v, b) : em5_c3(a, b, v);
}

// q += a b (SUB: q -= a b), the terms in (va, vb) order
template <bool SUB>
RSAC_HD void em5_lin_mul(const double *a, const double *b, double *q) {
#pragma unroll
    for (int va = 0; va < 4; ++va)
#pragma unroll
        for (int vb = 0; vb < 4; ++vb) {
            const int k = va <= vb ? em5_q2(va, vb) : em5_q2(vb, va);
            q[k] = SUB ? q[k] - a[va] * b[vb] : q[k] + a[va] * b[vb];
        }
}
// c += q l, the terms in (k, v) order
RSAC_HD void em5_quad_mul(const double *q, const double *l, double *c) {
#pragma unroll
    for (int k = 0; k < 10; ++k)
#pragma unroll
        for (int v = 0; v < 4; ++v) c[em5_qv(k, v)] = c[em5_qv(k, v)] + q[k] * l[v];
}

RSAC_HD double em5_sel3(int i, double a, double b, double c) { return i == 0 ? a : i == 1 ? b : c; }

// row r (0 .. 9) of the 10 x 20 constraint matrix; N[v][m]: entry m (row-major) of X, Y, Z, W
RSAC_HD void em5_row(const double (&N)[4][9], int r, double (&row)[20]) {
    double acc[20];
#pragma unroll
    for (int k = 0; k < 20; ++k) acc[k] = 0.0;
    if (r < 9) {
        const int i = r / 3, j = r - 3 * i;
        double Ei[3][4];  // row i of E
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
            for (int v = 0; v < 4; ++v) Ei[m][v] = em5_sel3(i, N[v][m], N[v][3 + m], N[v][6 + m]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {  // (E E^T)_ik E_kj
            double Q[10];
#pragma unroll
            for (int t = 0; t < 10; ++t) Q[t] = 0.0;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                double Ekm[4];
#pragma unroll
                for (int v = 0; v < 4; ++v) Ekm[v] = N[v][3 * k + m];
                em5_lin_mul<false>(Ei[m], Ekm, Q);
            }
            double Ekj[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) Ekj[v] = em5_sel3(j, N[v][3 * k], N[v][3 * k + 1], N[v][3 * k + 2]);
            em5_quad_mul(Q, Ekj, acc);
        }
        double tr[10];  // tr(E E^T): the squares of the nine entries in order
#pragma unroll
        for (int t = 0; t < 10; ++t) tr[t] = 0.0;
#pragma unroll
        for (int m = 0; m < 9; ++m) {
            double Em[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) Em[v] = N[v][m];
            em5_lin_mul<false>(Em, Em, tr);
        }
        double Eij[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) Eij[v] = em5_sel3(j, Ei[0][v], Ei[1][v], Ei[2][v]);
        double T[20];
#pragma unroll
        for (int k = 0; k < 20; ++k) T[k] = 0.0;
        em5_quad_mul(tr, Eij, T);
#pragma unroll
        for (int k = 0; k < 20; ++k) row[k] = 2.0 * acc[k] - T[k];
    } else {
        // det E along the first row: E_0k times its cofactor E_1a E_2b - E_1b E_2a, (a, b) = (1, 2), (2, 0), (0, 1)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int a = (k + 1) % 3, b = (k + 2) % 3;
            double E1a[4], E1b[4], E2a[4], E2b[4], E0k[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                E1a[v] = N[v][3 + a]; E1b[v] = N[v][3 + b];
                E2a[v] = N[v][6 + a]; E2b[v] = N[v][6 + b];
                E0k[v] = N[v][k];
            }
            double Q[10];
#pragma unroll
            for (int t = 0; t < 10; ++t) Q[t] = 0.0;
            em5_lin_mul<false>(E1a, E2b, Q);
            em5_lin_mul<true>(E1b, E2a, Q);
            em5_quad_mul(Q, E0k, acc);
        }
#pragma unroll
        for (int k = 0; k < 20; ++k) row[k] = acc[k];
    }
}

// out[0 .. DA + DB] = a b (degrees DA, DB), the terms in (i, j) order
template <int DA, int DB>
RSAC_HD void em5_pmul(const double *a, const double *b, double *out) {
#pragma unroll
    for (int k = 0; k <= DA + DB; ++k) out[k] = 0.0;
#pragma unroll
    for (int i = 0; i <= DA; ++i)
#pragma unroll
        for (int j = 0; j <= DB; ++j) out[i + j] = out[i + j] + a[i] * b[j];
}

// T[t][j]: columns 10 .. 19 of reduced rows 4 + t (x^2z, x^2, y^2z, y^2, xyz, xy).
// B[i][0], B[i][1]: cubics in z (4 coefficients, lowest first) times x and y; B[i][2]: the quartic;
// row i from reduced rows e = 4 + 2 i, f = 5 + 2 i as <e> - z <f>.  c[0 .. 10] = det B(z).
RSAC_HD void em5_poly(const double (&T)[6][10], double (&B)[3][3][5], double *c) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double *e = T[2 * i], *f = T[2 * i + 1];
#pragma unroll
        for (int u = 0; u < 2; ++u) {  // x: columns 0 .. 2 (x z^2, x z, x); y: 3 .. 5
            B[i][u][0] = e[3 * u + 2];
            B[i][u][1] = e[3 * u + 1] - f[3 * u + 2];
            B[i][u][2] = e[3 * u] - f[3 * u + 1];
            B[i][u][3] = -f[3 * u];
            B[i][u][4] = 0.0;
        }
        B[i][2][0] = e[9];
        B[i][2][1] = e[8] - f[9];
        B[i][2][2] = e[7] - f[8];
        B[i][2][3] = e[6] - f[7];
        B[i][2][4] = -f[6];
    }
    // det = b00 (b11 b22 - b12 b21) - b01 (b10 b22 - b12 b20) + b02 (b10 b21 - b11 b20)
    double p[8], q[8], m[8], t0[11], t1[11], t2[11];
    em5_pmul<3, 4>(B[1][1], B[2][2], p);
    em5_pmul<4, 3>(B[1][2], B[2][1], q);
#pragma unroll
    for (int k = 0; k < 8; ++k) m[k] = p[k] - q[k];
    em5_pmul<3, 7>(B[0][0], m, t0);
    em5_pmul<3, 4>(B[1][0], B[2][2], p);
    em5_pmul<4, 3>(B[1][2], B[2][0], q);
#pragma unroll
    for (int k = 0; k < 8; ++k) m[k] = p[k] - q[k];
    em5_pmul<3, 7>(B[0][1], m, t1);
    double p6[7], q6[7], m6[7];
    em5_pmul<3, 3>(B[1][0], B[2][1], p6);
    em5_pmul<3, 3>(B[1][1], B[2][0], q6);
#pragma unroll
    for (int k = 0; k < 7; ++k) m6[k] = p6[k] - q6[k];
    em5_pmul<4, 6>(B[0][2], m6, t2);
#pragma unroll
    for (int k = 0; k < 11; ++k) c[k] = t0[k] - t1[k] + t2[k];
}

// C = A B^T (3 x 3, row-major), the sums left to right
RSAC_HD void em5_mul_abt(const double *A, const double *B, double *C) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1] + A[3 * i + 2] * B[3 * j + 2];
}

// kEm5Polish Gauss-Newton steps on the ten constraints r(s) = (2 E E^T E - tr(E E^T) E, det E) in
// s = (x, y, z), E = x X + y Y + z Z + W: s -= (J^T J)^-1 J^T r with the 3 x 3 system solved by its
// adjugate.  The elimination, the degree-10 polynomial and the back-substitution lose digits on
// badly conditioned samples; the steps bring a root they located back to the constraints' own
// accuracy.  A step that is not finite (singular J^T J) ends the polish where it stands.
constexpr int kEm5Polish = 6;
RSAC_HD void em5_polish(const double (&N)[4][9], double *s) {
    for (int it = 0; it < kEm5Polish; ++it) {
        double E[9], G[9], GE[9];
#pragma unroll
        for (int m = 0; m < 9; ++m) E[m] = s[0] * N[0][m] + s[1] * N[1][m] + s[2] * N[2][m] + N[3][m];
        em5_mul_abt(E, E, G);
        mat3mul(G, E, GE);
        const double trG = G[0] + G[4] + G[8];
        double r[10];
#pragma unroll
        for (int m = 0; m < 9; ++m) r[m] = 2.0 * GE[m] - trG * E[m];
        // the cofactors of E (d det / d E)
        const double C[9] = {E[4] * E[8] - E[5] * E[7], E[5] * E[6] - E[3] * E[8], E[3] * E[7] - E[4] * E[6],
                             E[2] * E[7] - E[1] * E[8], E[0] * E[8] - E[2] * E[6], E[1] * E[6] - E[0] * E[7],
                             E[1] * E[5] - E[2] * E[4], E[2] * E[3] - E[0] * E[5], E[0] * E[4] - E[1] * E[3]};
        r[9] = E[0] * C[0] + E[1] * C[1] + E[2] * C[2];
        double J[3][10];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            double A1[9], A2[9], dG[9], dGE[9], GN[9];
            em5_mul_abt(N[v], E, A1);
            em5_mul_abt(E, N[v], A2);
#pragma unroll
            for (int m = 0; m < 9; ++m) dG[m] = A1[m] + A2[m];
            mat3mul(dG, E, dGE);
            mat3mul(G, N[v], GN);
            const double trd = dG[0] + dG[4] + dG[8];
            double dd = 0.0;
#pragma unroll
            for (int m = 0; m < 9; ++m) {
                J[v][m] = 2.0 * (dGE[m] + GN[m]) - trd * E[m] - trG * N[v][m];
                dd = dd + C[m] * N[v][m];
            }
            J[v][9] = dd;
        }
        double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
#pragma unroll
        for (int m = 0; m < 10; ++m) {
            a00 = a00 + J[0][m] * J[0][m]; a01 = a01 + J[0][m] * J[1][m]; a02 = a02 + J[0][m] * J[2][m];
            a11 = a11 + J[1][m] * J[1][m]; a12 = a12 + J[1][m] * J[2][m]; a22 = a22 + J[2][m] * J[2][m];
            b0 = b0 + J[0][m] * r[m]; b1 = b1 + J[1][m] * r[m]; b2 = b2 + J[2][m] * r[m];
        }
        const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
        const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
        const double det = a00 * c00 + a01 * c01 + a02 * c02;
        const double d0 = (c00 * b0 + c01 * b1 + c02 * b2) / det;
        const double d1 = (c01 * b0 + c11 * b1 + c12 * b2) / det;
        const double d2 = (c02 * b0 + c12 * b1 + c22 * b2) / det;
        if (!dfinite(d0) || !dfinite(d1) || !dfinite(d2)) break;
        s[0] = s[0] - d0;
        s[1] = s[1] - d1;
        s[2] = s[2] - d2;
    }
}

// the model of root z: F (row-major, unit Frobenius norm) = Kinv2^T E Kinv1 with E = x X + y Y + z Z
// + W; Eo (may be null): E at unit norm.  false for a non-finite or zero-norm result.
RSAC_HD bool em5_model(const double (&N)[4][9], const double (&B)[3][3][5], double z, const double *Kinv1,
                       const double *Kinv2, double *F, double *Eo) {
    double b[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        b[i][0] = poly_eval<3>(B[i][0], z);
        b[i][1] = poly_eval<3>(B[i][1], z);
        b[i][2] = poly_eval<4>(B[i][2], z);
    }
    // (x, y, 1) spans the null space of b: the cross product of two rows, the pair (0,1), (0,2),
    // (1,2) with the largest squared norm (the first such)
    double v[3] = {0.0, 0.0, 0.0}, best = -1.0;
#pragma unroll
    for (int pq = 0; pq < 3; ++pq) {
        const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
        const double w0 = b[p][1] * b[q][2] - b[p][2] * b[q][1];
        const double w1 = b[p][2] * b[q][0] - b[p][0] * b[q][2];
        const double w2 = b[p][0] * b[q][1] - b[p][1] * b[q][0];
        const double nn = w0 * w0 + w1 * w1 + w2 * w2;
        if (nn > best) { best = nn; v[0] = w0; v[1] = w1; v[2] = w2; }
    }
    double s[3] = {v[0] / v[2], v[1] / v[2], z};
    em5_polish(N, s);
    double E[9];
#pragma unroll
    for (int m = 0; m < 9; ++m) E[m] = s[0] * N[0][m] + s[1] * N[1][m] + s[2] * N[2][m] + N[3][m];
    // F = Kinv2^T E Kinv1
    double tmp[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            tmp[3 * i + j] = Kinv2[i] * E[j] + Kinv2[3 + i] * E[3 + j] + Kinv2[6 + i] * E[6 + j];
    mat3mul(tmp, Kinv1, F);
    double nrm = 0.0, ne = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        nrm = nrm + F[k] * F[k];
        ne = ne + E[k] * E[k];
    }
    if (!(nrm > 1e-300) || !dfinite(nrm) || !(ne > 1e-300) || !dfinite(ne)) return false;
    const double in = 1.0 / dsqrt(nrm);
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = F[k] * in;
    if (Eo) {
        const double ie = 1.0 / dsqrt(ne);
#pragma unroll
        for (int k = 0; k < 9; ++k) Eo[k] = E[k] * ie;
    }
    return true;
}

// the ray of a pixel: q = Kinv (x, y, 1), the sums left to right
RSAC_HD void em5_ray(const double *Kinv, float x, float y, double *q) {
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = Kinv[3 * i] * (double)x + Kinv[3 * i + 1] * (double)y + Kinv[3 * i + 2];
}

// x1,y1 -> x2,y2 (pixels; x2^T F x1 = 0) and the inverse intrinsics of the two views: up to ten
// models, row-major 3 x 3 each, at F[0 .. 9 n) (and E[0 .. 9 n) when E is non-null) in ascending
// root order; returns n (0 for a degenerate sample).
inline int em_minimal5(const float (&x1)[5], const float (&y1)[5], const float (&x2)[5], const float (&y2)[5],
                       const double *Kinv1, const double *Kinv2, double *F, double *E) {
    double A[5][9];
    double amax = 0.0;
    for (int i = 0; i < 5; ++i) {
        double q1[3], q2[3];
        em5_ray(Kinv1, x1[i], y1[i], q1);
        em5_ray(Kinv2, x2[i], y2[i], q2);
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) A[i][3 * a + b] = q2[a] * q1[b];
        for (int j = 0; j < 9; ++j) amax = dabs(A[i][j]) > amax ? dabs(A[i][j]) : amax;
    }
    int perm[9] = {0, 1, 2, 3, 4, 5, 6, 7, 8};
    for (int r = 0; r < 5; ++r) {
        int pr = r, pc = r;
        double best = -1.0;
        for (int i = r; i < 5; ++i)
            for (int j = r; j < 9; ++j)
                if (dabs(A[i][j]) > best) { best = dabs(A[i][j]); pr = i; pc = j; }
        if (!(best > 1e-12 * amax)) return 0;
        if (pr != r)
            for (int j = 0; j < 9; ++j) { const double tmp = A[r][j]; A[r][j] = A[pr][j]; A[pr][j] = tmp; }
        if (pc != r) {
            for (int i = 0; i < 5; ++i) { const double tmp = A[i][r]; A[i][r] = A[i][pc]; A[i][pc] = tmp; }
            const int tp = perm[r]; perm[r] = perm[pc]; perm[pc] = tp;
        }
        const double ip = 1.0 / A[r][r];
        for (int i = 0; i < 5; ++i) {
            if (i == r) continue;
            const double f = A[i][r] * ip;
            if (f == 0.0) continue;
            for (int j = r; j < 9; ++j) A[i][j] = A[i][j] - f * A[r][j];
        }
    }
    // null vector t (X, Y, Z, W): free column perm[5 + t] = 1, the other free columns 0
    double N[4][9];
    for (int t = 0; t < 4; ++t) {
        for (int u = 0; u < 4; ++u) N[t][perm[5 + u]] = t == u ? 1.0 : 0.0;
        for (int r = 0; r < 5; ++r) N[t][perm[r]] = -A[r][5 + t] / A[r][r];
    }
    double M[10][20];
    for (int r = 0; r < 10; ++r) em5_row(N, r, M[r]);
    for (int c = 0; c < 10; ++c) {
        int pr = c;
        double best = -1.0;
        for (int i = c; i < 10; ++i)
            if (dabs(M[i][c]) > best) { best = dabs(M[i][c]); pr = i; }
        if (!(best > 0.0)) return 0;
        if (pr != c)
            for (int j = 0; j < 20; ++j) { const double tmp = M[c][j]; M[c][j] = M[pr][j]; M[pr][j] = tmp; }
        const double ip = 1.0 / M[c][c];
        for (int i = 0; i < 10; ++i) {
            if (i == c) continue;
            const double f = M[i][c] * ip;
            if (f == 0.0) continue;
            for (int j = c; j < 20; ++j) M[i][j] = M[i][j] - f * M[c][j];
        }
    }
    double T[6][10];
    for (int t = 0; t < 6; ++t)
        for (int j = 0; j < 10; ++j) T[t][j] = M[4 + t][10 + j] / M[4 + t][4 + t];
    double B[3][3][5], c[11], roots[10];
    em5_poly(T, B, c);
    const int nr = poly10_real_roots(c, roots);
    int n = 0;
    for (int r = 0; r < nr; ++r)
        if (em5_model(N, B, roots[r], Kinv1, Kinv2, F + 9 * n, E ? E + 9 * n : nullptr)) ++n;
    return n;
}

// Kinv = adj(K) / det(K) in f64 (the one formula: the drivers upload what this returns); false for
// a singular or non-finite K
inline bool em5_kinv(const double *K, double *Kinv) {
    const double c00 = K[4] * K[8] - K[5] * K[7], c01 = K[5] * K[6] - K[3] * K[8], c02 = K[3] * K[7] - K[4] * K[6];
    const double det = K[0] * c00 + K[1] * c01 + K[2] * c02;
    if (!dfinite(det) || det == 0.0) return false;
    const double adj[9] = {c00, K[2] * K[7] - K[1] * K[8], K[1] * K[5] - K[2] * K[4],
                           c01, K[0] * K[8] - K[2] * K[6], K[2] * K[3] - K[0] * K[5],
                           c02, K[1] * K[6] - K[0] * K[7], K[0] * K[4] - K[1] * K[3]};
    for (int k = 0; k < 9; ++k) {
        Kinv[k] = adj[k] / det;
        if (!dfinite(Kinv[k])) return false;
    }
    return true;
}

// ---------------------------------------------------------------------------
// Pose (host only)
// ---------------------------------------------------------------------------
// M = K2^T F K1 projected onto the essential manifold: singular values (1, 1, 0) / sqrt 2 (unit
// Frobenius norm), sign: the largest-magnitude entry (the first in row-major order) is positive
inline bool em5_from_fundamental(const double *F, const double *K1, const double *K2, double *E) {
    double K2t[9], tmp[9], M[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) K2t[3 * i + j] = K2[3 * j + i];
    mat3mul(K2t, F, tmp);
    mat3mul(tmp, K1, M);
    for (int k = 0; k < 9; ++k)
        if (!dfinite(M[k])) return false;
    double w[3], ut[3][3], vt[3][3];
    cvq::svd3(M, w, ut, vt);
    if (!(w[1] > 0.0)) return false;  // rank < 2: no essential matrix
    const double s = 0.70710678118654752;
    double big = -1.0;
    int at = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            E[3 * i + j] = s * (ut[0][i] * vt[0][j] + ut[1][i] * vt[1][j]);
            if (dabs(E[3 * i + j]) > big) { big = dabs(E[3 * i + j]); at = 3 * i + j; }
        }
    if (E[at] < 0.0)
        for (int k = 0; k < 9; ++k) E[k] = -E[k];
    return true;
}

inline double em5_det3(const double *R) { return det3_rows(R, R + 3, R + 6); }

// The four (R, t) of E = [t]x R in the order (R_a, +t), (R_a, -t), (R_b, +t), (R_b, -t), R_a = U W V^T,
// R_b = U W^T V^T, t = U's third column (U, V made proper first), x2 ~ R x1 + t.  Every masked point is
// triangulated from its two rays (least squares on d1 R q1 - d2 q2 = -t); it is in front when both
// depths d1 q1_z, d2 q2_z are positive.  -> the candidate with most points in front (ties: the
// earlier one) and, in n_front[4], every candidate's count.  Returns the winner's count.
inline int em5_recover_pose(const double *pts1, const double *pts2, int n, const double *Kinv1, const double *Kinv2,
                            const double *E, const uint8_t *mask, double *R_out, double *t_out, int32_t *n_front) {
    double w[3], ut[3][3], vt[3][3];
    cvq::svd3(E, w, ut, vt);
    double U[9], Vt[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            U[3 * i + j] = ut[j][i];
            Vt[3 * i + j] = vt[i][j];
        }
    if (em5_det3(U) < 0.0)
        for (int k = 0; k < 9; ++k) U[k] = -U[k];
    if (em5_det3(Vt) < 0.0)
        for (int k = 0; k < 9; ++k) Vt[k] = -Vt[k];
    const double W[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1}, Wt[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
    double Rc[2][9], tmp[9];
    mat3mul(U, W, tmp);
    mat3mul(tmp, Vt, Rc[0]);
    mat3mul(U, Wt, tmp);
    mat3mul(tmp, Vt, Rc[1]);
    double t[3] = {U[2], U[5], U[8]};
    const double tn = dsqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    for (int k = 0; k < 3; ++k) t[k] = t[k] / tn;
    int cnt[4] = {0, 0, 0, 0};
    for (int i = 0; i < n; ++i) {
        if (mask && !mask[i]) continue;
        double q1[3], q2[3];
        em5_ray(Kinv1, (float)pts1[2 * i], (float)pts1[2 * i + 1], q1);
        em5_ray(Kinv2, (float)pts2[2 * i], (float)pts2[2 * i + 1], q2);
        for (int cnd = 0; cnd < 4; ++cnd) {
            const double *R = Rc[cnd >> 1];
            const double sg = (cnd & 1) ? -1.0 : 1.0;
            double a[3];
            for (int k = 0; k < 3; ++k) a[k] = R[3 * k] * q1[0] + R[3 * k + 1] * q1[1] + R[3 * k + 2] * q1[2];
            const double aa = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
            const double bb = q2[0] * q2[0] + q2[1] * q2[1] + q2[2] * q2[2];
            const double ab = a[0] * q2[0] + a[1] * q2[1] + a[2] * q2[2];
            const double at = sg * (a[0] * t[0] + a[1] * t[1] + a[2] * t[2]);
            const double bt = sg * (q2[0] * t[0] + q2[1] * t[1] + q2[2] * t[2]);
            const double det = aa * bb - ab * ab;
            const double d1 = (ab * bt - at * bb) / det, d2 = (aa * bt - ab * at) / det;
            if (d1 * q1[2] > 0.0 && d2 * q2[2] > 0.0) cnt[cnd]++;
        }
    }
    int bestc = 0;
    for (int cnd = 1; cnd < 4; ++cnd)
        if (cnt[cnd] > cnt[bestc]) bestc = cnd;
    memcpy(R_out, Rc[bestc >> 1], 9 * sizeof(double));
    for (int k = 0; k < 3; ++k) t_out[k] = (bestc & 1) ? -t[k] : t[k];
    if (n_front)
        for (int k = 0; k < 4; ++k) n_front[k] = cnt[k];
    return cnt[bestc];
}

}  // namespace rsac
