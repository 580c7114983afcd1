// The five-point essential matrix solver of the match verification (match_verify.hip:
// verify_pairs_essential_kernel and five_point_kernel), one sample per call, everything f64.  The
// rule is written down in include/iamx.h; tests/essential_reference.py restates it in numpy step by
// step.  Built with -ffp-contract=off like the rest of match_verify.hip: every multiply and add rounds
// on its own, in the order written here.
//
//   null space   5x9 system [ux uy u vx vy v x y 1], Gauss-Jordan with full pivoting -> X Y Z W
//   constraints  E = xX + yY + zZ + W;  det E and (E E^T - tr(E E^T)/2) E expanded over the 20
//                monomials  x3 x2y xy2 y3 x2z x2 xyz xy y2z y2 | xz2 xz x yz2 yz y z3 z2 z 1
//   elimination  Gauss-Jordan of the leading 10x10 block, row pivoting
//   polynomial   rows (x2z, x2), (xyz, xy), (y2z, y2) give B(z) [x y 1]^T = 0; det B(z), degree 10
//   roots        derivative chain: the roots of p^(j+1) cut [-R, R] into intervals on which p^(j) is
//                monotone; a sign change is bisected a fixed number of times
//   models       [x y 1] from the cross product of two rows of B(z), E scaled to unit norm
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FIVE_POINT_FN __host__ __device__ inline
#else
#define FIVE_POINT_FN inline
#endif

#define FIVE_POINT_MAX_ROOTS 10
#define FIVE_POINT_BISECT_INNER 32      /* bisections of a sign change of a derivative */
#define FIVE_POINT_BISECT_LAST 48       /* bisections of a sign change of the polynomial itself */
#define FIVE_POINT_NEWTON 2             /* polishing steps, kept only where they stay in the interval */

namespace five_point {

FIVE_POINT_FN bool finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// degree 1 (x y z 1) times degree 1 -> degree 2 (x2 xy y2 xz yz z2 x y z 1)
FIVE_POINT_FN void mul11(const double *p, const double *q, double *out)
{
    const int T[4][4] = {{0, 1, 3, 6}, {1, 2, 4, 7}, {3, 4, 5, 8}, {6, 7, 8, 9}};
    for (int k = 0; k < 10; ++k) out[k] = 0.0;
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) out[T[a][b]] = out[T[a][b]] + p[a] * q[b];
}

// degree 2 times degree 1 -> degree 3, in the monomial order of the constraint matrix
FIVE_POINT_FN void mul21(const double *p, const double *q, double *out)
{
    const int T[10][4] = {{0, 1, 4, 5},     {1, 2, 6, 7},     {2, 3, 8, 9},    {4, 6, 10, 11},
                          {6, 8, 13, 14},   {10, 13, 16, 17}, {5, 7, 11, 12},  {7, 9, 14, 15},
                          {11, 14, 17, 18}, {12, 15, 18, 19}};
    for (int k = 0; k < 20; ++k) out[k] = 0.0;
    for (int a = 0; a < 10; ++a)
        for (int b = 0; b < 4; ++b) out[T[a][b]] = out[T[a][b]] + p[a] * q[b];
}

// out[k] = sum over i ascending of a[i] b[k - i]
FIVE_POINT_FN void conv(const double *a, int la, const double *b, int lb, double *out)
{
    for (int k = 0; k < la + lb - 1; ++k) {
        double acc = 0.0;
        for (int i = 0; i < la; ++i)
            if (k - i >= 0 && k - i < lb) acc = acc + a[i] * b[k - i];
        out[k] = acc;
    }
}

// q[0 .. deg] ascending
FIVE_POINT_FN double horner(const double *q, int deg, double z)
{
    double v = q[deg];
    for (int i = deg - 1; i >= 0; --i) v = v * z + q[i];
    return v;
}

// unit Frobenius norm, largest-magnitude entry positive; false where an entry is not finite
FIVE_POINT_FN bool unit9(double *M)
{
    double ss = 0.0;
    for (int j = 0; j < 9; ++j) ss = ss + M[j] * M[j];
    const double fro = sqrt(ss);
    double big = -1.0, sign = 1.0;
    for (int j = 0; j < 9; ++j) {
        M[j] = M[j] / fro;
        if (fabs(M[j]) > big) { big = fabs(M[j]); sign = M[j] < 0.0 ? -1.0 : 1.0; }
    }
    bool fin = true;
    for (int j = 0; j < 9; ++j) {
        M[j] = M[j] * sign;
        fin = fin && finite(M[j]);
    }
    return fin;
}

// the camera matrix as the kernels take it: [fx skew cu; 0 fy cv; 0 0 1]
struct Camera {
    double fx, skew, cu, fy, cv;
};

// pixel -> ray
FIVE_POINT_FN void ray(const Camera &k, double u, double v, double &x, double &y)
{
    y = (v - k.cv) / k.fy;
    x = ((u - k.cu) - k.skew * y) / k.fx;
}

// F = K^-T E K^-1 in closed form, unit norm; false where F is not finite
FIVE_POINT_FN bool pixel_model(const Camera &k, const double *E, double *F)
{
    const double a = 1.0 / k.fx, d = 1.0 / k.fy;
    const double b = -((k.skew * d) * a);
    const double c = -(a * k.cu + b * k.cv);
    const double e = -(d * k.cv);
    double G[9];
    for (int i = 0; i < 3; ++i) {
        G[3 * i] = E[3 * i] * a;
        G[3 * i + 1] = E[3 * i] * b + E[3 * i + 1] * d;
        G[3 * i + 2] = (E[3 * i] * c + E[3 * i + 1] * e) + E[3 * i + 2];
    }
    for (int j = 0; j < 3; ++j) {
        F[j] = a * G[j];
        F[3 + j] = b * G[j] + d * G[3 + j];
        F[6 + j] = (c * G[j] + e * G[3 + j]) + G[6 + j];
    }
    return unit9(F);
}

// The real roots of c[0 .. 10] (ascending powers) in ascending order; -1 where the polynomial is
// passed over (a coefficient not finite, a zero leading coefficient, a bound that is not finite).
FIVE_POINT_FN int real_roots(const double *c, double *roots)
{
    const double lead = fabs(c[10]);
    double mx = 0.0;
    bool fin = finite(c[10]);
    for (int i = 0; i < 10; ++i) {
        fin = fin && finite(c[i]);
        if (fabs(c[i]) > mx) mx = fabs(c[i]);
    }
    const double R = 1.0 + mx / lead;
    if (!(fin && lead > 0.0 && finite(R))) return -1;
    double D[10][11];                       // D[j]: the j-th derivative, degree 10 - j
    for (int i = 0; i <= 10; ++i) D[0][i] = c[i];
    for (int j = 1; j < 10; ++j)
        for (int i = 0; i <= 10 - j; ++i) D[j][i] = D[j - 1][i + 1] * (double)(i + 1);
    double pts[12], next[10];
    int count = 0;
    for (int k = 1; k <= 10; ++k) {
        const double *q = D[10 - k];
        const bool last = k == 10;
        pts[0] = -R;
        pts[count + 1] = R;
        int ncount = 0;
        double fa = horner(q, k, pts[0]);
        for (int i = 0; i <= count; ++i) {
            const double a = pts[i], b = pts[i + 1];
            const double fb = horner(q, k, b);
            const bool sa = fa < 0.0;
            if (sa != (fb < 0.0)) {
                double lo = a, hi = b;
                const int steps = last ? FIVE_POINT_BISECT_LAST : FIVE_POINT_BISECT_INNER;
                for (int it = 0; it < steps; ++it) {
                    const double mid = 0.5 * (lo + hi);
                    if ((horner(q, k, mid) < 0.0) == sa) lo = mid; else hi = mid;
                }
                double z = 0.5 * (lo + hi);
                if (last) {
                    for (int it = 0; it < FIVE_POINT_NEWTON; ++it) {
                        const double zn = z - horner(q, 10, z) / horner(D[1], 9, z);
                        if (zn >= a && zn <= b) z = zn;
                    }
                }
                next[ncount++] = z;
            }
            fa = fb;
        }
        count = ncount;
        for (int i = 0; i < count; ++i) pts[i + 1] = next[i];
    }
    for (int i = 0; i < count; ++i) roots[i] = pts[i + 1];
    return count;
}

// One sample: r[5][4] = x1 y1 x2 y2 on calibrated rays.  Writes the models E[root][9] (unit norm,
// largest entry positive, ascending z; an entry that is not finite is left as it comes) and returns
// their number, 0 where the sample is passed over.
FIVE_POINT_FN int solve(const double (*r)[4], double (*E)[9])
{
    const double tiny = 0x1p-40;
    // ---- null space: full pivoting
    double S[5][9];
    double mx = 0.0;
    bool nan = false;
    for (int i = 0; i < 5; ++i) {
        const double x = r[i][0], y = r[i][1], u = r[i][2], v = r[i][3];
        S[i][0] = u * x; S[i][1] = u * y; S[i][2] = u;
        S[i][3] = v * x; S[i][4] = v * y; S[i][5] = v;
        S[i][6] = x; S[i][7] = y; S[i][8] = 1.0;
        for (int j = 0; j < 9; ++j) {
            const double w = fabs(S[i][j]);
            nan = nan || !(w == w);
            if (w > mx) mx = w;
        }
    }
    if (nan) return 0;
    double thr = mx * tiny;
    unsigned used_r = 0, used_c = 0;
    int pivcol[5];
    for (int step = 0; step < 5; ++step) {
        double best = -1.0;
        int pr = 0, pc = 0;
        for (int i = 0; i < 5; ++i)
            for (int j = 0; j < 9; ++j) {
                if ((used_r >> i & 1u) || (used_c >> j & 1u)) continue;
                const double w = fabs(S[i][j]);
                if (w > best) { best = w; pr = i; pc = j; }
            }
        if (!(best > thr)) return 0;
        for (int i = 0; i < 5; ++i) {
            if (i == pr) continue;
            const double f = S[i][pc] / S[pr][pc];
            for (int j = 0; j < 9; ++j) S[i][j] = S[i][j] - f * S[pr][j];
            S[i][pc] = 0.0;
        }
        used_r |= 1u << pr;
        used_c |= 1u << pc;
        pivcol[pr] = pc;
    }
    double P[9][4];                         // entry e of E = x P[e][0] + y P[e][1] + z P[e][2] + P[e][3]
    {
        int k = 0;
        for (int fk = 0; fk < 9; ++fk) {
            if (used_c >> fk & 1u) continue;
            for (int e = 0; e < 9; ++e) P[e][k] = 0.0;
            P[fk][k] = 1.0;
            for (int i = 0; i < 5; ++i) P[pivcol[i]][k] = -S[i][fk] / S[i][pivcol[i]];
            ++k;
        }
    }
    // ---- the ten constraints
    double A[10][20];
    {
        double t0[10], t1[10], m[10], c0[20], c1[20], c2[20];
        mul11(P[4], P[8], t0); mul11(P[5], P[7], t1);
        for (int k = 0; k < 10; ++k) m[k] = t0[k] - t1[k];
        mul21(m, P[0], c0);
        mul11(P[3], P[8], t0); mul11(P[5], P[6], t1);
        for (int k = 0; k < 10; ++k) m[k] = t0[k] - t1[k];
        mul21(m, P[1], c1);
        mul11(P[3], P[7], t0); mul11(P[4], P[6], t1);
        for (int k = 0; k < 10; ++k) m[k] = t0[k] - t1[k];
        mul21(m, P[2], c2);
        for (int k = 0; k < 20; ++k) A[0][k] = (c0[k] - c1[k]) + c2[k];
        double M[3][3][10];                 // E E^T, then its diagonal less half the trace
        for (int i = 0; i < 3; ++i)
            for (int j = i; j < 3; ++j) {
                double t2[10];
                mul11(P[3 * i], P[3 * j], t0);
                mul11(P[3 * i + 1], P[3 * j + 1], t1);
                mul11(P[3 * i + 2], P[3 * j + 2], t2);
                for (int k = 0; k < 10; ++k) {
                    M[i][j][k] = (t0[k] + t1[k]) + t2[k];
                    M[j][i][k] = M[i][j][k];
                }
            }
        for (int k = 0; k < 10; ++k) {
            const double t = 0.5 * ((M[0][0][k] + M[1][1][k]) + M[2][2][k]);
            for (int i = 0; i < 3; ++i) M[i][i][k] = M[i][i][k] - t;
        }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                mul21(M[i][0], P[j], c0);
                mul21(M[i][1], P[3 + j], c1);
                mul21(M[i][2], P[6 + j], c2);
                for (int k = 0; k < 20; ++k) A[1 + 3 * i + j][k] = (c0[k] + c1[k]) + c2[k];
            }
    }
    // ---- Gauss-Jordan of the leading block, rows swapped into place
    mx = 0.0;
    for (int i = 0; i < 10; ++i)
        for (int j = 0; j < 20; ++j) {
            const double w = fabs(A[i][j]);
            nan = nan || !(w == w);
            if (w > mx) mx = w;
        }
    if (nan) return 0;
    thr = mx * tiny;
    for (int c = 0; c < 10; ++c) {
        double best = -1.0;
        int who = c;
        for (int i = c; i < 10; ++i) {
            const double w = fabs(A[i][c]);
            if (w > best) { best = w; who = i; }
        }
        if (!(best > thr)) return 0;
        for (int j = 0; j < 20; ++j) {
            const double t = A[who][j];
            A[who][j] = A[c][j];
            A[c][j] = t;
        }
        const double piv = A[c][c];
        for (int j = 0; j < 20; ++j) A[c][j] = A[c][j] / piv;
        for (int i = 0; i < 10; ++i) {
            if (i == c) continue;
            const double f = A[i][c];
            for (int j = 0; j < 20; ++j) A[i][j] = A[i][j] - f * A[c][j];
            A[i][c] = 0.0;
        }
    }
    // ---- B(z) and its determinant
    double B[3][3][5];
    for (int k = 0; k < 3; ++k) {
        const double *hi = A[4 + 2 * k], *lo = A[5 + 2 * k];
        for (int col = 0; col < 3; ++col) {
            const int last = col == 0 ? 12 : col == 1 ? 15 : 19, deg = col == 2 ? 3 : 2;
            B[k][col][0] = hi[last];
            for (int p = 1; p <= deg; ++p) B[k][col][p] = hi[last - p] - lo[last - (p - 1)];
            B[k][col][deg + 1] = -lo[last - deg];
            if (deg == 2) B[k][col][4] = 0.0;
        }
    }
    double poly[11];
    {
        double u[9], v[9], p1[8], p2[8], p3[7], q1[11], q2[11], q3[11];
        conv(B[1][1], 4, B[2][2], 5, u); conv(B[1][2], 5, B[2][1], 4, v);
        for (int k = 0; k < 8; ++k) p1[k] = u[k] - v[k];
        conv(B[1][0], 4, B[2][2], 5, u); conv(B[1][2], 5, B[2][0], 4, v);
        for (int k = 0; k < 8; ++k) p2[k] = u[k] - v[k];
        conv(B[1][0], 4, B[2][1], 4, u); conv(B[1][1], 4, B[2][0], 4, v);
        for (int k = 0; k < 7; ++k) p3[k] = u[k] - v[k];
        conv(B[0][0], 4, p1, 8, q1);
        conv(B[0][1], 4, p2, 8, q2);
        conv(B[0][2], 5, p3, 7, q3);
        for (int k = 0; k < 11; ++k) poly[k] = (q1[k] - q2[k]) + q3[k];
    }
    double roots[FIVE_POINT_MAX_ROOTS];
    const int count = real_roots(poly, roots);
    if (count <= 0) return 0;
    // ---- models
    for (int rt = 0; rt < count; ++rt) {
        const double z = roots[rt];
        double b[3][3];
        for (int k = 0; k < 3; ++k) {
            b[k][0] = horner(B[k][0], 3, z);
            b[k][1] = horner(B[k][1], 3, z);
            b[k][2] = horner(B[k][2], 4, z);
        }
        double cr[3] = {0.0, 0.0, 0.0}, bn = 0.0;
        for (int pq = 0; pq < 3; ++pq) {
            const double *u = b[pq == 2 ? 1 : 0], *v = b[pq == 0 ? 1 : 2];
            const double w0 = u[1] * v[2] - u[2] * v[1], w1 = u[2] * v[0] - u[0] * v[2],
                         w2 = u[0] * v[1] - u[1] * v[0];
            const double nn = (w0 * w0 + w1 * w1) + w2 * w2;
            if (pq == 0 || nn > bn) { cr[0] = w0; cr[1] = w1; cr[2] = w2; bn = nn; }
        }
        const double x = cr[0] / cr[2], y = cr[1] / cr[2];
        for (int e = 0; e < 9; ++e) E[rt][e] = ((x * P[e][0] + y * P[e][1]) + z * P[e][2]) + P[e][3];
        unit9(E[rt]);
    }
    return count;
}

}  // namespace five_point
