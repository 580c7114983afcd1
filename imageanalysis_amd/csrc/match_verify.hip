// RANSAC verification of pair matches -- scripts/lib/matcher.py:90-142 filter_by_transform():
// cv2.findHomography / cv2.findFundamentalMat (RANSAC) on the undistorted keypoints of one pair,
// matches outside the tolerance dropped.  Here: a fixed number of minimal-sample hypotheses per
// pair, sampled by the stateless rule of verify_rule.h, each solved and scored in f64; the mask of
// the hypothesis with the most inliers (ties: the lowest index) is the result.  No refit, no
// adaptive stop: every decision can be restated (tests/verify_reference.py).
//
// One 256-lane workgroup per pair.  Per round of 32 hypotheses:
//   solve   lane = (hypothesis, row): 8 lanes hold the 8x9 system of one hypothesis, 9 doubles each.
//           Gauss-Jordan over the nine columns in order; the pivot search and the pivot row's
//           broadcast are shuffles inside the 8-lane group; the column loop is static.
//   model   the null vector, (fundamental) its smallest singular value zeroed by one-sided Jacobi,
//           the normalisation undone, scaled to unit Frobenius norm, largest entry positive.
//   score   each wave runs its 8 models, four at a time in registers, over the pair's points in LDS.
//   choose  lane 0 walks the 32 counts in hypothesis order.
// The essential model (five-point samples, csrc/five_point.h) has a kernel of its own further down.
// Built with -ffp-contract=off: the scoring pass and the final mask pass evaluate the same
// expression and must round it the same way wherever the compiler inlines it.
#include "iamx_common.h"
#include "verify_rule.h"
#include "five_point.h"

#include <math.h>

namespace {

constexpr int TILE = 2048;        // matches held in LDS at a time (the matcher clips a pair at 2000)
constexpr int HYP_ROUND = 32;     // hypotheses per round: 4 waves x 8 groups of 8 lanes

__device__ __forceinline__ void block_sum4(double (&v)[4], double (*sh)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v[k] += __shfl_xor(v[k], m);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) sh[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = ((sh[0][k] + sh[1][k]) + sh[2][k]) + sh[3][k];
}

__device__ __forceinline__ double dot3(double a0, double b0, double a1, double b1, double a2, double b2)
{
    return (a0 * b0 + a1 * b1) + a2 * b2;
}

// C = A B, 3x3 row major, each entry (a0 b0 + a1 b1) + a2 b2
__device__ __forceinline__ void mat3(const double (&A)[9], const double (&B)[9], double (&C)[9])
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            C[3 * i + j] = dot3(A[3 * i], B[j], A[3 * i + 1], B[3 + j], A[3 * i + 2], B[6 + j]);
}

// Zero the smallest singular value of F (3x3 row major): one-sided Jacobi on the columns, eight
// sweeps (no early exit: the same operations for every input), F V = U S; the column of least norm
// is cleared and F = (U S) V^T.
__device__ __forceinline__ void rank2(double (&F)[9])
{
    double A[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            A[i][j] = F[3 * i + j];
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 8; ++sweep) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const double alpha = dot3(A[0][p], A[0][p], A[1][p], A[1][p], A[2][p], A[2][p]);
                const double beta = dot3(A[0][q], A[0][q], A[1][q], A[1][q], A[2][q], A[2][q]);
                const double gamma = dot3(A[0][p], A[0][q], A[1][p], A[1][q], A[2][p], A[2][q]);
                double c = 1.0, s = 0.0;
                if (gamma != 0.0) {
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    c = 1.0 / sqrt(1.0 + t * t);
                    s = c * t;
                }
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double ap = A[i][p], aq = A[i][q];
                    A[i][p] = c * ap - s * aq;
                    A[i][q] = s * ap + c * aq;
                    const double vp = V[i][p], vq = V[i][q];
                    V[i][p] = c * vp - s * vq;
                    V[i][q] = s * vp + c * vq;
                }
            }
        }
    }
    double nrm[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) nrm[j] = dot3(A[0][j], A[0][j], A[1][j], A[1][j], A[2][j], A[2][j]);
    int k = 0;
    if (nrm[1] < nrm[k]) k = 1;
    if (nrm[2] < (k == 1 ? nrm[1] : nrm[0])) k = 2;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (j == k) A[i][j] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            F[3 * i + j] = dot3(A[i][0], V[j][0], A[i][1], V[j][1], A[i][2], V[j][2]);
}

// Is the match an inlier of M?  The one expression both the scoring and the mask pass use.
template <int MODEL>
__device__ __forceinline__ bool verify_inlier(const double (&M)[9], double x1, double y1, double x2,
                                              double y2, double tol2)
{
    if (MODEL == IAMX_VERIFY_HOMOGRAPHY) {
        const double w = (M[6] * x1 + M[7] * y1) + M[8];
        const double u = ((M[0] * x1 + M[1] * y1) + M[2]) / w;
        const double v = ((M[3] * x1 + M[4] * y1) + M[5]) / w;
        const double dx = u - x2, dy = v - y2;
        const double err = dx * dx + dy * dy;
        return w != 0.0 && fabs(w) <= 1.7976931348623157e308 && err <= tol2;
    } else {
        const double l2x = (M[0] * x1 + M[1] * y1) + M[2];
        const double l2y = (M[3] * x1 + M[4] * y1) + M[5];
        const double l2z = (M[6] * x1 + M[7] * y1) + M[8];
        const double l1x = (M[0] * x2 + M[3] * y2) + M[6];
        const double l1y = (M[1] * x2 + M[4] * y2) + M[7];
        const double e = (x2 * l2x + y2 * l2y) + l2z;
        const double e2 = e * e;
        const double ea = e2 / (l1x * l1x + l1y * l1y);
        const double eb = e2 / (l2x * l2x + l2y * l2y);
        return ea <= tol2 && eb <= tol2;      // max(ea, eb) <= tol2, a NaN in either is an outlier
    }
}

template <int MODEL>
__global__ __launch_bounds__(256) void verify_pairs_kernel(
    const float4 *__restrict__ pts, const int64_t *__restrict__ m_off, int64_t total,
    const double *__restrict__ tol, int hypotheses, uint64_t seed, uint8_t *__restrict__ mask,
    double *__restrict__ out_model, int32_t *__restrict__ out_best, int32_t *__restrict__ status)
{
    constexpr int K = MODEL == IAMX_VERIFY_HOMOGRAPHY ? 4 : 8;
    __shared__ float4 pts_s[TILE];
    __shared__ double red_s[4][4];
    __shared__ double x_s[HYP_ROUND][9];       // null vectors of the round
    __shared__ double model_s[HYP_ROUND][9];   // finished models of the round
    __shared__ int fin_s[HYP_ROUND];
    __shared__ int cnt_s[HYP_ROUND];
    __shared__ double best_model_s[9];
    __shared__ int best_s[2];                  // hypothesis, count

    const int pair = blockIdx.x, tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63, grp = lane >> 3, row = lane & 7;
    const int64_t off = m_off[pair], n64 = m_off[pair + 1] - off;
    double *om = out_model + (int64_t)pair * 9;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);

    if (off < 0 || n64 < 0 || n64 > 0x7fffffff || off + n64 > total) {
        // offsets that leave the arena: nothing of the pair is read or written
        if (tid == 0) {
            status[pair] = IAMX_VERIFY_NO_MODEL;
            out_best[2 * pair] = -1;
            out_best[2 * pair + 1] = 0;
        }
        if (tid < 9) om[tid] = qnan;
        return;
    }
    const int n = (int)n64;
    const float4 *P = pts + off;
    uint8_t *msk = mask + off;

    if (n < K) {
        for (int i = tid; i < n; i += 256) msk[i] = 1;
        if (tid < 9) om[tid] = qnan;
        if (tid == 0) {
            status[pair] = IAMX_VERIFY_TOO_FEW;
            out_best[2 * pair] = -1;
            out_best[2 * pair + 1] = -1;
        }
        return;
    }

    // ---- Hartley normalisation, once per pair
    double s4[4] = {0, 0, 0, 0};
    for (int i = tid; i < n; i += 256) {
        const float4 p = P[i];
        s4[0] += (double)p.x; s4[1] += (double)p.y; s4[2] += (double)p.z; s4[3] += (double)p.w;
    }
    block_sum4(s4, red_s);
    const double cx1 = s4[0] / n, cy1 = s4[1] / n, cx2 = s4[2] / n, cy2 = s4[3] / n;
    double d4[4] = {0, 0, 0, 0};
    for (int i = tid; i < n; i += 256) {
        const float4 p = P[i];
        const double ax = (double)p.x - cx1, ay = (double)p.y - cy1;
        const double bx = (double)p.z - cx2, by = (double)p.w - cy2;
        d4[0] += sqrt(ax * ax + ay * ay);
        d4[1] += sqrt(bx * bx + by * by);
    }
    block_sum4(d4, red_s);
    const double md1 = d4[0] / n, md2 = d4[1] / n;
    const double tl = tol[pair], tol2 = tl * tl;
    const bool sane = md1 > 0.0 && md2 > 0.0 && md1 <= 1.7976931348623157e308
                      && md2 <= 1.7976931348623157e308;
    if (tid == 0) { best_s[0] = -1; best_s[1] = 0; }
    const bool one_tile = n <= TILE;
    if (one_tile)
        for (int i = tid; i < n; i += 256) pts_s[i] = P[i];
    __syncthreads();

    if (sane) {
        const double s1 = 1.4142135623730951 / md1, s2 = 1.4142135623730951 / md2;
        const double T1[9] = {s1, 0.0, -(s1 * cx1), 0.0, s1, -(s1 * cy1), 0.0, 0.0, 1.0};
        const int rounds = (hypotheses + HYP_ROUND - 1) / HYP_ROUND;
        for (int round = 0; round < rounds; ++round) {
            const int hl = wave * 8 + grp;
            const int h = round * HYP_ROUND + hl;
            // ---- this lane's row of the 8x9 system
            int32_t smp[VERIFY_MAX_SAMPLE];
            verify_sample(n, K, h, seed, smp);
            const int want = MODEL == IAMX_VERIFY_HOMOGRAPHY ? (row >> 1) : row;
            int mi = smp[0];
#pragma unroll
            for (int j = 1; j < K; ++j) mi = want == j ? smp[j] : mi;
            const float4 sp = P[mi];
            const double x = ((double)sp.x - cx1) * s1, y = ((double)sp.y - cy1) * s1;
            const double u = ((double)sp.z - cx2) * s2, v = ((double)sp.w - cy2) * s2;
            double a[9];
            if (MODEL == IAMX_VERIFY_HOMOGRAPHY) {
                const bool odd = row & 1;
                const double t = odd ? v : u;
                a[0] = odd ? 0.0 : -x; a[1] = odd ? 0.0 : -y; a[2] = odd ? 0.0 : -1.0;
                a[3] = odd ? -x : 0.0; a[4] = odd ? -y : 0.0; a[5] = odd ? -1.0 : 0.0;
                a[6] = t * x; a[7] = t * y; a[8] = t;
            } else {
                a[0] = u * x; a[1] = u * y; a[2] = u;
                a[3] = v * x; a[4] = v * y; a[5] = v;
                a[6] = x; a[7] = y; a[8] = 1.0;
            }
            double mx = 0.0;
#pragma unroll
            for (int j = 0; j < 9; ++j) mx = fmax(mx, fabs(a[j]));
#pragma unroll
            for (int m = 1; m < 8; m <<= 1) mx = fmax(mx, __shfl_xor(mx, m, 8));
            const double thr = mx * 0x1p-40;
            // ---- Gauss-Jordan over the columns in order
            bool used = false;
            double pval = 1.0;
            int pivcol = -1;
            unsigned free_cols = 0;
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                double pv = used ? -1.0 : fabs(a[c]);
                int who = row;
#pragma unroll
                for (int m = 1; m < 8; m <<= 1) {
                    const double ov = __shfl_xor(pv, m, 8);
                    const int ow = __shfl_xor(who, m, 8);
                    if (ov > pv || (ov == pv && ow < who)) { pv = ov; who = ow; }
                }
                double pj[9];
#pragma unroll
                for (int j = 0; j < 9; ++j) pj[j] = __shfl(a[j], who, 8);
                if (!(pv > thr)) {
                    free_cols |= 1u << c;
                } else if (row == who) {
                    used = true;
                    pivcol = c;
                    pval = a[c];
                } else {
                    const double f = a[c] / pj[c];
#pragma unroll
                    for (int j = 0; j < 9; ++j)
                        if (j != c) a[j] = a[j] - f * pj[j];
                    a[c] = 0.0;
                }
            }
            // ---- the null vector: last free column 1, the other free columns 0, pivots follow
            const int L = 31 - __clz((int)(free_cols | 1u));     // free_cols != 0: 8 rows, 9 columns
            double aL = a[0];
#pragma unroll
            for (int j = 1; j < 9; ++j) aL = L == j ? a[j] : aL;
            if (row == 0) {
#pragma unroll
                for (int j = 0; j < 9; ++j) x_s[hl][j] = j == L ? 1.0 : 0.0;
            }
            __syncthreads();
            if (used) x_s[hl][pivcol] = -aL / pval;
            __syncthreads();
            double Mh[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) Mh[j] = x_s[hl][j];
            // ---- back to pixels
            double M[9], B[9];
            if (MODEL == IAMX_VERIFY_HOMOGRAPHY) {
                const double T2i[9] = {1.0 / s2, 0.0, cx2, 0.0, 1.0 / s2, cy2, 0.0, 0.0, 1.0};
                mat3(T2i, Mh, B);
            } else {
                rank2(Mh);
                const double T2t[9] = {s2, 0.0, 0.0, 0.0, s2, 0.0, -(s2 * cx2), -(s2 * cy2), 1.0};
                mat3(T2t, Mh, B);
            }
            mat3(B, T1, M);
            double ss = 0.0;
#pragma unroll
            for (int j = 0; j < 9; ++j) ss += M[j] * M[j];
            const double fro = sqrt(ss);
            double big = 0.0, sign = 1.0;
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                M[j] = M[j] / fro;
                if (fabs(M[j]) > big) { big = fabs(M[j]); sign = M[j] < 0.0 ? -1.0 : 1.0; }
            }
            bool fin = true;
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                M[j] = sign * M[j];
                fin = fin && fabs(M[j]) <= 1.7976931348623157e308;
            }
            if (row == 0) {
#pragma unroll
                for (int j = 0; j < 9; ++j) model_s[hl][j] = M[j];
                fin_s[hl] = (fin && h < hypotheses) ? 1 : 0;
            }
            __syncthreads();
            // ---- score: this wave's 8 models, four at a time, over every match
            int cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int t0 = 0; t0 < n; t0 += TILE) {
                const int tn = min(TILE, n - t0);
                if (!one_tile) {
                    __syncthreads();
                    for (int i = tid; i < tn; i += 256) pts_s[i] = P[t0 + i];
                    __syncthreads();
                }
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    double Q[4][9];
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int j = 0; j < 9; ++j) Q[m][j] = model_s[wave * 8 + half * 4 + m][j];
                    for (int i = lane; i < tn; i += 64) {
                        const float4 p = pts_s[i];
                        const double x1 = p.x, y1 = p.y, x2 = p.z, y2 = p.w;
#pragma unroll
                        for (int m = 0; m < 4; ++m)
                            cnt[half * 4 + m] += verify_inlier<MODEL>(Q[m], x1, y1, x2, y2, tol2) ? 1 : 0;
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < 8; ++m) {
#pragma unroll
                for (int k = 32; k >= 1; k >>= 1) cnt[m] += __shfl_xor(cnt[m], k);
                if (lane == 0) cnt_s[wave * 8 + m] = cnt[m];
            }
            __syncthreads();
            // ---- choose: most inliers, ties to the lowest hypothesis
            if (tid == 0) {
                int bh = best_s[0], bc = best_s[1], bi = -1;
                for (int i = 0; i < HYP_ROUND; ++i)
                    if (fin_s[i] && cnt_s[i] > bc) { bc = cnt_s[i]; bh = round * HYP_ROUND + i; bi = i; }
                if (bi >= 0) {
                    best_s[0] = bh;
                    best_s[1] = bc;
                    for (int j = 0; j < 9; ++j) best_model_s[j] = model_s[bi][j];
                }
            }
            __syncthreads();
        }
    }

    // ---- the chosen model's mask
    const int bh = best_s[0], bc = best_s[1];
    if (bh < 0) {
        for (int i = tid; i < n; i += 256) msk[i] = 0;
        if (tid < 9) om[tid] = qnan;
        if (tid == 0) {
            status[pair] = IAMX_VERIFY_NO_MODEL;
            out_best[2 * pair] = -1;
            out_best[2 * pair + 1] = 0;
        }
        return;
    }
    double M[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) M[j] = best_model_s[j];
    for (int i = tid; i < n; i += 256) {
        const float4 p = P[i];
        msk[i] = verify_inlier<MODEL>(M, p.x, p.y, p.z, p.w, tol2) ? 1 : 0;
    }
    if (tid < 9) om[tid] = best_model_s[tid];
    if (tid == 0) {
        status[pair] = IAMX_VERIFY_OK;
        out_best[2 * pair] = bh;
        out_best[2 * pair + 1] = bc;
    }
}

// ---- the essential model: five-point samples on calibrated rays (five_point.h), scored as a pixel F.
// Per round of 256 hypotheses:
//   solve   every lane runs one sample through five_point::solve into registers / scratch: at most
//           ten models E each; F = K^-T E K^-1 decides which are valid.
//   order   a candidate's place is the number of valid candidates before it in (hypothesis, root)
//           order (the lanes' counts summed in LDS).
//   pass    CAND_PASS candidates at a time go into the LDS list, in that order;
//   score   each wave takes every fourth group of four: F from E, then over every match;
//   choose  lane 0 walks the pass's counts: most inliers, ties to the earliest (hypothesis, root).
constexpr int ESS_ROUND = 256;
constexpr int CAND_PASS = 320;

__global__ __launch_bounds__(256) void verify_pairs_essential_kernel(
    const float4 *__restrict__ pts, const int64_t *__restrict__ m_off, int64_t total,
    five_point::Camera cam, const double *__restrict__ tol, int hypotheses, uint64_t seed,
    uint8_t *__restrict__ mask, double *__restrict__ out_model, double *__restrict__ out_essential,
    int32_t *__restrict__ out_best, int32_t *__restrict__ status)
{
    constexpr int K = 5;
    __shared__ float4 pts_s[TILE];
    __shared__ double cand_s[CAND_PASS][9];    // E of the pass's candidates
    __shared__ int candh_s[CAND_PASS];         // their hypotheses
    __shared__ int cnt_s[CAND_PASS];
    __shared__ int nvalid_s[ESS_ROUND];
    __shared__ double best_model_s[9], best_ess_s[9];
    __shared__ int best_s[2];                  // hypothesis, count

    const int pair = blockIdx.x, tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int64_t off = m_off[pair], n64 = m_off[pair + 1] - off;
    double *om = out_model + (int64_t)pair * 9;
    double *oe = out_essential ? out_essential + (int64_t)pair * 9 : nullptr;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);

    if (off < 0 || n64 < 0 || n64 > 0x7fffffff || off + n64 > total) {
        // offsets that leave the arena: nothing of the pair is read or written
        if (tid == 0) {
            status[pair] = IAMX_VERIFY_NO_MODEL;
            out_best[2 * pair] = -1;
            out_best[2 * pair + 1] = 0;
        }
        if (tid < 9) { om[tid] = qnan; if (oe) oe[tid] = qnan; }
        return;
    }
    const int n = (int)n64;
    const float4 *P = pts + off;
    uint8_t *msk = mask + off;

    if (n < K) {
        for (int i = tid; i < n; i += 256) msk[i] = 1;
        if (tid < 9) { om[tid] = qnan; if (oe) oe[tid] = qnan; }
        if (tid == 0) {
            status[pair] = IAMX_VERIFY_TOO_FEW;
            out_best[2 * pair] = -1;
            out_best[2 * pair + 1] = -1;
        }
        return;
    }

    const double tl = tol[pair], tol2 = tl * tl;
    if (tid == 0) { best_s[0] = -1; best_s[1] = 0; }
    const bool one_tile = n <= TILE;
    if (one_tile)
        for (int i = tid; i < n; i += 256) pts_s[i] = P[i];
    __syncthreads();

    const int rounds = (hypotheses + ESS_ROUND - 1) / ESS_ROUND;
    for (int round = 0; round < rounds; ++round) {
        // ---- solve: one sample per lane
        const int h = round * ESS_ROUND + tid;
        double Eo[FIVE_POINT_MAX_ROOTS][9];
        int nr = 0;
        unsigned valid = 0;
        if (h < hypotheses) {
            int32_t smp[VERIFY_MAX_SAMPLE];
            verify_sample(n, K, h, seed, smp);
            double r[5][4];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const float4 sp = P[smp[j]];
                five_point::ray(cam, (double)sp.x, (double)sp.y, r[j][0], r[j][1]);
                five_point::ray(cam, (double)sp.z, (double)sp.w, r[j][2], r[j][3]);
            }
            nr = five_point::solve(r, Eo);
            for (int k = 0; k < nr; ++k) {
                bool fin = true;
                for (int j = 0; j < 9; ++j) fin = fin && five_point::finite(Eo[k][j]);
                double F[9];
                fin = five_point::pixel_model(cam, Eo[k], F) && fin;
                valid |= fin ? 1u << k : 0u;
            }
        }
        nvalid_s[tid] = __popc(valid);
        __syncthreads();
        // ---- order: candidates before this lane's, and in the round
        int first = 0, ncand = 0;
        for (int i = 0; i < ESS_ROUND; ++i) {
            const int v = nvalid_s[i];
            first += i < tid ? v : 0;
            ncand += v;
        }
        __syncthreads();
        for (int base = 0; base < ncand; base += CAND_PASS) {
            // ---- pass: candidates base .. base + CAND_PASS - 1 into the list
            int place = first - base;
            for (int k = 0; k < nr; ++k) {
                if (!(valid >> k & 1u)) continue;
                if (place >= 0 && place < CAND_PASS) {
                    for (int j = 0; j < 9; ++j) cand_s[place][j] = Eo[k][j];
                    candh_s[place] = h;
                }
                ++place;
            }
            __syncthreads();
            const int nc = min(CAND_PASS, ncand - base);
            // ---- score: four candidates at a time, every fourth group to this wave
            for (int c0 = wave * 4; c0 < nc; c0 += 16) {
                double Q[4][9];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int slot = min(c0 + m, nc - 1);
                    double E[9];
#pragma unroll
                    for (int j = 0; j < 9; ++j) E[j] = cand_s[slot][j];
                    five_point::pixel_model(cam, E, Q[m]);
                }
                int cnt[4] = {0, 0, 0, 0};
                for (int i = lane; i < n; i += 64) {
                    const float4 p = one_tile ? pts_s[i] : P[i];
                    const double x1 = p.x, y1 = p.y, x2 = p.z, y2 = p.w;
#pragma unroll
                    for (int m = 0; m < 4; ++m)
                        cnt[m] += verify_inlier<IAMX_VERIFY_FUNDAMENTAL>(Q[m], x1, y1, x2, y2, tol2) ? 1 : 0;
                }
#pragma unroll
                for (int m = 0; m < 4; ++m) {
#pragma unroll
                    for (int k = 32; k >= 1; k >>= 1) cnt[m] += __shfl_xor(cnt[m], k);
                    if (lane == 0 && c0 + m < nc) cnt_s[c0 + m] = cnt[m];
                }
            }
            __syncthreads();
            // ---- choose
            if (tid == 0) {
                int bc = best_s[1], bi = -1;
                for (int i = 0; i < nc; ++i)
                    if (cnt_s[i] > bc) { bc = cnt_s[i]; bi = i; }
                if (bi >= 0) {
                    best_s[0] = candh_s[bi];
                    best_s[1] = bc;
                    double E[9], F[9];
                    for (int j = 0; j < 9; ++j) E[j] = cand_s[bi][j];
                    five_point::pixel_model(cam, E, F);
                    for (int j = 0; j < 9; ++j) { best_ess_s[j] = E[j]; best_model_s[j] = F[j]; }
                }
            }
            __syncthreads();
        }
    }

    // ---- the chosen model's mask
    const int bh = best_s[0], bc = best_s[1];
    if (bh < 0) {
        for (int i = tid; i < n; i += 256) msk[i] = 0;
        if (tid < 9) { om[tid] = qnan; if (oe) oe[tid] = qnan; }
        if (tid == 0) {
            status[pair] = IAMX_VERIFY_NO_MODEL;
            out_best[2 * pair] = -1;
            out_best[2 * pair + 1] = 0;
        }
        return;
    }
    double M[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) M[j] = best_model_s[j];
    for (int i = tid; i < n; i += 256) {
        const float4 p = P[i];
        msk[i] = verify_inlier<IAMX_VERIFY_FUNDAMENTAL>(M, p.x, p.y, p.z, p.w, tol2) ? 1 : 0;
    }
    if (tid < 9) { om[tid] = best_model_s[tid]; if (oe) oe[tid] = best_ess_s[tid]; }
    if (tid == 0) {
        status[pair] = IAMX_VERIFY_OK;
        out_best[2 * pair] = bh;
        out_best[2 * pair + 1] = bc;
    }
}

// the solver alone: one sample per lane
__global__ __launch_bounds__(64) void five_point_kernel(const double *__restrict__ rays, int n,
                                                        double *__restrict__ E, int32_t *__restrict__ count)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double r[5][4], Eo[FIVE_POINT_MAX_ROOTS][9];
    for (int j = 0; j < 5; ++j)
        for (int k = 0; k < 4; ++k) r[j][k] = rays[(int64_t)i * 20 + j * 4 + k];
    const int nr = five_point::solve(r, Eo);
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    for (int k = 0; k < FIVE_POINT_MAX_ROOTS; ++k)
        for (int j = 0; j < 9; ++j) E[((int64_t)i * FIVE_POINT_MAX_ROOTS + k) * 9 + j] = k < nr ? Eo[k][j] : qnan;
    count[i] = nr;
}

}  // namespace

extern "C" int iamx_verify_pairs(const float *pts, const int64_t *m_off, int n_pairs, int64_t total,
                                 int model, const double *tol, int hypotheses, uint64_t seed,
                                 uint8_t *mask, double *out_model, int32_t *out_best,
                                 int32_t *status, void *stream)
{
    IAMX_REQUIRE(n_pairs >= 0 && total >= 0 && hypotheses >= 1, "bad size");
    IAMX_REQUIRE(model == IAMX_VERIFY_HOMOGRAPHY || model == IAMX_VERIFY_FUNDAMENTAL, "unknown model");
    IAMX_REQUIRE(m_off && tol && out_model && out_best && status, "null pointer");
    IAMX_REQUIRE(total == 0 || (pts && mask), "null pointer");
    IAMX_REQUIRE(((uintptr_t)pts & 15) == 0, "pts is not 16-byte aligned");
    if (n_pairs == 0) return IAMX_OK;
    const float4 *p4 = reinterpret_cast<const float4 *>(pts);
    if (model == IAMX_VERIFY_HOMOGRAPHY)
        hipLaunchKernelGGL(verify_pairs_kernel<IAMX_VERIFY_HOMOGRAPHY>, dim3((unsigned)n_pairs), dim3(256),
                           0, iamx::as_stream(stream), p4, m_off, total, tol, hypotheses, seed, mask,
                           out_model, out_best, status);
    else
        hipLaunchKernelGGL(verify_pairs_kernel<IAMX_VERIFY_FUNDAMENTAL>, dim3((unsigned)n_pairs), dim3(256),
                           0, iamx::as_stream(stream), p4, m_off, total, tol, hypotheses, seed, mask,
                           out_model, out_best, status);
    return iamx::check_launch("iamx_verify_pairs");
}

extern "C" int iamx_verify_pairs_essential(const float *pts, const int64_t *m_off, int n_pairs,
                                           int64_t total, const double *K, const double *tol,
                                           int hypotheses, uint64_t seed, uint8_t *mask,
                                           double *out_model, double *out_essential, int32_t *out_best,
                                           int32_t *status, void *stream)
{
    IAMX_REQUIRE(n_pairs >= 0 && total >= 0 && hypotheses >= 1, "bad size");
    IAMX_REQUIRE(m_off && K && tol && out_model && out_best && status, "null pointer");
    IAMX_REQUIRE(total == 0 || (pts && mask), "null pointer");
    IAMX_REQUIRE(((uintptr_t)pts & 15) == 0, "pts is not 16-byte aligned");
    IAMX_REQUIRE(K[3] == 0.0 && K[6] == 0.0 && K[7] == 0.0 && K[8] == 1.0,
                 "K is not an upper triangular camera matrix with K[8] = 1");
    IAMX_REQUIRE(five_point::finite(K[0]) && five_point::finite(K[4]) && K[0] != 0.0 && K[4] != 0.0,
                 "K has a focal length that is zero or not finite");
    IAMX_REQUIRE(five_point::finite(K[1]) && five_point::finite(K[2]) && five_point::finite(K[5]),
                 "K has an entry that is not finite");
    if (n_pairs == 0) return IAMX_OK;
    const five_point::Camera cam = {K[0], K[1], K[2], K[4], K[5]};
    hipLaunchKernelGGL(verify_pairs_essential_kernel, dim3((unsigned)n_pairs), dim3(256), 0,
                       iamx::as_stream(stream), reinterpret_cast<const float4 *>(pts), m_off, total, cam,
                       tol, hypotheses, seed, mask, out_model, out_essential, out_best, status);
    return iamx::check_launch("iamx_verify_pairs_essential");
}

extern "C" int iamx_five_point(const double *rays, int n, double *E, int32_t *count, void *stream)
{
    IAMX_REQUIRE(n >= 0, "bad size");
    IAMX_REQUIRE(rays && E && count, "null pointer");
    if (n == 0) return IAMX_OK;
    hipLaunchKernelGGL(five_point_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0,
                       iamx::as_stream(stream), rays, n, E, count);
    return iamx::check_launch("iamx_five_point");
}

extern "C" int iamx_verify_sample(int64_t n, int k, int64_t hyp, uint64_t seed, int32_t *out)
{
    IAMX_REQUIRE(out, "null pointer");
    IAMX_REQUIRE(k >= 1 && k <= VERIFY_MAX_SAMPLE && n >= k && n <= 0x7fffffff && hyp >= 0, "bad size");
    int32_t s[VERIFY_MAX_SAMPLE];
    verify_sample(n, k, hyp, seed, s);
    for (int d = 0; d < k; ++d) out[d] = s[d];
    return IAMX_OK;
}
