// The 'smart' strategy on the device (gfx950) -- scripts/lib/matcher.py:358-593 smart_pair_matches(),
// the loop body :474-580 for a batch of ordered pairs, one workgroup per pair:
//
//   matcher.py:476       trans_pts = cv2.perspectiveTransform(src_pts, H)     (f64, stored as float32)
//   matcher.py:480-511   per query row, over its <= 3 neighbours: break at distance >= 300, break at
//                        ratio < match_ratio, skip size_diff > 1.25, the smallest
//                        metric = raw_dist * size_diff / ratio (the first survivor always taken)
//   matcher.py:516-524   seven nested bins, best_dist < 32 .. 2048, in query-row order
//   matcher.py:529       a bin below min_pairs is not looked at
//   matcher.py:530-532   src / dst = kp.pt of the bin's matches -> cv2.findHomography(RANSAC, tol)
//   matcher.py:533-541   the inliers in order, count_unique() = len(filter_duplicates())
//   matcher.py:542-555   strictly more unique inliers than the best so far: the bin's inliers become
//                        the pair's list, its homography the next pass' H, and the loop goes on
//   matcher.py:582-593   len(best) >= min_pairs, filter_duplicates, >= min_pairs again
//
// iamx_smart_stats materialises the bins of one pass (points in the layout iamx_verify_pairs reads),
// the caller runs iamx_verify_pairs over the n_pairs * 7 segments, iamx_smart_select reads the masks,
// keeps the pair's running best and list, and refits the taken bin's inliers by least squares
// (iamx_homography_fit's kernel) for the next pass.  The consensus is this package's rule
// (csrc/verify_rule.h), not cv2's, and the refit has no LM polish: parity UNPINNED there.
//
// No contraction anywhere in this file: every expression rounds as the Python it restates.  The
// pragma below is this source's -ffp-contract=off (the build's table of per-file flags stays as it is).
#include "iamx_common.h"
#include "key_dedupe.h"

// (It covers what follows it in THIS file.  The two headers above hold no floating-point arithmetic;
//  any that is ever added to them, or to a header included from here on, needs a pragma of its own.)
#pragma clang fp contract(off)

namespace {

using namespace iamx_kd;          // NT = 256, compact(), dedupe(), block_sum()
constexpr int NB = IAMX_SMART_BINS;
constexpr int MAX_ROWS = 1 << 24;
constexpr int SWEEPS = 12;                 // cyclic Jacobi sweeps of the 9 x 9 eigenproblem
static_assert(NB == 7, "the bins are best_dist < 32 * 2^b, b = 0 .. 6");

typedef int v2i __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double nan_d() { return __longlong_as_double(0x7FF8000000000000LL); }

// ---------------------------------------------------------------------------------
// least-squares homography of one segment, by the whole workgroup
// ---------------------------------------------------------------------------------
// sums of K doubles over the workgroup in a fixed order: lanes by xor tree, then the four waves
template <int K>
__device__ __forceinline__ void block_sum_d(double (&v)[K], double *red)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += __shfl_xor(v[k], m);
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[(threadIdx.x >> 6) * K + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((red[k] + red[K + k]) + red[2 * K + k]) + red[3 * K + k];
}

struct FitLds {
    double red[4 * 45];
    double A[81], V[81];
    double h[9];
    int status;
};

// cv2's least-squares kernel (HomographyEstimatorCallback::runKernel) without the LM polish, with
// Hartley's normalisation: centroid, mean distance sqrt 2.  pts [n][4] from `o` on; mask (or null)
// selects the points.  Every thread returns the status; thread 0 holds H in L.h.
__device__ int fit_segment(const float *__restrict__ pts, const uint8_t *__restrict__ mask, int64_t o,
                           int n, FitLds &L)
{
    const float4 *P = reinterpret_cast<const float4 *>(pts) + o;
    const uint8_t *M = mask ? mask + o : nullptr;
    // centroids
    double s[5] = {0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < n; i += NT) {
        if (M && !M[i]) continue;
        const float4 p = P[i];
        s[0] += (double)p.x; s[1] += (double)p.y; s[2] += (double)p.z; s[3] += (double)p.w;
        s[4] += 1.0;
    }
    block_sum_d<5>(s, L.red);
    const double cnt = s[4];
    if (cnt < 4.0) return IAMX_FIT_TOO_FEW;
    const double c1x = s[0] / cnt, c1y = s[1] / cnt, c2x = s[2] / cnt, c2y = s[3] / cnt;
    // mean distances
    double d[2] = {0, 0};
    for (int i = threadIdx.x; i < n; i += NT) {
        if (M && !M[i]) continue;
        const float4 p = P[i];
        const double ax = (double)p.x - c1x, ay = (double)p.y - c1y;
        const double bx = (double)p.z - c2x, by = (double)p.w - c2y;
        d[0] += sqrt(ax * ax + ay * ay);
        d[1] += sqrt(bx * bx + by * by);
    }
    block_sum_d<2>(d, L.red);
    const double md1 = d[0] / cnt, md2 = d[1] / cnt;
    if (!(md1 > 0.0) || !(md2 > 0.0) || md1 > 1.7e308 || md2 > 1.7e308) return IAMX_FIT_DEGENERATE;
    const double s1 = sqrt(2.0) / md1, s2 = sqrt(2.0) / md2;
    // L^T L, upper triangle
    double a[45];
#pragma unroll
    for (int k = 0; k < 45; ++k) a[k] = 0.0;
    for (int i = threadIdx.x; i < n; i += NT) {
        if (M && !M[i]) continue;
        const float4 p = P[i];
        const double X = ((double)p.x - c1x) * s1, Y = ((double)p.y - c1y) * s1;
        const double x = ((double)p.z - c2x) * s2, y = ((double)p.w - c2y) * s2;
        const double lx[9] = {X, Y, 1.0, 0.0, 0.0, 0.0, -x * X, -x * Y, -x};
        const double ly[9] = {0.0, 0.0, 0.0, X, Y, 1.0, -y * X, -y * Y, -y};
        int k = 0;
#pragma unroll
        for (int j = 0; j < 9; ++j)
#pragma unroll
            for (int c = j; c < 9; ++c, ++k) a[k] += lx[j] * lx[c] + ly[j] * ly[c];
    }
    block_sum_d<45>(a, L.red);
    if (threadIdx.x == 0) {
        double *A = L.A, *V = L.V;
        int k = 0;
        for (int j = 0; j < 9; ++j)
            for (int c = j; c < 9; ++c, ++k) A[9 * j + c] = A[9 * c + j] = a[k];
        for (int j = 0; j < 81; ++j) V[j] = (j % 10 == 0) ? 1.0 : 0.0;
        for (int sweep = 0; sweep < SWEEPS; ++sweep)
            for (int p = 0; p < 8; ++p)
                for (int q = p + 1; q < 9; ++q) {
                    const double apq = A[9 * p + q];
                    if (apq == 0.0) continue;
                    const double theta = (A[9 * q + q] - A[9 * p + p]) / (2.0 * apq);
                    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                    for (int r = 0; r < 9; ++r) {              // columns p, q of A and of V
                        const double u = A[9 * r + p], v = A[9 * r + q];
                        A[9 * r + p] = c * u - sn * v;
                        A[9 * r + q] = sn * u + c * v;
                        const double e = V[9 * r + p], f = V[9 * r + q];
                        V[9 * r + p] = c * e - sn * f;
                        V[9 * r + q] = sn * e + c * f;
                    }
                    for (int r = 0; r < 9; ++r) {              // rows p, q of A
                        const double u = A[9 * p + r], v = A[9 * q + r];
                        A[9 * p + r] = c * u - sn * v;
                        A[9 * q + r] = sn * u + c * v;
                    }
                    A[9 * p + q] = A[9 * q + p] = 0.0;
                }
        int least = 0;
        for (int j = 1; j < 9; ++j)
            if (A[10 * j] < A[10 * least]) least = j;
        double h0[9], m[9], h[9];
        for (int j = 0; j < 9; ++j) h0[j] = V[9 * j + least];
        // H = T2^-1 H0 T1
        const double t1x = -(s1 * c1x), t1y = -(s1 * c1y), is2 = 1.0 / s2;
        for (int r = 0; r < 3; ++r) {
            m[3 * r] = h0[3 * r] * s1;
            m[3 * r + 1] = h0[3 * r + 1] * s1;
            m[3 * r + 2] = (h0[3 * r] * t1x + h0[3 * r + 1] * t1y) + h0[3 * r + 2];
        }
        for (int c = 0; c < 3; ++c) {
            h[c] = m[c] * is2 + c2x * m[6 + c];
            h[3 + c] = m[3 + c] * is2 + c2y * m[6 + c];
            h[6 + c] = m[6 + c];
        }
        const double h22 = h[8];
        bool finite = true;
        for (int j = 0; j < 9; ++j) {
            h[j] = h[j] / h22;
            finite = finite && fabs(h[j]) <= 1.7e308;      // (false for a NaN)
            L.h[j] = h[j];
        }
        L.status = finite ? IAMX_FIT_OK : IAMX_FIT_DEGENERATE;
    }
    __syncthreads();
    return L.status;
}

// taken == null: block b fits segment b.  taken given (the select stage): block b is a pair, and fits
// segment b * NB + taken[b] - 1 where taken[b] > 0, else leaves everything of it alone.
__global__ __launch_bounds__(NT) void fit_kernel(const float *__restrict__ pts,
                                                 const int64_t *__restrict__ seg_off,
                                                 const uint8_t *__restrict__ mask,
                                                 const int32_t *__restrict__ taken, int64_t total,
                                                 const double *__restrict__ fallback,
                                                 double *__restrict__ H, int32_t *__restrict__ status)
{
    __shared__ FitLds L;
    const int b = blockIdx.x;
    int64_t seg = b;
    if (taken) {
        const int t = taken[b];
        if (t <= 0 || t > NB) return;
        seg = (int64_t)b * NB + (t - 1);
    }
    const int64_t o = seg_off[seg], n64 = seg_off[seg + 1] - o;
    int st;
    if (o < 0 || n64 < 0 || o + n64 > total || n64 >= (1ll << 31)) st = IAMX_FIT_DEGENERATE;
    else st = fit_segment(pts, mask, o, (int)n64, L);
    if (threadIdx.x == 0) {
        for (int j = 0; j < 9; ++j)
            H[9 * (int64_t)b + j] = st == IAMX_FIT_OK ? L.h[j] : (fallback ? fallback[9 * seg + j] : nan_d());
        status[b] = st;
    }
}

// ---------------------------------------------------------------------------------
// one pass' candidate choice and bins
// ---------------------------------------------------------------------------------
struct StatArgs {
    const int32_t *idx, *d2;           // [rows][3] iamx_knn3_l2_pairs
    const int64_t *row_off;            // [n_pairs + 1]
    const int32_t *pairs;              // [n_pairs][2] image slots (query, train)
    const int64_t *kp_off;
    const float *xy, *size;            // kp.pt [total kp][2], kp.size [total kp]
    const double *H;                   // [n_pairs][9]
    const int32_t *active;             // [n_pairs] or null
    double match_ratio, min_pairs;
    int64_t cap;
    int32_t *bin_cnt, *seg_cnt;        // [n_pairs][NB]
    int64_t *seg_off;
    float *pts;
    int32_t *rows;
    int32_t *flag;
};

struct Hm { double m[9]; };

// matcher.py:480-524 for query row i: the bins the row's survivor is in (bit b: best_dist <
// 32 << b) and its train row; 0 where no neighbour survives.  zero: the nearest distance is 0.
__device__ __forceinline__ unsigned choose(const int32_t *__restrict__ nn, const int32_t *__restrict__ dd,
                                           int i, const float *__restrict__ xq, const float *__restrict__ xt,
                                           const float *__restrict__ sq, const float *__restrict__ st,
                                           const Hm &H, double match_ratio, int &train, bool &zero)
{
    train = -1;
    const int d0 = dd[0];
    zero = d0 == 0;
    if (zero) return 0u;                   // python divides 0.0 by 0.0 at j = 0: ZeroDivisionError
    // cv2.perspectiveTransform: doubles, the quotient by a reciprocal, stored as float32
    const double x = (double)xq[2 * i], y = (double)xq[2 * i + 1];
    double w = x * H.m[6] + y * H.m[7] + H.m[8];
    float px = 0.0f, py = 0.0f;
    if (w != 0.0) {
        w = 1.0 / w;
        px = (float)((x * H.m[0] + y * H.m[1] + H.m[2]) * w);
        py = (float)((x * H.m[3] + y * H.m[4] + H.m[5]) * w);
    }
    // cv2's DMatch.distance: float32 sqrt of the exact squared distance (csrc/match_knn2.hip)
    const float f0 = (float)sqrt((double)d0);
    const double s1 = (double)sq[i];
    int best = -1;
    double best_metric = 0.0;
    float best_dist = 0.0f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int dj = dd[j];
        if (dj >= 90000) break;            // m[j].distance >= 300 (a missing neighbour too)
        const double ratio = (double)f0 / (double)(float)sqrt((double)dj);
        if (ratio < match_ratio) break;
        const int t = nn[j];
        const float dx = xt[2 * t] - px, dy = xt[2 * t + 1] - py;
        const float raw = (float)sqrt((double)(dx * dx + dy * dy));     // np.linalg.norm of float32
        const double s2 = (double)st[t];
        const double size_diff = s1 > s2 ? s1 / s2 : s2 / s1;
        if (size_diff > 1.25) continue;
        const double metric = (double)raw * size_diff / ratio;
        if (best < 0 || metric < best_metric) {
            best = j;
            best_metric = metric;
            best_dist = raw;
            train = t;
        }
    }
    if (best < 0) return 0u;
    unsigned m = 0;
#pragma unroll
    for (int b = 0; b < NB; ++b)
        if (best_dist < (float)(32 << b)) m |= 1u << b;
    return m | 0x80000000u;                // bit 31: the row has a survivor (it may be in no bin)
}

// is a bin of `len` members looked at?  (matcher.py:529, and the four points a homography needs)
__device__ __forceinline__ bool gate(int len, double min_pairs)
{
    return (double)len >= min_pairs && len >= 4;
}

struct PairCtx {
    int64_t b0;
    int n;
    bool live, oversize;
    const float *xq, *xt, *sq, *st;
    Hm H;
};

__device__ __forceinline__ PairCtx pair_ctx(const StatArgs &A, int p)
{
    PairCtx c;
    c.b0 = A.row_off[p];
    const int64_t n64 = A.row_off[p + 1] - c.b0;
    c.live = A.active == nullptr || A.active[p] != 0;
    c.oversize = c.live && (n64 < 0 || n64 > MAX_ROWS);
    c.n = !c.live || c.oversize ? 0 : (int)n64;
    const int64_t oq = A.kp_off[A.pairs[2 * p]], ot = A.kp_off[A.pairs[2 * p + 1]];
    c.xq = A.xy + 2 * oq; c.xt = A.xy + 2 * ot;
    c.sq = A.size + oq; c.st = A.size + ot;
#pragma unroll
    for (int j = 0; j < 9; ++j) c.H.m[j] = A.H[9 * (int64_t)p + j];
    return c;
}

__global__ __launch_bounds__(NT) void smart_count_kernel(StatArgs A)
{
    __shared__ int wsum[NT / 64][NB];
    const int p = blockIdx.x;
    const PairCtx c = pair_ctx(A, p);
    int cnt[NB], zd = 0;
#pragma unroll
    for (int b = 0; b < NB; ++b) cnt[b] = 0;
    for (int i = threadIdx.x; i < c.n; i += NT) {
        bool zero;
        int t;
        const unsigned m = choose(A.idx + 3 * (c.b0 + i), A.d2 + 3 * (c.b0 + i), i, c.xq, c.xt, c.sq, c.st,
                                  c.H, A.match_ratio, t, zero);
        zd += zero ? 1 : 0;
#pragma unroll
        for (int b = 0; b < NB; ++b) cnt[b] += (m >> b) & 1;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        zd += __shfl_xor(zd, s);
#pragma unroll
        for (int b = 0; b < NB; ++b) cnt[b] += __shfl_xor(cnt[b], s);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b) wsum[threadIdx.x >> 6][b] = cnt[b];
        if (zd) atomicAdd(A.flag, zd);
    }
    if (threadIdx.x == 0 && c.oversize) atomicAdd(A.flag + 1, 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        // a bin with as many members as the last bin that was looked at IS that bin (the bins are
        // nested): its consensus would be the same and cannot win under `>`, so it gets no segment
        int prev = -1;
        for (int b = 0; b < NB; ++b) {
            const int m = wsum[0][b] + wsum[1][b] + wsum[2][b] + wsum[3][b];
            A.bin_cnt[p * NB + b] = m;
            const bool g = gate(m, A.min_pairs);
            A.seg_cnt[p * NB + b] = g && m != prev ? m : 0;
            if (g) prev = m;
        }
    }
}

__global__ __launch_bounds__(NT) void smart_fill_kernel(StatArgs A)
{
    __shared__ int wcnt[NT / 64][NB];
    const int p = blockIdx.x;
    unsigned on = 0;
    int base[NB];
    int64_t first[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        base[b] = 0;
        first[b] = 0;
        if (A.seg_cnt[p * NB + b] > 0) {
            on |= 1u << b;
            first[b] = A.seg_off[p * NB + b];
        }
    }
    if (!on) return;
    const PairCtx c = pair_ctx(A, p);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int s = 0; s < c.n; s += NT) {
        const int i = s + threadIdx.x;
        unsigned m = 0;
        int t = -1;
        if (i < c.n) {
            bool zero;
            m = choose(A.idx + 3 * (c.b0 + i), A.d2 + 3 * (c.b0 + i), i, c.xq, c.xt, c.sq, c.st, c.H,
                       A.match_ratio, t, zero) & on;
        }
        int pre[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const unsigned long long bal = __ballot((m >> b) & 1);
            pre[b] = __popcll(bal & ((1ull << lane) - 1));
            if (lane == 0) wcnt[wave][b] = __popcll(bal);
        }
        __syncthreads();
        if (m) {
            const float x1 = c.xq[2 * i], y1 = c.xq[2 * i + 1], x2 = c.xt[2 * t], y2 = c.xt[2 * t + 1];
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                if (!((m >> b) & 1)) continue;
                int pos = base[b] + pre[b];
                for (int w = 0; w < wave; ++w) pos += wcnt[w][b];
                const int64_t o = first[b] + pos;
                if (o < 0 || o >= A.cap) continue;          // (never: cap >= NB * rows)
                *reinterpret_cast<float4 *>(A.pts + 4 * o) = make_float4(x1, y1, x2, y2);
                *reinterpret_cast<v2i *>(A.rows + 2 * o) = v2i{i, t};
            }
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) base[b] += wcnt[0][b] + wcnt[1][b] + wcnt[2][b] + wcnt[3][b];
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------
// the walk over a pass' bins
// ---------------------------------------------------------------------------------
struct SelArgs {
    const int32_t *pairs;              // [n_pairs][2] image slots (query, train)
    const int64_t *kp_off;
    const int32_t *key2;               // [total kp][2] round-half-even(100 * kp.pt) ("%.2f")
    const int32_t *active;             // [n_pairs] or null
    double min_pairs;
    const int32_t *bin_cnt, *seg_cnt;  // [n_pairs][NB]
    const int64_t *seg_off;            // [n_pairs * NB + 1]
    const int32_t *rows;               // [cap][2]
    const uint8_t *mask;               // [cap] iamx_verify_pairs
    const int32_t *vstatus;            // [n_pairs * NB]
    int64_t cap;
    int stride, tab_size;
    int32_t *work;                     // [n_pairs][6 * stride + 2 * tab_size]
    int32_t *best;                     // [n_pairs][2] unique, fitted of the pair's list (read and written)
    int32_t *improved;                 // [n_pairs] 0, or 1 + the bin that was taken last
    int32_t *out_slots;                // [n_pairs][stride][2]
    int32_t *out_cnt, *stats;          // [n_pairs], [n_pairs][NB][3]
    int32_t *flag;
};

__global__ __launch_bounds__(NT) void smart_select_kernel(SelArgs A)
{
    __shared__ int red[NT / 64];
    const int p = blockIdx.x;
    if (A.active && A.active[p] == 0) {                 // nothing of the pair's state is touched
        if (threadIdx.x == 0) A.improved[p] = 0;
        return;
    }
    int32_t *w = A.work + (int64_t)p * (6 * (int64_t)A.stride + 2 * (int64_t)A.tab_size);
    int32_t *cand = w, *slotq = w + 2 * (int64_t)A.stride, *slott = slotq + A.stride,
            *cont = slott + A.stride, *keep = cont + A.stride, *tabq = keep + A.stride,
            *tabt = tabq + A.tab_size;
    int32_t *out = A.out_slots + (int64_t)p * A.stride * 2;
    int32_t *stat = A.stats + (int64_t)p * NB * 3;
    const int32_t *kq = A.key2 + 2 * A.kp_off[A.pairs[2 * p]], *kt = A.key2 + 2 * A.kp_off[A.pairs[2 * p + 1]];
    int best = A.best[2 * p], best_fit = A.best[2 * p + 1], taken = 0, prev_fit = -1, prev_uniq = -1;
    bool refused = false;
    for (int b = 0; b < NB; ++b) {
        const int seg = p * NB + b, len = A.bin_cnt[seg];
        int fit = -1, uniq = -1;
        if (gate(len, A.min_pairs)) {
            const int n = A.seg_cnt[seg];
            const int64_t o = A.seg_off[seg];
            if (n == 0) {                               // the same set as the bin before it
                fit = prev_fit;
                uniq = prev_uniq;
            } else if (n > A.stride || o < 0 || o + n > A.cap) {
                refused = true;                         // (never: the caller sizes stride and cap)
            } else {
                const uint8_t *mk = A.mask + o;
                const int32_t *rw = A.rows + 2 * o;
                // a bin without a model (IAMX_VERIFY_NO_MODEL) has no inliers
                fit = A.vstatus[seg] != IAMX_VERIFY_OK ? 0 :
                    compact(red, n, [&](int i) { return mk[i] != 0; },
                            [&](int pos, int i) { cand[2 * pos] = rw[2 * i]; cand[2 * pos + 1] = rw[2 * i + 1]; });
                uniq = dedupe(red, kq, kt, cand, fit, tabq, tabt, slotq, slott, cont, keep, A.tab_size);
                if (uniq > best) {                      // strictly more (matcher.py:542)
                    best = uniq;
                    best_fit = fit;
                    taken = b + 1;
                    compact(red, fit, [&](int i) { return keep[i] != 0; },
                            [&](int pos, int i) { out[2 * pos] = cand[2 * i]; out[2 * pos + 1] = cand[2 * i + 1]; });
                }
                prev_fit = fit;
                prev_uniq = uniq;
            }
        }
        if (threadIdx.x == 0) { stat[3 * b] = len; stat[3 * b + 1] = fit; stat[3 * b + 2] = uniq; }
    }
    if (threadIdx.x == 0) {
        if (refused) {
            atomicAdd(A.flag + 1, 1);
            taken = 0;
        }
        A.improved[p] = taken;
        if (taken) {
            // matcher.py:582-593: the fitted list, then the de-duplicated one, against min_pairs
            A.best[2 * p] = best;
            A.best[2 * p + 1] = best_fit;
            A.out_cnt[p] = (double)best_fit >= A.min_pairs && (double)best >= A.min_pairs ? best : 0;
        }
    }
}

__global__ __launch_bounds__(NT) void smart_pack_kernel(const int32_t *__restrict__ cnt,
                                                        const int64_t *__restrict__ off,
                                                        const int32_t *__restrict__ slots, int stride,
                                                        int64_t cap, int32_t *__restrict__ out_rows)
{
    const int p = blockIdx.x;
    const int c = cnt[p];
    const int64_t o = off[p];
    if (c <= 0 || c > stride || o < 0 || o + c > cap) return;
    const v2i *src = reinterpret_cast<const v2i *>(slots) + (int64_t)p * stride;
    v2i *dst = reinterpret_cast<v2i *>(out_rows) + o;
    for (int i = threadIdx.x; i < c; i += NT) dst[i] = src[i];
}

}  // namespace

extern "C" int iamx_homography_fit(const float *pts, const int64_t *seg_off, const uint8_t *mask,
                                   int n_seg, int64_t total, double *H, int32_t *status, void *stream)
{
    IAMX_REQUIRE(pts && seg_off && H && status, "null pointer");
    IAMX_REQUIRE(n_seg >= 0 && total >= 0, "negative count");
    IAMX_REQUIRE(((uintptr_t)pts & 15) == 0, "pts must be 16-byte aligned");
    if (n_seg == 0) return IAMX_OK;
    hipLaunchKernelGGL(fit_kernel, dim3((unsigned)n_seg), dim3(NT), 0, iamx::as_stream(stream), pts,
                       seg_off, mask, (const int32_t *)nullptr, total, (const double *)nullptr, H, status);
    return iamx::check_launch("iamx_homography_fit");
}

extern "C" int iamx_smart_stats(const int32_t *idx, const int32_t *d2, const int64_t *row_off,
                                const int32_t *pairs, const int64_t *kp_off, const float *xy,
                                const float *size, const double *H, const int32_t *active, int n_pairs,
                                double match_ratio, double min_pairs, int64_t cap, int32_t *bin_cnt,
                                int32_t *seg_cnt, int64_t *seg_off, float *pts, int32_t *rows,
                                int32_t *flag, void *stream)
{
    IAMX_REQUIRE(idx && d2 && row_off && pairs && kp_off && xy && size && H && bin_cnt && seg_cnt &&
                     seg_off && pts && rows && flag,
                 "null pointer");
    IAMX_REQUIRE(n_pairs >= 0 && cap >= 0, "negative count");
    IAMX_REQUIRE((int64_t)n_pairs * NB < (1ll << 31), "too many segments");
    IAMX_REQUIRE(((uintptr_t)pts & 15) == 0, "pts must be 16-byte aligned");
    IAMX_REQUIRE(match_ratio == match_ratio, "match_ratio is not a number");
    if (n_pairs == 0) return IAMX_OK;
    hipStream_t st = iamx::as_stream(stream);
    StatArgs A{idx, d2, row_off, pairs, kp_off, xy, size, H, active, match_ratio, min_pairs, cap,
               bin_cnt, seg_cnt, seg_off, pts, rows, flag};
    hipLaunchKernelGGL(smart_count_kernel, dim3((unsigned)n_pairs), dim3(NT), 0, st, A);
    int rc = iamx::check_launch("iamx_smart_stats");
    if (rc != IAMX_OK) return rc;
    rc = iamx_exclusive_scan_i32(seg_cnt, (int64_t)n_pairs * NB, seg_off, stream);
    if (rc != IAMX_OK) return rc;
    hipLaunchKernelGGL(smart_fill_kernel, dim3((unsigned)n_pairs), dim3(NT), 0, st, A);
    return iamx::check_launch("iamx_smart_stats");
}

extern "C" int iamx_smart_select(const int32_t *pairs, const int64_t *kp_off, const int32_t *key2,
                                 const int32_t *active, int n_pairs, double min_pairs,
                                 const int32_t *bin_cnt, const int32_t *seg_cnt, const int64_t *seg_off,
                                 const float *pts, const int32_t *rows, const uint8_t *mask,
                                 const int32_t *vstatus, const double *vmodel, int64_t cap, int stride,
                                 int tab_size, int32_t *work, int32_t *best, int32_t *improved,
                                 int32_t *out_slots, int32_t *out_cnt, int64_t *out_off,
                                 int32_t *out_rows, int64_t out_cap, int32_t *stats, double *H,
                                 int32_t *fit_status, int32_t *flag, void *stream)
{
    IAMX_REQUIRE(pairs && kp_off && key2 && bin_cnt && seg_cnt && seg_off && pts && rows && mask &&
                     vstatus && vmodel && work && best && improved && out_slots && out_cnt && out_off &&
                     out_rows && stats && H && fit_status && flag,
                 "null pointer");
    IAMX_REQUIRE(n_pairs >= 0 && cap >= 0 && out_cap >= 0, "negative count");
    IAMX_REQUIRE((int64_t)n_pairs * NB < (1ll << 31), "too many segments");
    IAMX_REQUIRE(stride >= 1 && stride <= MAX_ROWS, "stride outside 1..2^24");
    IAMX_REQUIRE(tab_size >= 64 && (tab_size & (tab_size - 1)) == 0 && (int64_t)tab_size >= 2 * (int64_t)stride,
                 "tab_size must be a power of two >= max(64, 2 * stride)");
    IAMX_REQUIRE(((uintptr_t)pts & 15) == 0, "pts must be 16-byte aligned");
    hipStream_t st = iamx::as_stream(stream);
    if (n_pairs) {
        SelArgs A{pairs, kp_off, key2, active, min_pairs, bin_cnt, seg_cnt, seg_off, rows, mask, vstatus,
                  cap, stride, tab_size, work, best, improved, out_slots, out_cnt, stats, flag};
        hipLaunchKernelGGL(smart_select_kernel, dim3((unsigned)n_pairs), dim3(NT), 0, st, A);
        int rc = iamx::check_launch("iamx_smart_select");
        if (rc != IAMX_OK) return rc;
        // the taken bin's inliers, refitted: the next pass' H (the consensus model where the fit fails)
        hipLaunchKernelGGL(fit_kernel, dim3((unsigned)n_pairs), dim3(NT), 0, st, pts, seg_off, mask,
                           (const int32_t *)improved, cap, vmodel, H, fit_status);
        rc = iamx::check_launch("iamx_smart_select");
        if (rc != IAMX_OK) return rc;
    }
    const int rc = iamx_exclusive_scan_i32(out_cnt, n_pairs, out_off, stream);
    if (rc != IAMX_OK) return rc;
    if (n_pairs)
        hipLaunchKernelGGL(smart_pack_kernel, dim3((unsigned)n_pairs), dim3(NT), 0, st,
                           (const int32_t *)out_cnt, (const int64_t *)out_off,
                           (const int32_t *)out_slots, stride, out_cap, out_rows);
    return iamx::check_launch("iamx_smart_select");
}
