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
#include "bin_select.h"

// (It covers what follows it in THIS file.  The headers above hold no floating-point arithmetic;
//  any that is ever added to them, or to a header included from here on, needs a pragma of its own.)
#pragma clang fp contract(off)

namespace {

using namespace iamx_bs;          // NT = 256, gate(), the bin kernels, walk_bins(), scan_and_pack()
constexpr int NB = IAMX_SMART_BINS;
constexpr int SWEEPS = 12;                 // cyclic Jacobi sweeps of the 9 x 9 eigenproblem
static_assert(NB == 7, "the bins are best_dist < 32 * 2^b, b = 0 .. 6");

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

// the row rule of bin_select.h's bin kernels; a pair that is not active has no rows
struct SmartRule {
    typedef StatArgs Args;
    static __device__ __forceinline__ int n_bins(const StatArgs &) { return NB; }
    const StatArgs &A;
    int64_t b0;
    int n;
    bool oversize;
    const float *xq, *xt, *sq, *st;
    Hm H;
    __device__ __forceinline__ SmartRule(const StatArgs &A_, int p) : A(A_)
    {
        b0 = A.row_off[p];
        const int64_t n64 = A.row_off[p + 1] - b0;
        const bool live = A.active == nullptr || A.active[p] != 0;
        oversize = live && (n64 < 0 || n64 > MAX_ROWS);
        n = !live || oversize ? 0 : (int)n64;
        const int64_t oq = A.kp_off[A.pairs[2 * p]], ot = A.kp_off[A.pairs[2 * p + 1]];
        xq = A.xy + 2 * oq; xt = A.xy + 2 * ot;
        sq = A.size + oq; st = A.size + ot;
#pragma unroll
        for (int j = 0; j < 9; ++j) H.m[j] = A.H[9 * (int64_t)p + j];
    }
    __device__ __forceinline__ unsigned bins(int i, bool &zero, int &t) const
    {
        return choose(A.idx + 3 * (b0 + i), A.d2 + 3 * (b0 + i), i, xq, xt, sq, st, H, A.match_ratio, t, zero);
    }
    __device__ __forceinline__ float4 point(int i, int &t) const
    {
        return make_float4(xq[2 * i], xq[2 * i + 1], xt[2 * t], xt[2 * t + 1]);
    }
};

// ---------------------------------------------------------------------------------
// the walk over a pass' bins
// ---------------------------------------------------------------------------------
struct SelArgs {
    const int32_t *pairs;              // [n_pairs][2] image slots (query, train)
    const int64_t *kp_off;
    const int32_t *key2;               // [total kp][2] round-half-even(100 * kp.pt) ("%.2f")
    const int32_t *active;             // [n_pairs] or null
    double min_pairs;
    Segments S;
    int tab_size;
    int32_t *work;                     // [n_pairs][6 * stride + 2 * tab_size]
    int32_t *best;                     // [n_pairs][2] unique, fitted of the pair's list (read and written)
    int32_t *improved;                 // [n_pairs] 0, or 1 + the bin that was taken last
    int32_t *out_slots;                // [n_pairs][stride][2]
    int32_t *out_cnt, *stats;          // [n_pairs], [n_pairs][NB][3]
    int32_t *flag;
};

// matcher.py:542-555: the walk starts at the pair's running best
__global__ __launch_bounds__(NT) void smart_select_kernel(SelArgs A)
{
    __shared__ int red[NT / 64];
    const int p = blockIdx.x;
    if (A.active && A.active[p] == 0) {                 // nothing of the pair's state is touched
        if (threadIdx.x == 0) A.improved[p] = 0;
        return;
    }
    const Walked w = walk_bins(red, A.S, p, NB, A.min_pairs, PairKeys(A.key2, A.kp_off, A.pairs, p),
                               WorkSlice(A.work, p, A.S.stride, A.tab_size),
                               A.out_slots + (int64_t)p * A.S.stride * 2, A.stats + (int64_t)p * NB * 3,
                               A.best[2 * p], A.best[2 * p + 1]);
    if (threadIdx.x == 0) {
        if (w.refused) atomicAdd(A.flag + 1, 1);
        const int taken = w.refused ? 0 : w.taken;
        A.improved[p] = taken;
        if (taken) {
            // matcher.py:582-593: the fitted list, then the de-duplicated one, against min_pairs
            A.best[2 * p] = w.best;
            A.best[2 * p + 1] = w.best_fit;
            A.out_cnt[p] = (double)w.best_fit >= A.min_pairs && (double)w.best >= A.min_pairs ? w.best : 0;
        }
    }
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
    hipLaunchKernelGGL((bin_count_kernel<NB, SmartRule>), dim3((unsigned)n_pairs), dim3(NT), 0, st, A);
    int rc = iamx::check_launch("iamx_smart_stats");
    if (rc != IAMX_OK) return rc;
    rc = iamx_exclusive_scan_i32(seg_cnt, (int64_t)n_pairs * NB, seg_off, stream);
    if (rc != IAMX_OK) return rc;
    hipLaunchKernelGGL((bin_fill_kernel<NB, SmartRule>), dim3((unsigned)n_pairs), dim3(NT), 0, st, A);
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
    IAMX_REQUIRE_WORK_SLICE(stride, tab_size);
    IAMX_REQUIRE(((uintptr_t)pts & 15) == 0, "pts must be 16-byte aligned");
    hipStream_t st = iamx::as_stream(stream);
    if (n_pairs) {
        SelArgs A{pairs, kp_off, key2, active, min_pairs,
                  {bin_cnt, seg_cnt, seg_off, rows, mask, vstatus, cap, stride},
                  tab_size, work, best, improved, out_slots, out_cnt, stats, flag};
        hipLaunchKernelGGL(smart_select_kernel, dim3((unsigned)n_pairs), dim3(NT), 0, st, A);
        int rc = iamx::check_launch("iamx_smart_select");
        if (rc != IAMX_OK) return rc;
        // the taken bin's inliers, refitted: the next pass' H (the consensus model where the fit fails)
        hipLaunchKernelGGL(fit_kernel, dim3((unsigned)n_pairs), dim3(NT), 0, st, pts, seg_off, mask,
                           (const int32_t *)improved, cap, vmodel, H, fit_status);
        rc = iamx::check_launch("iamx_smart_select");
        if (rc != IAMX_OK) return rc;
    }
    return scan_and_pack("iamx_smart_select", n_pairs, out_cnt, out_off, out_slots, stride, out_rows,
                         out_cap, stream);
}
