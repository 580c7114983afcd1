// Surface-consistency and depth culls of match chains (gfx950) -- the rules the reference's
// scripts/4c-surface-outliers3.py and scripts/4c-by-depth.py apply, in today's matches_grouped
// layout.  All arithmetic is f64.  Contraction is switched off for the whole file by the pragma
// below the includes (the file's own statement of -ffp-contract=off; build.sh's flag table has no
// entry for it): every product and sum is rounded on its own, in the order
// tests/surface_cull_restatement.py writes them.  No
// floating-point atomics anywhere: every sum has one fixed order (left to right where a rule says
// so, a fixed tree over fixed tiles otherwise), so no result depends on the launch geometry or
// differs between two runs.  Integer atomics only count.
//
//   surface_knn_fit      per observation of an image-major table: its min(k, n) nearest
//                        observations of the same image in pixels, order (d2, index), the
//                        reference's walk (at most n_pos neighbours with d2 > 0), the closed-form
//                        line of 3-D distance over pixel distance through the used neighbours, and
//                        per used neighbour |line - distance| addressed to the neighbour's chain.
//   surface_chain_metric per chain the sum of what is addressed to it, in (observation, slot)
//                        order, and the count.
//   chain_outlier_stats  mean and population deviation of a metric over the looked-at chains, the
//                        one- or two-sided flag, the flagged chains compacted in ascending order.
//   chain_depths         camera-to-point distances, their per-image mean and deviation, per chain
//                        the mean |depth - image mean| over its members.
#include <math.h>

#include "iamx_common.h"

// no multiply and add of this file's own expressions is fused, host or device (the bit-for-bit cases
// of tests/test_surface_cull_gpu.py are what holds it to that)
#pragma clang fp contract(off)

namespace {

constexpr int KNN_QUERIES = 128;    // queries (threads) of one workgroup
constexpr int KNN_TILE = 256;       // candidates staged in LDS at a time
constexpr int MAX_K = IAMX_SURFACE_MAX_K;
constexpr int NT = 256;             // threads of every other kernel here, and IAMX_CHAIN_STATS_TILE
static_assert(NT == IAMX_CHAIN_STATS_TILE, "the fixed reduction tile is one workgroup");

// the image that owns observation o: the last i with img_ptr[i] <= o (empty images are passed over)
__device__ __forceinline__ int image_of(const int64_t *__restrict__ img_ptr, int n_images, int64_t o)
{
    int lo = 0, hi = n_images;          // invariant: img_ptr[lo] <= o, answer in [lo, hi)
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (img_ptr[mid] <= o) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ double dist3(const double *__restrict__ ned, int64_t a, int64_t b)
{
    const double dx = ned[3 * a] - ned[3 * b], dy = ned[3 * a + 1] - ned[3 * b + 1],
                 dz = ned[3 * a + 2] - ned[3 * b + 2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// One workgroup per block of KNN_QUERIES consecutive observations.  The table is image-major, so a
// block's queries lie in a run of images: the workgroup walks that run, stages each image's pixels
// through LDS in tiles of KNN_TILE, and the lanes whose query is of that image keep their
// neighbour list.  The list (d2 and index, kk entries per lane, slot-major so that the lanes of a
// wave hit different banks) lives in dynamic LDS: indexed at run time it would otherwise be scratch.
__global__ __launch_bounds__(KNN_QUERIES) void surface_knn_fit_kernel(
    const int64_t *__restrict__ img_ptr, const double *__restrict__ uv, const double *__restrict__ ned,
    const int32_t *__restrict__ chain, int n_images, int64_t n_obs, int k, int n_pos,
    int32_t *__restrict__ tgt, double *__restrict__ val, int32_t *__restrict__ used,
    double *__restrict__ fit, int32_t *__restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double *l_d2 = reinterpret_cast<double *>(lds_raw);                   // [k][KNN_QUERIES]
    double *t_u = l_d2 + (size_t)k * KNN_QUERIES;                         // [KNN_TILE]
    double *t_v = t_u + KNN_TILE;                                         // [KNN_TILE]
    int32_t *l_ix = reinterpret_cast<int32_t *>(t_v + KNN_TILE);          // [k][KNN_QUERIES]
    __shared__ int s_first, s_last;

    const int lane = threadIdx.x;
    const int64_t q0 = (int64_t)blockIdx.x * KNN_QUERIES;
    const int64_t q = q0 + lane;
    const bool live = q < n_obs;
    int my_img = -1;
    double qu = 0.0, qv = 0.0;
    if (live) {
        my_img = image_of(img_ptr, n_images, q);
        qu = uv[2 * q];
        qv = uv[2 * q + 1];
    }
    if (lane == 0) s_first = my_img;
    if (live && (q + 1 == n_obs || lane == KNN_QUERIES - 1)) s_last = my_img;
    __syncthreads();
    const int first = s_first, last = s_last;

    int cnt = 0, kk = 0;
    double worst = 0.0;
    bool small = true;
    for (int im = first; im <= last; ++im) {
        int64_t lo = img_ptr[im], hi = img_ptr[im + 1];
        lo = lo < 0 ? 0 : lo;
        hi = hi > n_obs ? n_obs : hi;
        const int64_t n = hi - lo;
        if (n <= 0) continue;
        const bool mine = live && my_img == im && n >= 3;
        if (live && my_img == im) {
            small = n < 3;
            kk = n < (int64_t)k ? (int)n : k;
        }
        if (n < 3) continue;                                              // (uniform: n is the workgroup's)
        for (int64_t base = lo; base < hi; base += KNN_TILE) {
            const int len = hi - base < KNN_TILE ? (int)(hi - base) : KNN_TILE;
            __syncthreads();
            for (int t = lane; t < len; t += KNN_QUERIES) {
                t_u[t] = uv[2 * (base + t)];
                t_v[t] = uv[2 * (base + t) + 1];
            }
            __syncthreads();
            if (!mine) continue;
            for (int t = 0; t < len; ++t) {
                const double du = qu - t_u[t], dv = qv - t_v[t];
                const double d2 = du * du + dv * dv;
                // candidates come in ascending index: an equal d2 never displaces an earlier one
                if (cnt < kk || d2 < worst) {
                    int s = cnt < kk ? cnt : kk - 1;
                    while (s > 0 && l_d2[(s - 1) * KNN_QUERIES + lane] > d2) {
                        l_d2[s * KNN_QUERIES + lane] = l_d2[(s - 1) * KNN_QUERIES + lane];
                        l_ix[s * KNN_QUERIES + lane] = l_ix[(s - 1) * KNN_QUERIES + lane];
                        --s;
                    }
                    l_d2[s * KNN_QUERIES + lane] = d2;
                    l_ix[s * KNN_QUERIES + lane] = (int32_t)(base + t - lo);
                    if (cnt < kk) ++cnt;
                    if (cnt == kk) worst = l_d2[(kk - 1) * KNN_QUERIES + lane];
                }
            }
        }
    }
    if (!live) return;
    const int64_t lo = img_ptr[my_img] < 0 ? 0 : img_ptr[my_img];

    // the reference's walk: the list in order, stopping in front of positive neighbour n_pos + 1
    int m = 0, positives = 0;
    double sx = 0.0, sy = 0.0;
    if (!small) {
        for (int s = 0; s < cnt; ++s) {
            const double d2 = l_d2[s * KNN_QUERIES + lane];
            if (d2 > 0.0 && ++positives > n_pos) break;
            sx = sx + sqrt(d2);
            sy = sy + dist3(ned, q, lo + l_ix[s * KNN_QUERIES + lane]);
            ++m;
        }
    }
    double a = 0.0, b = 0.0;
    int st = small ? IAMX_SURFACE_SKIPPED_SMALL : IAMX_SURFACE_SKIPPED_FLAT;
    if (m > 0) {
        const double xm = sx / (double)m, ym = sy / (double)m;
        double sxx = 0.0, sxy = 0.0;
        for (int s = 0; s < m; ++s) {
            const double ex = sqrt(l_d2[s * KNN_QUERIES + lane]) - xm;
            const double ey = dist3(ned, q, lo + l_ix[s * KNN_QUERIES + lane]) - ym;
            sxx = sxx + ex * ex;
            sxy = sxy + ex * ey;
        }
        if (sxx == 0.0) {
            m = 0;
        } else if (sxx != sxx) {                                           // NaN pixels or positions: no line
            m = 0;
        } else {
            a = sxy / sxx;
            b = ym - a * xm;
            st = IAMX_SURFACE_FITTED;
        }
    }
    int32_t *my_tgt = tgt + q * k;
    double *my_val = val + q * k;
    for (int s = 0; s < m; ++s) {
        const int64_t j = lo + l_ix[s * KNN_QUERIES + lane];
        const double x = sqrt(l_d2[s * KNN_QUERIES + lane]);
        const double y = dist3(ned, q, j);
        my_tgt[s] = chain[j];
        my_val[s] = fabs((a * x + b) - y);
    }
    for (int s = m; s < k; ++s) {
        my_tgt[s] = -1;
        my_val[s] = 0.0;
    }
    used[q] = m;
    fit[2 * q] = a;
    fit[2 * q + 1] = b;
    status[q] = st;
}

// ---------------------------------------------------------------------------------------------
// per-chain sums in (observation, slot) order: count, scan, unordered fill, per-chain sort
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void metric_count_kernel(const int32_t *__restrict__ tgt, int64_t n_slots,
                                                          int64_t n_chains, int32_t *__restrict__ count)
{
    const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (e >= n_slots) return;
    const int c = tgt[e];
    if (c >= 0 && c < n_chains) atomicAdd(&count[c], 1);
}

__global__ __launch_bounds__(NT) void metric_fill_kernel(const int32_t *__restrict__ tgt, int64_t n_slots,
                                                         int64_t n_chains, const int64_t *__restrict__ off,
                                                         int32_t *__restrict__ cursor, int32_t *__restrict__ order)
{
    const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (e >= n_slots) return;
    const int c = tgt[e];
    if (c < 0 || c >= n_chains) return;
    const int at = atomicAdd(&cursor[c], 1);
    const int64_t pos = off[c] + at;
    if (pos < off[c + 1] && pos < n_slots) order[pos] = (int32_t)e;
}

__device__ __forceinline__ void sift_down(int32_t *__restrict__ h, int64_t root, int64_t end)
{
    for (;;) {
        int64_t child = 2 * root + 1;
        if (child >= end) return;
        if (child + 1 < end && h[child] < h[child + 1]) ++child;
        if (h[root] >= h[child]) return;
        const int32_t t = h[root];
        h[root] = h[child];
        h[child] = t;
        root = child;
    }
}

// one thread per chain: its slots' indices come in the order the fill's atomics fell; sorting them
// ascending (heapsort, in place) gives the one order the sum is defined in
__global__ __launch_bounds__(NT) void metric_sum_kernel(
    const double *__restrict__ val, int64_t n_slots, int64_t n_chains, const int64_t *__restrict__ off,
    int32_t *__restrict__ order, const uint8_t *__restrict__ looked, double *__restrict__ sum,
    const int32_t *__restrict__ count, double *__restrict__ metric, unsigned long long *__restrict__ counters)
{
    __shared__ int s_uncounted, s_looked;
    if (threadIdx.x == 0) s_uncounted = s_looked = 0;
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (c < n_chains) {
        int64_t b = off[c], e = off[c + 1];
        if (b < 0 || e > n_slots || e < b) b = e = 0;
        int32_t *h = order + b;
        const int64_t n = e - b;
        for (int64_t i = n / 2 - 1; i >= 0; --i) sift_down(h, i, n);
        for (int64_t end = n - 1; end > 0; --end) {
            const int32_t t = h[0];
            h[0] = h[end];
            h[end] = t;
            sift_down(h, 0, end);
        }
        double s = 0.0;
        for (int64_t i = 0; i < n; ++i) {
            const int64_t at = h[i];
            if (at >= 0 && at < n_slots) s = s + val[at];
        }
        sum[c] = s;
        metric[c] = n > 0 ? s / (double)count[c] : 0.0;
        if (looked[c]) {
            atomicAdd(&s_looked, 1);
            if (n == 0) atomicAdd(&s_uncounted, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_uncounted) atomicAdd(&counters[IAMX_SURFACE_N_UNCOUNTED], (unsigned long long)s_uncounted);
        if (s_looked) atomicAdd(&counters[IAMX_SURFACE_N_LOOKED], (unsigned long long)s_looked);
    }
}

__global__ __launch_bounds__(NT) void metric_zero_kernel(int64_t n_chains, const uint8_t *__restrict__ looked,
                                                         double *__restrict__ sum, int32_t *__restrict__ count,
                                                         double *__restrict__ metric,
                                                         unsigned long long *__restrict__ counters)
{
    const int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (c >= n_chains) return;
    sum[c] = 0.0;
    count[c] = 0;
    metric[c] = 0.0;
    if (looked[c]) {
        atomicAdd(&counters[IAMX_SURFACE_N_UNCOUNTED], 1ull);
        atomicAdd(&counters[IAMX_SURFACE_N_LOOKED], 1ull);
    }
}

__global__ __launch_bounds__(NT) void status_count_kernel(const int32_t *__restrict__ status, int64_t n_obs,
                                                          unsigned long long *__restrict__ counters)
{
    __shared__ int s_small, s_flat;
    if (threadIdx.x == 0) s_small = s_flat = 0;
    __syncthreads();
    const int64_t o = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (o < n_obs) {
        const int st = status[o];
        if (st == IAMX_SURFACE_SKIPPED_SMALL) atomicAdd(&s_small, 1);
        if (st == IAMX_SURFACE_SKIPPED_FLAT) atomicAdd(&s_flat, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_small) atomicAdd(&counters[IAMX_SURFACE_N_SMALL], (unsigned long long)s_small);
        if (s_flat) atomicAdd(&counters[IAMX_SURFACE_N_FLAT], (unsigned long long)s_flat);
    }
}

// ---------------------------------------------------------------------------------------------
// fixed-tree sums: a tile is NT consecutive entries, one per thread, folded pairwise in LDS; the
// tiles' sums are folded by ONE workgroup (thread t takes tiles t, t + NT, ... left to right, then
// the same LDS tree).  Neither step knows the grid.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_tree(double v, double *__restrict__ s)
{
    s[threadIdx.x] = v;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] = s[threadIdx.x] + s[threadIdx.x + w];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ int block_tree_int(int v, int *__restrict__ s)
{
    s[threadIdx.x] = v;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] = s[threadIdx.x] + s[threadIdx.x + w];
        __syncthreads();
    }
    const int r = s[0];
    __syncthreads();
    return r;
}

// pass 0: tile sums of metric and of the looked-at count; pass 1: of (average - metric)^2
__global__ __launch_bounds__(NT) void stats_tile_kernel(const double *__restrict__ metric,
                                                        const uint8_t *__restrict__ looked, int64_t n_chains,
                                                        int pass, const double *__restrict__ stats,
                                                        double *__restrict__ part, int32_t *__restrict__ part_n)
{
    __shared__ double s_d[NT];
    __shared__ int s_i[NT];
    const int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x;
    const bool in = c < n_chains && looked[c];
    double v = 0.0;
    if (in) {
        v = metric[c];
        if (pass == 1) {
            const double d = stats[IAMX_STATS_AVERAGE] - v;
            v = d * d;
        }
    }
    const double t = block_tree(v, s_d);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
    if (pass == 0) {
        const int n = block_tree_int(in ? 1 : 0, s_i);
        if (threadIdx.x == 0) part_n[blockIdx.x] = n;
    }
}

__global__ __launch_bounds__(NT) void stats_final_kernel(const double *__restrict__ part,
                                                         const int32_t *__restrict__ part_n, int64_t n_tiles,
                                                         int pass, double factor, double *__restrict__ stats)
{
    __shared__ double s_d[NT];
    __shared__ double s_n[NT];
    double v = 0.0, n = 0.0;
    for (int64_t t = threadIdx.x; t < n_tiles; t += NT) {
        v = v + part[t];
        if (pass == 0) n = n + (double)part_n[t];                         // (integers: exact in any order)
    }
    const double total = block_tree(v, s_d);
    if (pass == 0) {
        const double cnt = block_tree(n, s_n);
        if (threadIdx.x == 0) {
            stats[IAMX_STATS_N] = cnt;
            stats[IAMX_STATS_AVERAGE] = cnt > 0.0 ? total / cnt : 0.0;
        }
    } else if (threadIdx.x == 0) {
        const double cnt = stats[IAMX_STATS_N];
        const double sd = cnt > 0.0 ? sqrt(total / cnt) : 0.0;
        stats[IAMX_STATS_STDDEV] = sd;
        stats[IAMX_STATS_BAND] = factor * sd;
    }
}

__device__ __forceinline__ bool is_outlier(double metric, const double *__restrict__ stats, int two_sided)
{
    const double avg = stats[IAMX_STATS_AVERAGE], sd = stats[IAMX_STATS_STDDEV], band = stats[IAMX_STATS_BAND];
    if (!(sd > 0.0)) return false;
    return two_sided ? fabs(avg - metric) >= band : metric > avg + band;
}

__global__ __launch_bounds__(NT) void stats_flag_kernel(const double *__restrict__ metric,
                                                        const uint8_t *__restrict__ looked, int64_t n_chains,
                                                        int two_sided, const double *__restrict__ stats,
                                                        uint8_t *__restrict__ flag, int32_t *__restrict__ tile_cnt)
{
    __shared__ int s_i[NT];
    const int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x;
    int f = 0;
    if (c < n_chains) {
        f = looked[c] && is_outlier(metric[c], stats, two_sided) ? 1 : 0;
        flag[c] = (uint8_t)f;
    }
    const int n = block_tree_int(f, s_i);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = n;
}

__global__ __launch_bounds__(NT) void stats_compact_kernel(const double *__restrict__ metric,
                                                           const uint8_t *__restrict__ flag, int64_t n_chains,
                                                           const int64_t *__restrict__ tile_off, int64_t n_tiles,
                                                           int32_t *__restrict__ out_idx,
                                                           double *__restrict__ out_metric,
                                                           int64_t *__restrict__ n_flagged)
{
    __shared__ int s_scan[NT];
    const int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x;
    const int f = c < n_chains ? (int)flag[c] : 0;
    s_scan[threadIdx.x] = f;
    __syncthreads();
    for (int w = 1; w < NT; w <<= 1) {                                    // inclusive scan
        const int add = (int)threadIdx.x >= w ? s_scan[threadIdx.x - w] : 0;
        __syncthreads();
        s_scan[threadIdx.x] += add;
        __syncthreads();
    }
    if (f) {
        const int64_t at = tile_off[blockIdx.x] + s_scan[threadIdx.x] - 1;
        if (at >= 0 && at < n_chains) {
            out_idx[at] = (int32_t)c;
            out_metric[at] = metric[c];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_flagged = tile_off[n_tiles];
}

// ---------------------------------------------------------------------------------------------
// depths
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void depth_obs_kernel(const int64_t *__restrict__ img_ptr,
                                                       const double *__restrict__ ned, int n_images,
                                                       int64_t n_obs, const double *__restrict__ pos,
                                                       double *__restrict__ depth)
{
    const int64_t o = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (o >= n_obs) return;
    const double *p = pos + (int64_t)image_of(img_ptr, n_images, o) * 3;
    const double dx = ned[3 * o] - p[0], dy = ned[3 * o + 1] - p[1], dz = ned[3 * o + 2] - p[2];
    depth[o] = sqrt((dx * dx + dy * dy) + dz * dz);
}

// one workgroup per image: thread t takes observations t, t + NT, ... left to right, then the tree
__global__ __launch_bounds__(NT) void depth_image_kernel(const int64_t *__restrict__ img_ptr,
                                                         const double *__restrict__ depth, int64_t n_obs,
                                                         double *__restrict__ z)
{
    __shared__ double s_d[NT];
    const int im = blockIdx.x;
    int64_t lo = img_ptr[im], hi = img_ptr[im + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_obs ? n_obs : hi;
    const int64_t n = hi > lo ? hi - lo : 0;
    double v = 0.0;
    for (int64_t o = lo + threadIdx.x; o < hi; o += NT) v = v + depth[o];
    const double mean = n > 0 ? block_tree(v, s_d) / (double)n : 0.0;
    v = 0.0;
    for (int64_t o = lo + threadIdx.x; o < hi; o += NT) {
        const double d = depth[o] - mean;
        v = v + d * d;
    }
    const double var = n > 0 ? block_tree(v, s_d) / (double)n : 0.0;
    if (threadIdx.x == 0) {
        z[3 * im] = mean;
        z[3 * im + 1] = sqrt(var);
        z[3 * im + 2] = (double)n;
    }
}

__global__ __launch_bounds__(NT) void depth_chain_kernel(const int64_t *__restrict__ img_ptr, int n_images,
                                                         int64_t n_obs, const double *__restrict__ depth,
                                                         const double *__restrict__ z,
                                                         const int64_t *__restrict__ chain_ptr,
                                                         const int32_t *__restrict__ chain_obs, int64_t n_chains,
                                                         double *__restrict__ metric, uint8_t *__restrict__ looked)
{
    const int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (c >= n_chains) return;
    int64_t b = chain_ptr[c], e = chain_ptr[c + 1];
    if (b < 0 || e > n_obs || e < b) b = e = 0;
    double s = 0.0;
    int64_t n = 0;
    if (e - b >= 2) {
        for (int64_t i = b; i < e; ++i) {
            const int64_t o = chain_obs[i];
            if (o < 0 || o >= n_obs) continue;
            s = s + fabs(depth[o] - z[3 * (int64_t)image_of(img_ptr, n_images, o)]);
            ++n;
        }
    }
    metric[c] = n >= 2 ? s / (double)n : 0.0;
    looked[c] = n >= 2 ? 1 : 0;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + NT - 1) / NT); }

}  // namespace

extern "C" int iamx_surface_knn_fit(const int64_t *img_ptr, const double *uv, const double *ned,
                                    const int32_t *chain, int n_images, int64_t n_obs, int k, int n_pos,
                                    int32_t *tgt, double *val, int32_t *used, double *fit,
                                    int32_t *status, void *stream)
{
    IAMX_REQUIRE(n_images >= 0 && n_obs >= 0, "bad size");
    IAMX_REQUIRE(k >= 1 && k <= MAX_K, "k outside 1..32");
    IAMX_REQUIRE(n_pos >= 1 && n_pos <= MAX_K, "n_pos outside 1..32");
    IAMX_REQUIRE(n_obs * (int64_t)k <= 0x7fffffffLL, "n_obs * k does not fit 31 bits");
    if (n_obs == 0) return IAMX_OK;
    IAMX_REQUIRE(n_images >= 1, "observations without an image");
    IAMX_REQUIRE(img_ptr && uv && ned && chain && tgt && val && used && fit && status, "null pointer");
    const size_t lds = (size_t)k * KNN_QUERIES * (sizeof(double) + sizeof(int32_t)) +
                       2 * KNN_TILE * sizeof(double);
    hipLaunchKernelGGL(surface_knn_fit_kernel, dim3((unsigned)((n_obs + KNN_QUERIES - 1) / KNN_QUERIES)),
                       dim3(KNN_QUERIES), lds, iamx::as_stream(stream), img_ptr, uv, ned, chain, n_images,
                       n_obs, k, n_pos, tgt, val, used, fit, status);
    return iamx::check_launch("iamx_surface_knn_fit");
}

extern "C" int iamx_surface_chain_metric(const int32_t *tgt, const double *val, const int32_t *status,
                                         int64_t n_obs, int k, const uint8_t *looked, int64_t n_chains,
                                         double *sum, int32_t *count, double *metric, int64_t *counters,
                                         int64_t *work_off, int32_t *work_order, void *stream)
{
    IAMX_REQUIRE(n_obs >= 0 && n_chains >= 0, "bad size");
    IAMX_REQUIRE(k >= 1 && k <= MAX_K, "k outside 1..32");
    IAMX_REQUIRE(n_obs * (int64_t)k <= 0x7fffffffLL, "n_obs * k does not fit 31 bits");
    IAMX_REQUIRE(n_chains <= 0x7fffffffLL, "too many chains");
    if (n_chains == 0) return IAMX_OK;
    IAMX_REQUIRE(looked && sum && count && metric && counters, "null pointer");
    hipStream_t st = iamx::as_stream(stream);
    unsigned long long *cnt64 = reinterpret_cast<unsigned long long *>(counters);
    hipError_t e = hipMemsetAsync(counters, 0, IAMX_SURFACE_N_COUNTERS * sizeof(int64_t), st);
    if (e != hipSuccess)
        return iamx::fail(IAMX_ELAUNCH, "iamx_surface_chain_metric: clearing the counters: %s", hipGetErrorString(e));
    if (n_obs == 0) {
        hipLaunchKernelGGL(metric_zero_kernel, dim3(blocks_of(n_chains)), dim3(NT), 0, st, n_chains, looked,
                           sum, count, metric, cnt64);
        return iamx::check_launch("iamx_surface_chain_metric");
    }
    IAMX_REQUIRE(tgt && val && status && work_off && work_order, "null pointer");
    const int64_t n_slots = n_obs * k;
    e = hipMemsetAsync(count, 0, n_chains * sizeof(int32_t), st);
    if (e != hipSuccess)
        return iamx::fail(IAMX_ELAUNCH, "iamx_surface_chain_metric: clearing the counts: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(status_count_kernel, dim3(blocks_of(n_obs)), dim3(NT), 0, st, status, n_obs, cnt64);
    hipLaunchKernelGGL(metric_count_kernel, dim3(blocks_of(n_slots)), dim3(NT), 0, st, tgt, n_slots, n_chains,
                       count);
    int rc = iamx::check_launch("iamx_surface_chain_metric");
    if (rc != IAMX_OK) return rc;
    rc = iamx_exclusive_scan_i32(count, n_chains, work_off, stream);
    if (rc != IAMX_OK) return rc;
    // the counts serve as the fill's cursors and end where they were
    e = hipMemsetAsync(count, 0, n_chains * sizeof(int32_t), st);
    if (e != hipSuccess)
        return iamx::fail(IAMX_ELAUNCH, "iamx_surface_chain_metric: clearing the cursors: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(metric_fill_kernel, dim3(blocks_of(n_slots)), dim3(NT), 0, st, tgt, n_slots, n_chains,
                       (const int64_t *)work_off, count, work_order);
    hipLaunchKernelGGL(metric_sum_kernel, dim3(blocks_of(n_chains)), dim3(NT), 0, st, val, n_slots, n_chains,
                       (const int64_t *)work_off, work_order, looked, sum, (const int32_t *)count, metric, cnt64);
    return iamx::check_launch("iamx_surface_chain_metric");
}

extern "C" int iamx_chain_outlier_stats(const double *metric, const uint8_t *looked, int64_t n_chains,
                                        double factor, int two_sided, double *stats, uint8_t *flag,
                                        int32_t *out_idx, double *out_metric, int64_t *n_flagged,
                                        double *work_part, int32_t *work_cnt, int64_t *work_off, void *stream)
{
    IAMX_REQUIRE(n_chains >= 0 && n_chains <= 0x7fffffffLL, "bad size");
    IAMX_REQUIRE(factor == factor, "factor is NaN");
    if (n_chains == 0) return IAMX_OK;
    IAMX_REQUIRE(metric && looked && stats && flag && out_idx && out_metric && n_flagged && work_part &&
                     work_cnt && work_off,
                 "null pointer");
    hipStream_t st = iamx::as_stream(stream);
    const int64_t n_tiles = (n_chains + NT - 1) / NT;
    const dim3 grid((unsigned)n_tiles), one(1), block(NT);
    hipLaunchKernelGGL(stats_tile_kernel, grid, block, 0, st, metric, looked, n_chains, 0, (const double *)stats,
                       work_part, work_cnt);
    hipLaunchKernelGGL(stats_final_kernel, one, block, 0, st, (const double *)work_part,
                       (const int32_t *)work_cnt, n_tiles, 0, factor, stats);
    hipLaunchKernelGGL(stats_tile_kernel, grid, block, 0, st, metric, looked, n_chains, 1, (const double *)stats,
                       work_part, work_cnt);
    hipLaunchKernelGGL(stats_final_kernel, one, block, 0, st, (const double *)work_part,
                       (const int32_t *)work_cnt, n_tiles, 1, factor, stats);
    hipLaunchKernelGGL(stats_flag_kernel, grid, block, 0, st, metric, looked, n_chains, two_sided,
                       (const double *)stats, flag, work_cnt);
    int rc = iamx::check_launch("iamx_chain_outlier_stats");
    if (rc != IAMX_OK) return rc;
    rc = iamx_exclusive_scan_i32(work_cnt, n_tiles, work_off, stream);
    if (rc != IAMX_OK) return rc;
    hipLaunchKernelGGL(stats_compact_kernel, grid, block, 0, st, metric, (const uint8_t *)flag, n_chains,
                       (const int64_t *)work_off, n_tiles, out_idx, out_metric, n_flagged);
    return iamx::check_launch("iamx_chain_outlier_stats");
}

extern "C" int iamx_chain_depths(const int64_t *img_ptr, const double *ned, int n_images, int64_t n_obs,
                                 const double *pos, const int64_t *chain_ptr, const int32_t *chain_obs,
                                 int64_t n_chains, double *depth, double *z, double *metric,
                                 uint8_t *looked, void *stream)
{
    IAMX_REQUIRE(n_images >= 0 && n_obs >= 0 && n_chains >= 0, "bad size");
    IAMX_REQUIRE(n_obs <= 0x7fffffffLL && n_chains <= 0x7fffffffLL, "too many observations or chains");
    IAMX_REQUIRE(n_obs == 0 || n_images >= 1, "observations without an image");
    if (n_images == 0 && n_chains == 0) return IAMX_OK;
    IAMX_REQUIRE(n_images == 0 || (img_ptr && z), "null pointer");
    IAMX_REQUIRE(n_obs == 0 || (ned && pos && depth && chain_obs), "null pointer");
    IAMX_REQUIRE(n_chains == 0 || (chain_ptr && metric && looked), "null pointer");
    hipStream_t st = iamx::as_stream(stream);
    if (n_obs)
        hipLaunchKernelGGL(depth_obs_kernel, dim3(blocks_of(n_obs)), dim3(NT), 0, st, img_ptr, ned, n_images,
                           n_obs, pos, depth);
    if (n_images)
        hipLaunchKernelGGL(depth_image_kernel, dim3((unsigned)n_images), dim3(NT), 0, st, img_ptr,
                           (const double *)depth, n_obs, z);
    if (n_chains)
        hipLaunchKernelGGL(depth_chain_kernel, dim3(blocks_of(n_chains)), dim3(NT), 0, st, img_ptr, n_images,
                           n_obs, (const double *)depth, (const double *)z, chain_ptr, chain_obs, n_chains,
                           metric, looked);
    return iamx::check_launch("iamx_chain_depths");
}
