// Dense surface (gfx950): robust DSM fusion from per-cell height histograms.  The rules are stated in
// imageanalysis_amd/dense.py's docstring ("ROBUST FUSION RULES") and restated in numpy by
// tests/dense_fuse_restatement.py; this file follows them operation by operation.  The only floating
// point is the splat's: the cell and q = rint(up 1024) of a point, each operation rounded on its own
// (the pragma below switches contraction off for the whole file, as csrc/dense_sweep.hip does).
// Everything behind q is int64, and every cell value is a minimum, a maximum or a count kept by
// integer atomics, so the result does not depend on scheduling or on the order of the points.
//
// range_kernel, hist_kernel, sum_kernel: one thread per point, the splat's 25 bytes read per point
// (24 of ned, 1 of keep).  A point's acceptance (keep, the cell inside the raster, |q| <= 1e15) is
// evaluated by one function in all three, so the three agree on it by construction.
//
// select_kernel: a workgroup of 128 threads owns 128 consecutive cells.  Their histograms are 128 bins
// consecutive dwords: every thread loads them with consecutive dword addresses across the wave, puts
// them into LDS and stores the zeroes of the next level over them with the same addresses, so both
// directions are whole 256-byte wave accesses.  Thread i then walks cell i's bins in LDS, serially, as
// the rule reads.  The LDS pitch is bins | 1 dwords: odd, so the 64 lanes of a wave, each at the same
// bin of its own cell, fall on 64 different banks.  (One thread per cell reading its bins from global
// memory makes every load instruction touch 64 lines, 4 bins bytes apart; a wave per cell with a bin
// per lane leaves lanes idle below 64 bins, needs cross-lane steps for the three-bin sums and starts a
// wave for 4 bins bytes.  DESIGN section 4.)  A workgroup none of whose cells holds a point leaves at
// once: its histograms were never added to.
#include <math.h>

#include "iamx_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;                              // the point passes
constexpr int CELLS = 128;                                // the select: cells, and threads, per workgroup
constexpr int MAX_BINS = IAMX_DENSE_FUSE_MAX_BINS;        // 64
constexpr int MAX_PITCH = MAX_BINS | 1;

struct Frame {
    double x0, y1, gsd;
    int W, H;
};

// the splat's acceptance of point g -> its cell and q; false: the point takes no part
__device__ __forceinline__ bool accept(const double *__restrict__ ned, const uint8_t *__restrict__ keep, int64_t g,
                                       const Frame &F, int64_t &cell, int64_t &q)
{
    if (keep && !keep[g]) return false;
    const double north = ned[3 * g], east = ned[3 * g + 1], up = -ned[3 * g + 2];
    const double r = floor((F.y1 - north) / F.gsd), c = floor((east - F.x0) / F.gsd);
    const double qd = rint(up * 1024.0);
    if (!(r >= 0.0 && r <= (double)(F.H - 1) && c >= 0.0 && c <= (double)(F.W - 1))) return false;
    if (!(fabs(qd) <= 1e15)) return false;                // (NaN too)
    cell = (int64_t)r * F.W + (int64_t)c;
    q = (int64_t)qd;
    return true;
}

// the bin width of a window: max(wmin, ceil((hi - lo + 1) / bins)); hi - lo + 1 <= 2e15 + 1
__device__ __forceinline__ int64_t bin_width(int64_t lo, int64_t hi, int bins, int64_t wmin)
{
    const int64_t w = (hi - lo + bins) / bins;            // = ceil((hi - lo + 1) / bins), hi >= lo
    return w > wmin ? w : wmin;
}

__global__ __launch_bounds__(THREADS) void range_kernel(const double *__restrict__ ned, const uint8_t *__restrict__ keep,
                                                        int64_t n, Frame F, int32_t *__restrict__ count,
                                                        int64_t *__restrict__ window)
{
    const int64_t g = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (g >= n) return;
    int64_t cell, q;
    if (!accept(ned, keep, g, F, cell, q)) return;
    atomicAdd(reinterpret_cast<int *>(count + cell), 1);
    atomicMin(reinterpret_cast<long long *>(window + 2 * cell), (long long)q);
    atomicMax(reinterpret_cast<long long *>(window + 2 * cell + 1), (long long)q);
}

__global__ __launch_bounds__(THREADS) void hist_kernel(const double *__restrict__ ned, const uint8_t *__restrict__ keep,
                                                       int64_t n, Frame F, const int64_t *__restrict__ window, int bins,
                                                       int64_t wmin, uint32_t *__restrict__ hist)
{
    const int64_t g = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (g >= n) return;
    int64_t cell, q;
    if (!accept(ned, keep, g, F, cell, q)) return;
    const int64_t lo = window[2 * cell], hi = window[2 * cell + 1];
    if (q < lo || q > hi) return;
    const int64_t b = (q - lo) / bin_width(lo, hi, bins, wmin);     // < bins: (hi - lo) / wb <= bins - 1
    if (b >= bins) return;                                // (a window that is not these points': nothing is written)
    atomicAdd(hist + cell * bins + b, 1u);
}

__global__ __launch_bounds__(CELLS) void select_kernel(const int32_t *__restrict__ count, int64_t cells, int bins,
                                                       int64_t wmin, int t, uint32_t *__restrict__ hist,
                                                       int64_t *__restrict__ window)
{
    __shared__ uint32_t tile[CELLS * MAX_PITCH];
    const int tid = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * CELLS;
    const int here = (int)(cells - first < CELLS ? cells - first : CELLS);
    const int32_t mine = tid < here ? count[first + tid] : 0;
    if (!__syncthreads_or(mine > 0)) {                    // nothing landed in these cells: hist is zero as it is
        if (tid < here) window[2 * (first + tid)] = 0, window[2 * (first + tid) + 1] = 0;
        return;
    }
    const int pitch = bins | 1;
    uint32_t *__restrict__ h = hist + first * bins;
    for (int i = tid; i < here * bins; i += CELLS) {
        tile[(i / bins) * pitch + i % bins] = h[i];
        h[i] = 0;
    }
    __syncthreads();
    if (tid >= here) return;
    int64_t *__restrict__ win = window + 2 * (first + tid);
    if (mine <= 0) {
        win[0] = 0;
        win[1] = 0;
        return;
    }
    const uint32_t *__restrict__ hb = tile + tid * pitch;
    // s_b = hist[b - 1] + hist[b] + hist[b + 1] as a sliding sum of uint64 (three counts of < 2^32)
    uint64_t smax = 0;
    {
        uint64_t prev = 0, cur = hb[0];
        for (int b = 0; b < bins; ++b) {
            const uint64_t next = b + 1 < bins ? hb[b + 1] : 0;
            const uint64_t s = prev + cur + next;
            smax = s > smax ? s : smax;
            prev = cur;
            cur = next;
        }
    }
    int best = 0;                                         // the HIGHEST b with s_b 256 >= t smax (smax >= 1: one exists)
    {
        uint64_t prev = 0, cur = hb[0];
        const uint64_t need = (uint64_t)t * smax;
        for (int b = 0; b < bins; ++b) {
            const uint64_t next = b + 1 < bins ? hb[b + 1] : 0;
            if ((prev + cur + next) * 256 >= need) best = b;
            prev = cur;
            cur = next;
        }
    }
    const int64_t lo = win[0], hi = win[1];
    const int64_t wb = bin_width(lo, hi, bins, wmin);
    const int64_t lo2 = lo + (int64_t)(best - 1) * wb, hi2 = lo + (int64_t)(best + 2) * wb - 1;   // (both from the OLD lo)
    win[0] = lo2 > lo ? lo2 : lo;
    win[1] = hi2 < hi ? hi2 : hi;
}

__global__ __launch_bounds__(THREADS) void sum_kernel(const double *__restrict__ ned, const uint8_t *__restrict__ keep,
                                                      int64_t n, Frame F, const int64_t *__restrict__ window,
                                                      int32_t *__restrict__ support, int64_t *__restrict__ sum)
{
    const int64_t g = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (g >= n) return;
    int64_t cell, q;
    if (!accept(ned, keep, g, F, cell, q)) return;
    if (q < window[2 * cell] || q > window[2 * cell + 1]) return;
    atomicAdd(reinterpret_cast<int *>(support + cell), 1);
    atomicAdd(reinterpret_cast<unsigned long long *>(sum + cell), (unsigned long long)(long long)q);
}

}  // namespace

// the arguments every point pass shares (the splat's checks)
#define IAMX_FUSE_POINTS(num_points, width, height, x0, y1, gsd)                                                       \
    do {                                                                                                               \
        IAMX_REQUIRE(num_points >= 0 && num_points < ((int64_t)1 << 31) * THREADS, "bad point count");                 \
        IAMX_REQUIRE(width >= 1 && height >= 1 && width <= IAMX_DENSE_MAX_RASTER && height <= IAMX_DENSE_MAX_RASTER,   \
                     "raster size out of range");                                                                      \
        IAMX_REQUIRE(gsd > 0.0 && gsd < INFINITY && x0 == x0 && y1 == y1, "bad raster frame");                         \
    } while (0)

#define IAMX_FUSE_BINS(bins, wmin)                                                                                     \
    do {                                                                                                               \
        IAMX_REQUIRE(bins >= IAMX_DENSE_FUSE_MIN_BINS && bins <= IAMX_DENSE_FUSE_MAX_BINS, "bins out of range");       \
        IAMX_REQUIRE(wmin >= 1 && wmin <= ((int64_t)1 << 40), "the least bin width is 1 to 2^40");                     \
    } while (0)

static unsigned point_blocks(int64_t n) { return (unsigned)((n + THREADS - 1) / THREADS); }

extern "C" int iamx_dense_fuse_range(const double *ned, const uint8_t *keep, int64_t num_points, double x0, double y1,
                                     double gsd, int width, int height, int32_t *count, int64_t *window, void *stream)
{
    IAMX_FUSE_POINTS(num_points, width, height, x0, y1, gsd);
    if (num_points == 0) return IAMX_OK;
    IAMX_REQUIRE(ned && count && window, "null pointer");
    const Frame F = {x0, y1, gsd, width, height};
    hipLaunchKernelGGL(range_kernel, dim3(point_blocks(num_points)), dim3(THREADS), 0, iamx::as_stream(stream), ned, keep,
                       num_points, F, count, window);
    return iamx::check_launch("iamx_dense_fuse_range");
}

extern "C" int iamx_dense_fuse_hist(const double *ned, const uint8_t *keep, int64_t num_points, double x0, double y1,
                                    double gsd, int width, int height, const int64_t *window, int bins, int64_t wmin,
                                    uint32_t *hist, void *stream)
{
    IAMX_FUSE_POINTS(num_points, width, height, x0, y1, gsd);
    IAMX_FUSE_BINS(bins, wmin);
    if (num_points == 0) return IAMX_OK;
    IAMX_REQUIRE(ned && window && hist, "null pointer");
    const Frame F = {x0, y1, gsd, width, height};
    hipLaunchKernelGGL(hist_kernel, dim3(point_blocks(num_points)), dim3(THREADS), 0, iamx::as_stream(stream), ned, keep,
                       num_points, F, window, bins, wmin, hist);
    return iamx::check_launch("iamx_dense_fuse_hist");
}

extern "C" int iamx_dense_fuse_select(const int32_t *count, int width, int height, int bins, int64_t wmin, int share,
                                      uint32_t *hist, int64_t *window, void *stream)
{
    IAMX_REQUIRE(width >= 1 && height >= 1 && width <= IAMX_DENSE_MAX_RASTER && height <= IAMX_DENSE_MAX_RASTER,
                 "raster size out of range");
    IAMX_FUSE_BINS(bins, wmin);
    IAMX_REQUIRE(share >= 1 && share <= 256, "share is 1 to 256");
    IAMX_REQUIRE(count && hist && window, "null pointer");
    const int64_t cells = (int64_t)width * height;
    IAMX_REQUIRE(cells < ((int64_t)1 << 31) * CELLS, "too many cells for one call");
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)((cells + CELLS - 1) / CELLS)), dim3(CELLS), 0,
                       iamx::as_stream(stream), count, cells, bins, wmin, share, hist, window);
    return iamx::check_launch("iamx_dense_fuse_select");
}

extern "C" int iamx_dense_fuse_sum(const double *ned, const uint8_t *keep, int64_t num_points, double x0, double y1,
                                   double gsd, int width, int height, const int64_t *window, int32_t *support,
                                   int64_t *sum, void *stream)
{
    IAMX_FUSE_POINTS(num_points, width, height, x0, y1, gsd);
    if (num_points == 0) return IAMX_OK;
    IAMX_REQUIRE(ned && window && support && sum, "null pointer");
    const Frame F = {x0, y1, gsd, width, height};
    hipLaunchKernelGGL(sum_kernel, dim3(point_blocks(num_points)), dim3(THREADS), 0, iamx::as_stream(stream), ned, keep,
                       num_points, F, window, support, sum);
    return iamx::check_launch("iamx_dense_fuse_sum");
}
