// Dense surface, coarse to fine (gfx950): the window table of the guided sweep (iamx_dense_sweep_guided,
// csrc/dense_sweep.hip) from a coarse depth map.  The rules are dense.py's REFINEMENT RULES ("Guide"),
// restated in numpy by tests/dense_refine_restatement.py; integers and float64 only, every operation rounded
// on its own (the pragma below), and a minimum and a maximum, which do not depend on the order they are
// taken in.
//
// guide_kernel: one workgroup of 256 threads per tile of the fine image.  The tile's box of coarse pixels
// is walked with a stride of 256, each thread keeping the smallest and the largest inverse depth of its
// finite, positive entries; the 256 pairs meet in LDS by a tree of 8 halvings, and thread 0 turns them into
// (first, count).  A thread without an entry carries (+inf, -inf), which loses every comparison; the box
// held none iff the minimum is still +inf.  No atomics.
#include <math.h>

#include "iamx_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int TILE_W = IAMX_DENSE_TILE_W;
constexpr int TILE_H = IAMX_DENSE_TILE_H;

struct GuideArgs {
    const float *coarse;         // [hc][wc], NaN: none
    int wc, hc, w, h;
    int tiles_x, tiles_y;
    double w_far, step;
    int total, radius, pad;
    int32_t *windows;            // [tiles_y][tiles_x][2]
};

// the coarse pixels that the fine pixels a0 .. a1 (of n) fall into, one more either side, inside 0 .. nc - 1
__device__ __forceinline__ void coarse_span(int a0, int a1, int n, int nc, int &c0, int &c1)
{
    c0 = max((int)(((int64_t)(2 * a0 + 1) * nc) / (2 * (int64_t)n)) - 1, 0);
    c1 = min((int)(((int64_t)(2 * a1 + 1) * nc) / (2 * (int64_t)n)) + 1, nc - 1);
}

__global__ __launch_bounds__(THREADS) void guide_kernel(GuideArgs A)
{
    __shared__ double s_min[THREADS], s_max[THREADS];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x, ty = blockIdx.y;
    const int x0 = max(TILE_W * tx - A.radius, 0), x1 = min(TILE_W * tx + TILE_W - 1 + A.radius, A.w - 1);
    const int y0 = max(TILE_H * ty - A.radius, 0), y1 = min(TILE_H * ty + TILE_H - 1 + A.radius, A.h - 1);
    int c0, c1, r0, r1;
    coarse_span(x0, x1, A.w, A.wc, c0, c1);
    coarse_span(y0, y1, A.h, A.hc, r0, r1);
    const int bw = c1 - c0 + 1, bh = r1 - r0 + 1;          // (both at least 1: c0 <= c1 by construction)
    const int64_t cells = (int64_t)bw * bh;

    double wmin = INFINITY, wmax = -INFINITY;
    for (int64_t i = tid; i < cells; i += THREADS) {
        const int by = (int)(i / bw), bx = (int)(i - (int64_t)by * bw);
        const float z = A.coarse[(int64_t)(r0 + by) * A.wc + (c0 + bx)];
        if (z > 0.0f && z < INFINITY) {                     // (a NaN fails both)
            const double wv = 1.0 / (double)z;
            wmin = wv < wmin ? wv : wmin;
            wmax = wv > wmax ? wv : wmax;
        }
    }
    s_min[tid] = wmin;
    s_max[tid] = wmax;
    __syncthreads();
    for (int half = THREADS / 2; half > 0; half >>= 1) {
        if (tid < half) {
            const double a = s_min[tid + half], b = s_max[tid + half];
            if (a < s_min[tid]) s_min[tid] = a;
            if (b > s_max[tid]) s_max[tid] = b;
        }
        __syncthreads();
    }
    if (tid != 0) return;
    int first = 0, count = 0;
    wmin = s_min[0];
    wmax = s_max[0];
    if (wmin < INFINITY) {
        // floor and ceil are whole doubles; the pad and the clamp stay in doubles, where nothing
        // overflows, and are exact wherever the integers of the rule are
        const double last = (double)(A.total - 1);
        double lo = floor((wmin - A.w_far) / A.step) - (double)A.pad;
        double hi = ceil((wmax - A.w_far) / A.step) + (double)A.pad;
        lo = lo < 0.0 ? 0.0 : (lo > last ? last : lo);
        hi = hi < 0.0 ? 0.0 : (hi > last ? last : hi);
        first = (int)lo;
        count = (int)hi - first + 1;
    }
    int32_t *e = A.windows + 2 * ((int64_t)ty * A.tiles_x + tx);
    e[0] = first;
    e[1] = count;
}

}  // namespace

extern "C" int iamx_dense_guide(const float *coarse_depth, int wc, int hc, int width, int height, double w_far,
                                double w_near, int planes_total, int radius, int pad, int32_t *windows, void *stream)
{
    IAMX_REQUIRE(planes_total >= 2 && planes_total <= IAMX_DENSE_GUIDED_MAX_PLANES, "planes_total out of range");
    IAMX_REQUIRE(radius >= 1 && radius <= IAMX_DENSE_MAX_RADIUS, "radius out of range");
    IAMX_REQUIRE(pad >= 0 && pad <= IAMX_DENSE_GUIDED_MAX_PLANES, "pad out of range");
    IAMX_REQUIRE(width >= 1 && height >= 1 && width <= IAMX_DENSE_MAX_SIDE && height <= IAMX_DENSE_MAX_SIDE,
                 "image size out of range");
    IAMX_REQUIRE(wc >= 1 && hc >= 1 && wc <= IAMX_DENSE_MAX_SIDE && hc <= IAMX_DENSE_MAX_SIDE,
                 "coarse image size out of range");
    IAMX_REQUIRE(w_far > 0.0 && w_near > w_far && w_near < INFINITY, "0 < w_far < w_near wanted");
    IAMX_REQUIRE(coarse_depth && windows, "null pointer");
    GuideArgs A;
    A.coarse = coarse_depth;
    A.wc = wc; A.hc = hc; A.w = width; A.h = height;
    A.tiles_x = (width + TILE_W - 1) / TILE_W;
    A.tiles_y = (height + TILE_H - 1) / TILE_H;
    A.w_far = w_far;
    A.step = (w_near - w_far) / (double)(planes_total - 1);
    A.total = planes_total; A.radius = radius; A.pad = pad;
    A.windows = windows;
    hipLaunchKernelGGL(guide_kernel, dim3(A.tiles_x, A.tiles_y), dim3(THREADS), 0, iamx::as_stream(stream), A);
    return iamx::check_launch("iamx_dense_guide");
}
