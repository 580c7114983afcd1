// Dense surface (gfx950): semi-global aggregation of the plane sweep's cost volume and the winner
// taken from it.  The rules are stated in imageanalysis_amd/dense.py's docstring ("SEMI-GLOBAL RULES")
// and restated in numpy by tests/dense_sgm_restatement.py; this file follows them bit for bit.  All of
// the aggregation is integer arithmetic, the two float32 operations of select are rounded on their own
// (the pragma below).
//
// sgm_path_kernel<ADD>: one launch per direction, one workgroup of one wave per path, lane = plane.
// The wave walks its path from the image's edge; per step
//   load       the lane's cost byte (and, ADD, its uint16 of total) -- these do not depend on the
//              recurrence, so they sit in a ring of U registers: a step takes its slot and at once asks
//              for the step U further on; no wait in the loop is for a load or a store younger than that;
//   neighbours L(d - 1) and L(d + 1) by v_mov_b32_dpp wave_shr:1 / wave_shl:1, the lane without one
//              receives BIG;
//   minimum    m of the step's L by four DPP butterflies inside the rows of 16 lanes (quad_perm,
//              quad_perm, row_half_mirror, row_mirror), four v_readlane and three s_min: m is in an
//              SGPR, no LDS;
//   store      total (p, d) (+)= L.  Within a launch every (p, d) has one owner: plain uint16
//              read-modify-write, no atomics.  The first direction of iamx_dense_sgm_paths stores
//              without reading, which is its zeroing: a caller's stale buffer cannot leak in.
// Lanes >= planes carry the cost BIG, so their L stays in [BIG, BIG + P2] and never wins a minimum.
// L starts as 0 with m = 0: the recurrence then yields C' at the path's first pixel, as the rule asks.
//
// sgm_select_kernel: one wave per pixel, lane = plane; argmin of T 64 + d by the same reduction (the
// smallest plane on a tie), lane 0 finishes the pixel.
#include <math.h>

#include "iamx_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int WAVE = 64;
constexpr int MAX_PLANES = IAMX_DENSE_SGM_MAX_PLANES;   // 64
constexpr int BIG = 1 << 20;
constexpr int U = 16;                                    // steps whose loads are in flight ahead of their use

static_assert(MAX_PLANES == WAVE, "lane = plane");
// L_r <= 254 + P2 <= 509 and T = sum over at most 8 directions <= 4072: a uint16 holds it, and
// T 64 + d < 2^31 is select's key
static_assert(8 * (254 + 255) == 4072 && 4072 <= 65535, "total fits a uint16");
static_assert(BIG > 509 + 255 && BIG + 255 + 255 < (1 << 30), "BIG never wins and never overflows");

template <int CTRL>
__device__ __forceinline__ int dpp(int old, int v)
{
    return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xf, 0xf, false);
}

// the minimum over the wave's 64 lanes, wave-uniform (every lane active).  `old` of the butterflies is
// the minimum's identity, which lets the compiler fold each move into a v_min_i32_dpp
__device__ __forceinline__ int wave_min(int v)
{
    constexpr int TOP = 0x7fffffff;
    v = min(v, dpp<0xb1>(TOP, v));    // quad_perm:[1,0,3,2]
    v = min(v, dpp<0x4e>(TOP, v));    // quad_perm:[2,3,0,1]
    v = min(v, dpp<0x141>(TOP, v));   // row_half_mirror
    v = min(v, dpp<0x140>(TOP, v));   // row_mirror: every lane holds its row's minimum
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

struct PathArgs {
    const uint8_t *volume;       // [h][w][planes]
    uint16_t *total;             // [h][w][planes]
    int w, h, planes;
    int dx, dy;
    int p1, p2, c_invalid;
};

// the paths of a direction: |dy| = 0: one per row; |dx| = 0: one per column; a diagonal: one from
// every pixel of the row it leaves (w of them), then one from every other pixel of the column it leaves
__device__ __forceinline__ void path_start(const PathArgs &A, int k, int &x0, int &y0, int &len)
{
    const int w = A.w, h = A.h, dx = A.dx, dy = A.dy;
    if (dy == 0) {
        x0 = dx > 0 ? 0 : w - 1; y0 = k; len = w;
    } else if (dx == 0) {
        x0 = k; y0 = dy > 0 ? 0 : h - 1; len = h;
    } else {
        if (k < w) {
            x0 = k; y0 = dy > 0 ? 0 : h - 1;
        } else {
            const int j = k - w + 1;                         // 1 .. h - 1
            x0 = dx > 0 ? 0 : w - 1; y0 = dy > 0 ? j : h - 1 - j;
        }
        len = min(dx > 0 ? w - x0 : x0 + 1, dy > 0 ? h - y0 : y0 + 1);
    }
}

template <bool ADD>
__global__ __launch_bounds__(WAVE) void sgm_path_kernel(PathArgs A)
{
    const int lane = threadIdx.x;
    int x0, y0, len;
    path_start(A, blockIdx.x, x0, y0, len);
    const bool act = lane < A.planes;
    const int64_t stride = ((int64_t)A.dy * A.w + A.dx) * A.planes;
    const int64_t first = ((int64_t)y0 * A.w + x0) * A.planes + (act ? lane : 0);   // (an idle lane reads plane 0)
    const uint8_t *__restrict__ vp = A.volume + first;
    uint16_t *__restrict__ tp = A.total + first;
    const int p1 = A.p1, p2 = A.p2, cinv = A.c_invalid;

    int c[U], t[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
        const int64_t o = stride * min(j, len - 1);          // (past the end: the last step's again, never used)
        c[j] = vp[o];
        t[j] = ADD ? tp[o] : 0;
    }
    int L = 0, m = 0;
    auto step = [&](int cj, int tj, int64_t i) {
        int cost = cj == 255 ? cinv : cj;
        cost = act ? cost : BIG;
        const int lo = dpp<0x138>(BIG, L);                   // wave_shr:1, lane d receives L(d - 1)
        const int hi = dpp<0x130>(BIG, L);                   // wave_shl:1, lane d receives L(d + 1)
        const int best = min(min(L, min(lo, hi) + p1), m + p2);
        L = cost + (best - m);
        m = wave_min(L);
        if (act) tp[stride * i] = (uint16_t)(tj + L);
    };
    // a ring of U registers: a step takes its slot's values and at once asks for those of the step U
    // further on, so no point of the loop waits for anything younger than U steps -- the stores included
    int base = 0;
    for (; base + U <= len; base += U) {
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const int cj = c[j], tj = t[j];
            const int64_t o = stride * min(base + j + U, len - 1);
            c[j] = vp[o];
            t[j] = ADD ? tp[o] : 0;
            step(cj, tj, base + j);
        }
    }
    // the last len - base < U steps sit in the ring already
#pragma unroll
    for (int j = 0; j < U; ++j)
        if (base + j < len) step(c[j], t[j], base + j);      // (wave-uniform)
}

struct SelectArgs {
    const uint16_t *total;       // [h][w][planes]
    const uint8_t *volume;       // [h][w][planes]
    int64_t pixels;
    int planes;
    double w_far, step;
    int max_cost;
    int32_t *plane;              // [h][w]
    uint8_t *cost;               // [h][w]
    uint16_t *tot0;              // [h][w]
    float *depth;                // [h][w]
};

constexpr int SELECT_THREADS = 256;

__global__ __launch_bounds__(SELECT_THREADS) void sgm_select_kernel(SelectArgs A)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t p = (int64_t)blockIdx.x * (SELECT_THREADS / WAVE) + (threadIdx.x >> 6);
    if (p >= A.pixels) return;                               // (wave-uniform)
    const uint16_t *__restrict__ T = A.total + p * A.planes;
    int key = 0x7fffffff;
    if (lane < A.planes) key = (int)T[lane] * WAVE + lane;
    key = wave_min(key);
    if (lane != 0) return;
    const int best = key & (WAVE - 1), t0 = key >> 6;
    float off = 0.0f;
    if (best > 0 && best < A.planes - 1) {
        const int tm = T[best - 1], tpl = T[best + 1];
        const int den = (tm - 2 * t0) + tpl;
        if (den > 0) {
            off = (float)(tm - tpl) / (float)(2 * den);
            off = off < -0.5f ? -0.5f : (off > 0.5f ? 0.5f : off);
        }
    }
    const int raw = A.volume[p * A.planes + best];
    float depth = __int_as_float(0x7fc00000);
    if (raw <= A.max_cost)
        depth = (float)(1.0 / (A.w_far + ((double)best + (double)off) * A.step));
    A.plane[p] = best;
    A.cost[p] = (uint8_t)raw;
    A.tot0[p] = (uint16_t)t0;
    A.depth[p] = depth;
}

int check_volume_args(const void *volume, int width, int height, int planes)
{
    IAMX_REQUIRE(planes >= 2 && planes <= MAX_PLANES, "planes out of range");
    IAMX_REQUIRE(width >= 1 && height >= 1 && width <= IAMX_DENSE_MAX_SIDE && height <= IAMX_DENSE_MAX_SIDE,
                 "image size out of range");
    IAMX_REQUIRE(volume, "null pointer");
    return IAMX_OK;
}

int launch_direction(const uint8_t *volume, int width, int height, int planes, int direction, int accumulate, int p1,
                     int p2, int c_invalid, uint16_t *total, void *stream)
{
    PathArgs A;
    A.volume = volume; A.total = total;
    A.w = width; A.h = height; A.planes = planes;
    // the directions of SEMI-GLOBAL RULES, in their order
    static const int dxs[8] = {1, -1, 0, 0, 1, -1, 1, -1}, dys[8] = {0, 0, 1, -1, 1, -1, -1, 1};
    A.dx = dxs[direction]; A.dy = dys[direction];
    A.p1 = p1; A.p2 = p2; A.c_invalid = c_invalid;
    const int n = A.dy == 0 ? height : (A.dx == 0 ? width : width + height - 1);
    if (accumulate)
        hipLaunchKernelGGL(sgm_path_kernel<true>, dim3(n), dim3(WAVE), 0, iamx::as_stream(stream), A);
    else
        hipLaunchKernelGGL(sgm_path_kernel<false>, dim3(n), dim3(WAVE), 0, iamx::as_stream(stream), A);
    return iamx::check_launch("iamx_dense_sgm_direction");
}

}  // namespace

extern "C" int iamx_dense_sgm_direction(const uint8_t *volume, int width, int height, int planes, int direction,
                                        int accumulate, int p1, int p2, int c_invalid, uint16_t *total, void *stream)
{
    if (int rc = check_volume_args(volume, width, height, planes)) return rc;
    IAMX_REQUIRE(direction >= 0 && direction < 8, "direction is 0 .. 7");
    IAMX_REQUIRE(p1 >= 0 && p1 <= p2 && p2 <= 255, "0 <= P1 <= P2 <= 255 wanted");
    IAMX_REQUIRE(c_invalid >= 0 && c_invalid <= 254, "c_invalid is 0 .. 254");
    IAMX_REQUIRE(total, "null pointer");
    return launch_direction(volume, width, height, planes, direction, accumulate != 0, p1, p2, c_invalid, total, stream);
}

extern "C" int iamx_dense_sgm_paths(const uint8_t *volume, int width, int height, int planes, int paths, int p1, int p2,
                                    int c_invalid, uint16_t *total, void *stream)
{
    if (int rc = check_volume_args(volume, width, height, planes)) return rc;
    IAMX_REQUIRE(paths == 4 || paths == 8, "paths is 4 or 8");
    IAMX_REQUIRE(p1 >= 0 && p1 <= p2 && p2 <= 255, "0 <= P1 <= P2 <= 255 wanted");
    IAMX_REQUIRE(c_invalid >= 0 && c_invalid <= 254, "c_invalid is 0 .. 254");
    IAMX_REQUIRE(total, "null pointer");
    for (int r = 0; r < paths; ++r)
        if (int rc = launch_direction(volume, width, height, planes, r, r > 0, p1, p2, c_invalid, total, stream)) return rc;
    return IAMX_OK;
}

extern "C" int iamx_dense_sgm_select(const uint16_t *total, const uint8_t *volume, int width, int height, int planes,
                                     double w_far, double step, int max_cost, int32_t *plane, uint8_t *cost,
                                     uint16_t *tot0, float *depth, void *stream)
{
    if (int rc = check_volume_args(volume, width, height, planes)) return rc;
    IAMX_REQUIRE(w_far > 0.0 && step > 0.0 && step < INFINITY, "0 < w_far and 0 < step wanted");
    IAMX_REQUIRE(max_cost >= 0 && max_cost <= 254, "max_cost is 0 .. 254");
    IAMX_REQUIRE(total && plane && cost && tot0 && depth, "null pointer");
    SelectArgs A;
    A.total = total; A.volume = volume;
    A.pixels = (int64_t)width * height;
    A.planes = planes; A.w_far = w_far; A.step = step; A.max_cost = max_cost;
    A.plane = plane; A.cost = cost; A.tot0 = tot0; A.depth = depth;
    const int per = SELECT_THREADS / WAVE;
    hipLaunchKernelGGL(sgm_select_kernel, dim3((unsigned)((A.pixels + per - 1) / per)), dim3(SELECT_THREADS), 0,
                       iamx::as_stream(stream), A);
    return iamx::check_launch("iamx_dense_sgm_select");
}
