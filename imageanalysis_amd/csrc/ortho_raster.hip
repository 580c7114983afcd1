// Orthomosaic rasteriser (gfx950): the textured surface grids of Step 5 composed top-down into one
// georeferenced raster.  The rules are stated in imageanalysis_amd/ortho.py's docstring and restated
// in numpy by tests/ortho_restatement.py; this file follows them operation by operation.
//
// One launch per image, on the caller's stream: the launches of a group are ordered, so every
// read-modify-write of the accumulators sees the images in group order and nothing depends on
// timing.  No atomics.
//
// A workgroup is 16 x 16 pixels of the image's bounding box.
//   phase 1  the 256 lanes test the image's 2 S^2 triangles (256 per round) against the block's
//            rectangle of pixel centres and compact the hits, in file order, into LDS: a ballot per
//            wave, the waves' counts through LDS.  Zero-area triangles are dropped here.
//   phase 2  each pixel walks that short list; the first triangle that covers its centre owns it.
// Coverage is integer: vertices arrive snapped to 1/256 pixel (int32, at most 2^28), edge functions
// are int64 products of int32 differences (at most 2^57).  The texture coordinate, the sample, the
// metric and the weight are float64, every product and sum rounded on its own.
#include <math.h>

#include "iamx_common.h"

// the float64 expressions restate numpy's: build.sh passes -ffp-contract=off for this file as well
#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int TILE = 16;
constexpr int MAX_S = 32;                          // grid steps per side (the reference's default: 8)
constexpr int MAX_V = (MAX_S + 1) * (MAX_S + 1);
constexpr int MAX_T = 2 * MAX_S * MAX_S;
constexpr int MAX_SIDE = 1 << 20;
constexpr int MAX_GRID = 2048;

enum { MODE_BEST = 0, MODE_FEATHER = 1 };

struct RasterParams {
    double sx, sy;            // frame pixels per camera pixel: w_s / width, h_s / height
    double width, height;     // the camera's image size
    double half;              // 0.5 min(width, height)
    double x0, y1, gsd;       // east of column 0's left side, north of row 0's top side, metres per pixel
    double cx, cy, bias;      // best: the image's centre and 0.1 span
};

// triangle t of the grid: cell t / 2 = (j, i), c = j (S + 1) + i, d = c + S + 1;
// the first is (d, d + 1, c + 1), the second (d, c + 1, c)
__device__ __forceinline__ void tri_vertices(int t, int S, int &a, int &b, int &c)
{
    const int cell = t >> 1, j = cell / S, i = cell - j * S;
    const int vc = j * (S + 1) + i, vd = vc + S + 1;
    a = vd;
    b = (t & 1) ? vc + 1 : vd + 1;
    c = (t & 1) ? vc : vc + 1;
}

// the edge from (xs, ys) to (xe, ye) at the centre (px, py); inside: w > 0, or w == 0 on a top-left edge
__device__ __forceinline__ bool edge_owns(int xs, int ys, int xe, int ye, int px, int py, int64_t &w)
{
    const int ex = xe - xs, ey = ye - ys;
    w = (int64_t)ex * (int64_t)(py - ys) - (int64_t)ey * (int64_t)(px - xs);
    return w > 0 || (w == 0 && (ey < 0 || (ey == 0 && ex > 0)));
}

__device__ __forceinline__ double lerp(double a, double b, double t) { return a + (b - a) * t; }

__device__ __forceinline__ uint8_t round_u8(double v) { return (uint8_t)(int)floor(v + 0.5); }

template <int MODE>
__global__ __launch_bounds__(THREADS) void raster_kernel(int S, const int32_t *__restrict__ X,
                                                         const int32_t *__restrict__ Y,
                                                         const double *__restrict__ uv,
                                                         const uint8_t *__restrict__ used,
                                                         const uint8_t *__restrict__ frame, int h_s, int w_s,
                                                         RasterParams p, int image_index, int c0, int r0, int H,
                                                         int W, double *__restrict__ acc,
                                                         int32_t *__restrict__ index,
                                                         uint16_t *__restrict__ count, uint8_t *__restrict__ bgr)
{
    __shared__ int32_t sX[MAX_V], sY[MAX_V];
    __shared__ uint16_t list[MAX_T];
    __shared__ int wave_n[THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = (S + 1) * (S + 1), T = 2 * S * S;
    for (int i = tid; i < V; i += THREADS) {
        sX[i] = X[i];
        sY[i] = Y[i];
    }
    __syncthreads();

    // ---- phase 1: the triangles whose box meets the block's pixel centres, in file order ----
    const int bc = c0 + TILE * (int)blockIdx.x, br = r0 + TILE * (int)blockIdx.y;
    const int lo_x = 256 * bc + 128, hi_x = lo_x + 256 * (TILE - 1);
    const int lo_y = 256 * br + 128, hi_y = lo_y + 256 * (TILE - 1);
    int n = 0;
    for (int base = 0; base < T; base += THREADS) {
        const int t = base + tid;
        bool hit = false;
        if (t < T && used[t >> 1]) {
            int a, b, c;
            tri_vertices(t, S, a, b, c);
            const int xa = sX[a], ya = sY[a], xb = sX[b], yb = sY[b], xc = sX[c], yc = sY[c];
            const int64_t area2 = (int64_t)(xb - xa) * (int64_t)(yc - ya) - (int64_t)(yb - ya) * (int64_t)(xc - xa);
            hit = area2 != 0 && min(xa, min(xb, xc)) <= hi_x && max(xa, max(xb, xc)) >= lo_x
                  && min(ya, min(yb, yc)) <= hi_y && max(ya, max(yb, yc)) >= lo_y;
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) wave_n[wave] = __popcll(m);
        __syncthreads();
        int off = n;
        for (int w = 0; w < wave; ++w) off += wave_n[w];
        if (hit) list[off + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)t;
        n += wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
        __syncthreads();
    }
    if (n == 0) return;

    // ---- phase 2: the first triangle of the list that covers the pixel's centre ----
    const int col = bc + (tid & (TILE - 1)), row = br + (tid >> 4);
    if (col >= W || row >= H) return;                  // (no barrier below)
    const int px = 256 * col + 128, py = 256 * row + 128;
    bool found = false;
    int a = 0, b = 0, c = 0;
    int64_t w0 = 0, w1 = 0, w2 = 0;
    for (int k = 0; k < n && !found; ++k) {
        tri_vertices(list[k], S, a, b, c);
        int xa = sX[a], ya = sY[a], xb = sX[b], yb = sY[b], xc = sX[c], yc = sY[c];
        const int64_t area2 = (int64_t)(xb - xa) * (int64_t)(yc - ya) - (int64_t)(yb - ya) * (int64_t)(xc - xa);
        if (area2 < 0) {                               // re-oriented to positive area: b <-> c
            int s = b; b = c; c = s;
            s = xb; xb = xc; xc = s;
            s = yb; yb = yc; yc = s;
        }
        // w_k: the edge opposite vertex k (b -> c, c -> a, a -> b)
        const bool in0 = edge_owns(xb, yb, xc, yc, px, py, w0);
        const bool in1 = edge_owns(xc, yc, xa, ya, px, py, w1);
        const bool in2 = edge_owns(xa, ya, xb, yb, px, py, w2);
        found = in0 && in1 && in2;
    }
    if (!found) return;

    const int64_t q = (int64_t)row * W + col;
    uint16_t seen = count[q];
    count[q] = (uint16_t)(seen < 65535 ? seen + 1 : 65535);

    if (MODE == MODE_BEST) {
        const double east = p.x0 + ((double)col + 0.5) * p.gsd, north = p.y1 - ((double)row + 0.5) * p.gsd;
        const double dx = p.cx - east, dy = p.cy - north;
        const double metric = sqrt(dx * dx + dy * dy) + p.bias;
        if (!(metric < acc[q])) return;                // (a tie: the earlier image keeps the pixel)
        acc[q] = metric;
        index[q] = image_index;
    }

    // ---- texture coordinate and sample ----
    const double d0 = (double)w0, d1 = (double)w1, d2 = (double)w2;
    const double den = (d0 + d1) + d2;
    const double u = ((d0 * uv[2 * a] + d1 * uv[2 * b]) + d2 * uv[2 * c]) / den;
    const double v = ((d0 * uv[2 * a + 1] + d1 * uv[2 * b + 1]) + d2 * uv[2 * c + 1]) / den;
    const double fu = fmin(fmax(u * p.sx - 0.5, 0.0), (double)(w_s - 1));
    const double fv = fmin(fmax(v * p.sy - 0.5, 0.0), (double)(h_s - 1));
    const int x0 = (int)fu, y0 = (int)fv;
    const int x1 = min(x0 + 1, w_s - 1), y1 = min(y0 + 1, h_s - 1);
    const double tx = fu - (double)x0, ty = fv - (double)y0;
    const uint8_t *t00 = frame + ((int64_t)y0 * w_s + x0) * 3, *t01 = frame + ((int64_t)y0 * w_s + x1) * 3;
    const uint8_t *t10 = frame + ((int64_t)y1 * w_s + x0) * 3, *t11 = frame + ((int64_t)y1 * w_s + x1) * 3;
    double val[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double top = lerp((double)t00[ch], (double)t01[ch], tx);
        const double bot = lerp((double)t10[ch], (double)t11[ch], tx);
        val[ch] = lerp(top, bot, ty);
    }

    if (MODE == MODE_BEST) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) bgr[3 * q + ch] = round_u8(val[ch]);
    } else {
        const double d = fmin(fmin(u, p.width - u), fmin(v, p.height - v));
        const double wgt = fmax(d / p.half, 0x1.0p-20);
        double4 *cell = reinterpret_cast<double4 *>(acc) + q;
        double4 s = *cell;
        s.x = s.x + wgt * val[0];
        s.y = s.y + wgt * val[1];
        s.z = s.z + wgt * val[2];
        s.w = s.w + wgt;
        *cell = s;
    }
}

template <int MODE>
__global__ __launch_bounds__(THREADS) void clear_kernel(int64_t n, double *__restrict__ acc,
                                                        int32_t *__restrict__ index, uint16_t *__restrict__ count,
                                                        uint8_t *__restrict__ bgr)
{
    for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < n; q += (int64_t)gridDim.x * THREADS) {
        if (MODE == MODE_BEST) {
            acc[q] = INFINITY;
            index[q] = -1;
        } else {
            reinterpret_cast<double4 *>(acc)[q] = make_double4(0.0, 0.0, 0.0, 0.0);
        }
        count[q] = 0;
        bgr[3 * q] = 0;
        bgr[3 * q + 1] = 0;
        bgr[3 * q + 2] = 0;
    }
}

__global__ __launch_bounds__(THREADS) void resolve_kernel(int64_t n, const double *__restrict__ acc,
                                                          const uint16_t *__restrict__ count,
                                                          uint8_t *__restrict__ bgr)
{
    for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < n; q += (int64_t)gridDim.x * THREADS) {
        if (count[q] == 0) continue;                   // (cleared to zero)
        const double4 s = reinterpret_cast<const double4 *>(acc)[q];
        bgr[3 * q] = round_u8(s.x / s.w);
        bgr[3 * q + 1] = round_u8(s.y / s.w);
        bgr[3 * q + 2] = round_u8(s.z / s.w);
    }
}

inline int grid_for(int64_t items)
{
    int64_t g = (items + THREADS - 1) / THREADS;
    if (g < 1) g = 1;
    return (int)(g < MAX_GRID ? g : MAX_GRID);
}

inline bool aligned32(const void *p) { return ((uintptr_t)p & 31) == 0; }

}  // namespace

extern "C" int iamx_ortho_max_steps(void) { return MAX_S; }

extern "C" int iamx_ortho_clear(int mode, int H, int W, double *acc, int32_t *index, uint16_t *count,
                                uint8_t *bgr, void *stream)
{
    IAMX_REQUIRE(mode == MODE_BEST || mode == MODE_FEATHER, "mode must be 0 (best) or 1 (feather)");
    IAMX_REQUIRE(acc && count && bgr && (mode == MODE_FEATHER || index), "null pointer");
    IAMX_REQUIRE(H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "raster sides out of range (1 .. 2^20)");
    IAMX_REQUIRE(mode == MODE_BEST || aligned32(acc), "the feather accumulator must be 32-byte aligned");
    const int64_t n = (int64_t)H * W;
    hipStream_t st = iamx::as_stream(stream);
    if (mode == MODE_BEST)
        hipLaunchKernelGGL(clear_kernel<MODE_BEST>, dim3(grid_for(n)), dim3(THREADS), 0, st, n, acc, index, count, bgr);
    else
        hipLaunchKernelGGL(clear_kernel<MODE_FEATHER>, dim3(grid_for(n)), dim3(THREADS), 0, st, n, acc, index, count,
                           bgr);
    return iamx::check_launch("iamx_ortho_clear");
}

extern "C" int iamx_ortho_raster_image(int mode, int S, const int32_t *X, const int32_t *Y, const double *uv,
                                       const uint8_t *used, const uint8_t *frame, int h_s, int w_s,
                                       const double *params, int image_index, int c0, int r0, int c1, int r1,
                                       int H, int W, double *acc, int32_t *index, uint16_t *count, uint8_t *bgr,
                                       void *stream)
{
    IAMX_REQUIRE(mode == MODE_BEST || mode == MODE_FEATHER, "mode must be 0 (best) or 1 (feather)");
    IAMX_REQUIRE(X && Y && uv && used && frame && params, "null pointer");
    IAMX_REQUIRE(acc && count && bgr && (mode == MODE_FEATHER || index), "null pointer");
    IAMX_REQUIRE(S >= 1 && S <= MAX_S, "grid steps out of range (1 .. 32)");
    IAMX_REQUIRE(h_s >= 1 && w_s >= 1, "empty frame");
    IAMX_REQUIRE(H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "raster sides out of range (1 .. 2^20)");
    IAMX_REQUIRE(mode == MODE_BEST || aligned32(acc), "the feather accumulator must be 32-byte aligned");
    if (c1 < c0 || r1 < r0) return 0;                  // covers nothing: no launch
    IAMX_REQUIRE(c0 >= 0 && r0 >= 0 && c1 < W && r1 < H, "the image's pixel box leaves the raster");
    RasterParams p;
    p.width = params[0];
    p.height = params[1];
    p.x0 = params[2];
    p.y1 = params[3];
    p.gsd = params[4];
    p.cx = params[5];
    p.cy = params[6];
    p.bias = params[7];
    IAMX_REQUIRE(p.width >= 1.0 && p.height >= 1.0, "camera image size must be at least 1 x 1");
    IAMX_REQUIRE(isfinite(p.x0) && isfinite(p.y1) && p.gsd > 0.0 && isfinite(p.gsd), "raster frame is not finite");
    IAMX_REQUIRE(isfinite(p.cx) && isfinite(p.cy) && isfinite(p.bias), "image centre is not finite");
    p.sx = (double)w_s / p.width;
    p.sy = (double)h_s / p.height;
    p.half = 0.5 * fmin(p.width, p.height);
    c0 &= ~(TILE - 1);                                 // blocks start on multiples of 16 of the raster
    r0 &= ~(TILE - 1);
    const int gx = (c1 - c0) / TILE + 1, gy = (r1 - r0) / TILE + 1;
    IAMX_REQUIRE(gy <= 65535, "the image's pixel box is too tall for one launch");
    hipStream_t st = iamx::as_stream(stream);
    if (mode == MODE_BEST)
        hipLaunchKernelGGL(raster_kernel<MODE_BEST>, dim3(gx, gy), dim3(THREADS), 0, st, S, X, Y, uv, used, frame, h_s,
                           w_s, p, image_index, c0, r0, H, W, acc, index, count, bgr);
    else
        hipLaunchKernelGGL(raster_kernel<MODE_FEATHER>, dim3(gx, gy), dim3(THREADS), 0, st, S, X, Y, uv, used, frame,
                           h_s, w_s, p, image_index, c0, r0, H, W, acc, index, count, bgr);
    return iamx::check_launch("iamx_ortho_raster_image");
}

extern "C" int iamx_ortho_resolve(int H, int W, const double *acc, const uint16_t *count, uint8_t *bgr,
                                  void *stream)
{
    IAMX_REQUIRE(acc && count && bgr, "null pointer");
    IAMX_REQUIRE(H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "raster sides out of range (1 .. 2^20)");
    IAMX_REQUIRE(aligned32(acc), "the feather accumulator must be 32-byte aligned");
    const int64_t n = (int64_t)H * W;
    hipLaunchKernelGGL(resolve_kernel, dim3(grid_for(n)), dim3(THREADS), 0, iamx::as_stream(stream), n, acc, count,
                       bgr);
    return iamx::check_launch("iamx_ortho_resolve");
}
