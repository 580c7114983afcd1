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
//
// Mode multiband (the second half of the file) blends along mode best's seams with Laplacian
// pyramids in float32: (a) mb_layer_kernel writes an image's colour and ownership layer over its
// pixel box with the coverage and sample code above, (b) mb_reduce_kernel makes the layer's
// Gaussian pyramid, (c) mb_accumulate_kernel expands, subtracts, multiplies and adds every level
// into the mosaic's accumulators, (d) mb_collapse_kernel resolves them from the top level down
// into bgr.  Per image the work is limited to the regions its layer can reach.
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

enum { MODE_BEST = 0, MODE_FEATHER = 1, MODE_OWNER = 2 };   // (MODE_OWNER: inside this file only)

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

// the winning triangle of a pixel: its vertices after re-orientation and its three edge values
struct Cover {
    int a, b, c;
    int64_t w0, w1, w2;
};

// what a block keeps in LDS: the image's snapped vertices and the triangles that meet the block
struct BlockLists {
    int32_t sX[MAX_V], sY[MAX_V];
    uint16_t list[MAX_T];
    int wave_n[THREADS / 64];
};

// ---- phase 1: the triangles whose box meets the block's pixel centres, in file order ----
// (all 256 lanes call it: it holds barriers) -> the length of L.list
__device__ __forceinline__ int block_triangles(int S, const int32_t *__restrict__ X, const int32_t *__restrict__ Y,
                                               const uint8_t *__restrict__ used, int bc, int br, BlockLists &L)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = (S + 1) * (S + 1), T = 2 * S * S;
    for (int i = tid; i < V; i += THREADS) {
        L.sX[i] = X[i];
        L.sY[i] = Y[i];
    }
    __syncthreads();
    const int lo_x = 256 * bc + 128, hi_x = lo_x + 256 * (TILE - 1);
    const int lo_y = 256 * br + 128, hi_y = lo_y + 256 * (TILE - 1);
    int n = 0;
    for (int base = 0; base < T; base += THREADS) {
        const int t = base + tid;
        bool hit = false;
        if (t < T && used[t >> 1]) {
            int a, b, c;
            tri_vertices(t, S, a, b, c);
            const int xa = L.sX[a], ya = L.sY[a], xb = L.sX[b], yb = L.sY[b], xc = L.sX[c], yc = L.sY[c];
            const int64_t area2 = (int64_t)(xb - xa) * (int64_t)(yc - ya) - (int64_t)(yb - ya) * (int64_t)(xc - xa);
            hit = area2 != 0 && min(xa, min(xb, xc)) <= hi_x && max(xa, max(xb, xc)) >= lo_x
                  && min(ya, min(yb, yc)) <= hi_y && max(ya, max(yb, yc)) >= lo_y;
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) L.wave_n[wave] = __popcll(m);
        __syncthreads();
        int off = n;
        for (int w = 0; w < wave; ++w) off += L.wave_n[w];
        if (hit) L.list[off + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)t;
        n += L.wave_n[0] + L.wave_n[1] + L.wave_n[2] + L.wave_n[3];
        __syncthreads();
    }
    return n;
}

// ---- phase 2: the first triangle of the list that covers the pixel's centre ----
__device__ __forceinline__ bool covering_triangle(int S, const BlockLists &L, int n, int col, int row, Cover &h)
{
    const int px = 256 * col + 128, py = 256 * row + 128;
    bool found = false;
    int a = 0, b = 0, c = 0;
    int64_t w0 = 0, w1 = 0, w2 = 0;
    for (int k = 0; k < n && !found; ++k) {
        tri_vertices(L.list[k], S, a, b, c);
        int xa = L.sX[a], ya = L.sY[a], xb = L.sX[b], yb = L.sY[b], xc = L.sX[c], yc = L.sY[c];
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
    h.a = a; h.b = b; h.c = c;
    h.w0 = w0; h.w1 = w1; h.w2 = w2;
    return found;
}

// ---- texture coordinate and sample ----
__device__ __forceinline__ void texture_sample(const Cover &h, const double *__restrict__ uv,
                                               const uint8_t *__restrict__ frame, int h_s, int w_s,
                                               const RasterParams &p, double &u, double &v, double val[3])
{
    const double d0 = (double)h.w0, d1 = (double)h.w1, d2 = (double)h.w2;
    const double den = (d0 + d1) + d2;
    u = ((d0 * uv[2 * h.a] + d1 * uv[2 * h.b]) + d2 * uv[2 * h.c]) / den;
    v = ((d0 * uv[2 * h.a + 1] + d1 * uv[2 * h.b + 1]) + d2 * uv[2 * h.c + 1]) / den;
    const double fu = fmin(fmax(u * p.sx - 0.5, 0.0), (double)(w_s - 1));
    const double fv = fmin(fmax(v * p.sy - 0.5, 0.0), (double)(h_s - 1));
    const int x0 = (int)fu, y0 = (int)fv;
    const int x1 = min(x0 + 1, w_s - 1), y1 = min(y0 + 1, h_s - 1);
    const double tx = fu - (double)x0, ty = fv - (double)y0;
    const uint8_t *t00 = frame + ((int64_t)y0 * w_s + x0) * 3, *t01 = frame + ((int64_t)y0 * w_s + x1) * 3;
    const uint8_t *t10 = frame + ((int64_t)y1 * w_s + x0) * 3, *t11 = frame + ((int64_t)y1 * w_s + x1) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double top = lerp((double)t00[ch], (double)t01[ch], tx);
        const double bot = lerp((double)t10[ch], (double)t11[ch], tx);
        val[ch] = lerp(top, bot, ty);
    }
}

// MODE_OWNER: mode best without its sample -- count, metric and index from the geometry alone
// (uv, frame and bgr are not read)
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
    __shared__ BlockLists L;
    const int tid = threadIdx.x;
    const int bc = c0 + TILE * (int)blockIdx.x, br = r0 + TILE * (int)blockIdx.y;
    const int n = block_triangles(S, X, Y, used, bc, br, L);
    if (n == 0) return;

    const int col = bc + (tid & (TILE - 1)), row = br + (tid >> 4);
    if (col >= W || row >= H) return;                  // (no barrier below)
    Cover h;
    if (!covering_triangle(S, L, n, col, row, h)) return;

    const int64_t q = (int64_t)row * W + col;
    uint16_t seen = count[q];
    count[q] = (uint16_t)(seen < 65535 ? seen + 1 : 65535);

    if (MODE != MODE_FEATHER) {
        const double east = p.x0 + ((double)col + 0.5) * p.gsd, north = p.y1 - ((double)row + 0.5) * p.gsd;
        const double dx = p.cx - east, dy = p.cy - north;
        const double metric = sqrt(dx * dx + dy * dy) + p.bias;
        if (!(metric < acc[q])) return;                // (a tie: the earlier image keeps the pixel)
        acc[q] = metric;
        index[q] = image_index;
    }
    if (MODE == MODE_OWNER) return;

    double u, v, val[3];
    texture_sample(h, uv, frame, h_s, w_s, p, u, v, val);

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

// params HOST f64 [8] -> RasterParams; the text of what is wrong with them, or null
inline const char *raster_params(const double *params, int h_s, int w_s, RasterParams &p)
{
    p.width = params[0];
    p.height = params[1];
    p.x0 = params[2];
    p.y1 = params[3];
    p.gsd = params[4];
    p.cx = params[5];
    p.cy = params[6];
    p.bias = params[7];
    if (!(p.width >= 1.0 && p.height >= 1.0)) return "camera image size must be at least 1 x 1";
    if (!(isfinite(p.x0) && isfinite(p.y1) && p.gsd > 0.0 && isfinite(p.gsd))) return "raster frame is not finite";
    if (!(isfinite(p.cx) && isfinite(p.cy) && isfinite(p.bias))) return "image centre is not finite";
    p.sx = (double)w_s / p.width;
    p.sy = (double)h_s / p.height;
    p.half = 0.5 * fmin(p.width, p.height);
    return nullptr;
}

// ================================ mode multiband ================================
// Laplacian pyramids in float32, every product and sum rounded on its own (no contraction in this
// file); the one division is done in float64 and rounded once.  A pixel of a level is a float4:
// a layer holds (C_b, C_g, C_r, A), an accumulator (N_b, N_g, N_r, D).  A layer level lives in a
// buffer of its REGION only (an inclusive box of the level, row-major); outside it the layer is 0.
constexpr int RT = 2 * TILE + 3;                   // the source rows / columns under 16 reduced ones
constexpr int ET = TILE / 2 + 2;                   // the coarse rows / columns under 16 expanded ones

struct Region {
    int y0, x0, y1, x1;                            // inclusive
};

__device__ __forceinline__ float4 zero4() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

__device__ __forceinline__ float4 region_load(const float4 *__restrict__ p, const Region &r, int y, int x)
{
    if (y < r.y0 || y > r.y1 || x < r.x0 || x > r.x1) return zero4();
    return p[(int64_t)(y - r.y0) * (r.x1 - r.x0 + 1) + (x - r.x0)];
}

// reduce: ((((g0 a + g1 b) + g2 c) + g1 d) + g0 e), g = (1, 4, 6) / 16
__device__ __forceinline__ float tap5(float a, float b, float c, float d, float e)
{
    return (((0.0625f * a + 0.25f * b) + 0.375f * c) + 0.25f * d) + 0.0625f * e;
}

__device__ __forceinline__ float4 tap5(const float4 &a, const float4 &b, const float4 &c, const float4 &d,
                                       const float4 &e)
{
    return make_float4(tap5(a.x, b.x, c.x, d.x, e.x), tap5(a.y, b.y, c.y, d.y, e.y), tap5(a.z, b.z, c.z, d.z, e.z),
                       tap5(a.w, b.w, c.w, d.w, e.w));
}

// expand: even 2m: ((X[m-1] + 6 X[m]) + X[m+1]) 0.125; odd 2m+1: (X[m] + X[m+1]) 0.5
__device__ __forceinline__ float up_even(float l, float m, float r) { return ((l + 6.0f * m) + r) * 0.125f; }
__device__ __forceinline__ float up_odd(float m, float r) { return (m + r) * 0.5f; }

// (b) reduce: 16 x 16 pixels of the coarser level per block from 35 x 35 of the finer one in LDS,
// rows first (along x), then columns.  The pitches are odd (35, 17 float4), so that lanes walking
// down a column of the tile fall on 16 different 16-byte slots of the bank row.
__global__ __launch_bounds__(THREADS) void mb_reduce_kernel(const float4 *__restrict__ src, Region sr,
                                                            float4 *__restrict__ dst, Region dr)
{
    __shared__ float4 tile[RT][RT];
    __shared__ float4 rows[RT][TILE + 1];
    const int tid = threadIdx.x;
    const int oy = dr.y0 + TILE * (int)blockIdx.y, ox = dr.x0 + TILE * (int)blockIdx.x;
    const int sy = 2 * oy - 2, sx = 2 * ox - 2;
    for (int i = tid; i < RT * RT; i += THREADS) {
        const int r = i / RT, c = i - r * RT;
        tile[r][c] = region_load(src, sr, sy + r, sx + c);
    }
    __syncthreads();
    for (int i = tid; i < RT * TILE; i += THREADS) {
        const int j = i / RT, r = i - j * RT;
        rows[r][j] = tap5(tile[r][2 * j], tile[r][2 * j + 1], tile[r][2 * j + 2], tile[r][2 * j + 3], tile[r][2 * j + 4]);
    }
    __syncthreads();
    const int tx = tid & (TILE - 1), ty = tid >> 4;
    const int y = oy + ty, x = ox + tx;
    if (y > dr.y1 || x > dr.x1) return;
    dst[(int64_t)(y - dr.y0) * (dr.x1 - dr.x0 + 1) + (x - dr.x0)] =
        tap5(rows[2 * ty][tx], rows[2 * ty + 1][tx], rows[2 * ty + 2][tx], rows[2 * ty + 3][tx], rows[2 * ty + 4][tx]);
}

// E(up) at the block's 16 x 16 pixels (origin oy, ox: multiples of 16), the first three planes:
// 10 x 10 coarse pixels in LDS, rows first (along x), then columns.  All 256 lanes call it.
__device__ __forceinline__ float4 expand_tile(const float4 *__restrict__ up, const Region &ur, int oy, int ox,
                                              float4 (*ct)[ET], float4 (*he)[TILE + 1])
{
    const int tid = threadIdx.x;
    const int my = oy / 2 - 1, mx = ox / 2 - 1;
    if (tid < ET * ET) {
        const int r = tid / ET, c = tid - r * ET;
        ct[r][c] = region_load(up, ur, my + r, mx + c);
    }
    __syncthreads();
    if (tid < ET * TILE) {
        const int r = tid >> 4, j = tid & (TILE - 1), m = (j >> 1) + 1;
        const float4 a = ct[r][m - 1], b = ct[r][m], c = ct[r][m + 1];
        he[r][j] = (j & 1) ? make_float4(up_odd(b.x, c.x), up_odd(b.y, c.y), up_odd(b.z, c.z), 0.0f)
                           : make_float4(up_even(a.x, b.x, c.x), up_even(a.y, b.y, c.y), up_even(a.z, b.z, c.z), 0.0f);
    }
    __syncthreads();
    const int tx = tid & (TILE - 1), ty = tid >> 4, m = (ty >> 1) + 1;
    const float4 a = he[m - 1][tx], b = he[m][tx], c = he[m + 1][tx];
    return (ty & 1) ? make_float4(up_odd(b.x, c.x), up_odd(b.y, c.y), up_odd(b.z, c.z), 0.0f)
                    : make_float4(up_even(a.x, b.x, c.x), up_even(a.y, b.y, c.y), up_even(a.z, b.z, c.z), 0.0f);
}

// (c) accumulate: LP = GC - E(GC of the coarser level) (the top level: LP = GC), N += GA LP, D += GA,
// over the finer layer's region; acc is the whole level [h][w]
__global__ __launch_bounds__(THREADS) void mb_accumulate_kernel(const float4 *__restrict__ fine, Region fr,
                                                                const float4 *__restrict__ coarse, Region cr,
                                                                float4 *__restrict__ acc, int w)
{
    __shared__ float4 ct[ET][ET];
    __shared__ float4 he[ET][TILE + 1];
    const int oy = (fr.y0 & ~(TILE - 1)) + TILE * (int)blockIdx.y, ox = (fr.x0 & ~(TILE - 1)) + TILE * (int)blockIdx.x;
    float4 e = zero4();
    if (coarse) e = expand_tile(coarse, cr, oy, ox, ct, he);       // (uniform over the block)
    const int y = oy + (int)(threadIdx.x >> 4), x = ox + (int)(threadIdx.x & (TILE - 1));
    if (y < fr.y0 || y > fr.y1 || x < fr.x0 || x > fr.x1) return;
    const float4 g = fine[(int64_t)(y - fr.y0) * (fr.x1 - fr.x0 + 1) + (x - fr.x0)];
    float4 *cell = acc + ((int64_t)y * w + x);
    float4 s = *cell;
    if (coarse) {
        s.x = s.x + g.w * (g.x - e.x);
        s.y = s.y + g.w * (g.y - e.y);
        s.z = s.z + g.w * (g.z - e.z);
    } else {
        s.x = s.x + g.w * g.x;
        s.y = s.y + g.w * g.y;
        s.z = s.z + g.w * g.z;
    }
    s.w = s.w + g.w;
    *cell = s;
}

// N / D: float64, rounded once to float32 (the correctly rounded float32 quotient)
__device__ __forceinline__ float quotient(float n, float d) { return d > 0.0f ? (float)((double)n / (double)d) : 0.0f; }

__device__ __forceinline__ uint8_t clamp_u8(float m) { return (uint8_t)(int)floorf(fminf(fmaxf(m, 0.0f), 255.0f) + 0.5f); }

// (d) collapse, one level: M = N / D + E(M of the coarser level) (the top level: M = N / D), over the
// whole level.  bgr == null: M replaces N in place (D stays); else the level is 0 and M ends in bgr.
__global__ __launch_bounds__(THREADS) void mb_collapse_kernel(float4 *__restrict__ acc, int h, int w,
                                                              const float4 *__restrict__ up, Region ur,
                                                              const uint16_t *__restrict__ count,
                                                              uint8_t *__restrict__ bgr)
{
    __shared__ float4 ct[ET][ET];
    __shared__ float4 he[ET][TILE + 1];
    const int oy = TILE * (int)blockIdx.y, ox = TILE * (int)blockIdx.x;
    float4 e = zero4();
    if (up) e = expand_tile(up, ur, oy, ox, ct, he);
    const int y = oy + (int)(threadIdx.x >> 4), x = ox + (int)(threadIdx.x & (TILE - 1));
    if (y >= h || x >= w) return;
    const int64_t q = (int64_t)y * w + x;
    float4 s = acc[q];
    s.x = quotient(s.x, s.w);
    s.y = quotient(s.y, s.w);
    s.z = quotient(s.z, s.w);
    if (up) {
        s.x = s.x + e.x;
        s.y = s.y + e.y;
        s.z = s.z + e.z;
    }
    if (!bgr) {
        acc[q] = s;
        return;
    }
    const bool seen = count[q] > 0;
    bgr[3 * q] = seen ? clamp_u8(s.x) : 0;
    bgr[3 * q + 1] = seen ? clamp_u8(s.y) : 0;
    bgr[3 * q + 2] = seen ? clamp_u8(s.z) : 0;
}

// (a) layer: C_k where image k covers the pixel (the sample, float64 cast to float32), A_k where it
// owns it, over the image's pixel box b; coverage and sample are raster_kernel's
__global__ __launch_bounds__(THREADS) void mb_layer_kernel(int S, const int32_t *__restrict__ X,
                                                           const int32_t *__restrict__ Y,
                                                           const double *__restrict__ uv,
                                                           const uint8_t *__restrict__ used,
                                                           const uint8_t *__restrict__ frame, int h_s, int w_s,
                                                           RasterParams p, int image_index, Region b, int W,
                                                           const int32_t *__restrict__ index,
                                                           float4 *__restrict__ layer)
{
    __shared__ BlockLists L;
    const int tid = threadIdx.x;
    const int bc = (b.x0 & ~(TILE - 1)) + TILE * (int)blockIdx.x, br = (b.y0 & ~(TILE - 1)) + TILE * (int)blockIdx.y;
    const int n = block_triangles(S, X, Y, used, bc, br, L);
    const int col = bc + (tid & (TILE - 1)), row = br + (tid >> 4);
    if (col < b.x0 || col > b.x1 || row < b.y0 || row > b.y1) return;
    float4 out = zero4();
    Cover h;
    if (n > 0 && covering_triangle(S, L, n, col, row, h)) {
        double u, v, val[3];
        texture_sample(h, uv, frame, h_s, w_s, p, u, v, val);
        out.x = (float)val[0];
        out.y = (float)val[1];
        out.z = (float)val[2];
    }
    out.w = index[(int64_t)row * W + col] == image_index ? 1.0f : 0.0f;
    layer[(int64_t)(row - b.y0) * (b.x1 - b.x0 + 1) + (col - b.x0)] = out;
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

inline bool level_side(int n) { return n >= 1 && n <= MAX_SIDE; }

inline bool region_in(const Region &r, int h, int w)
{
    return r.y0 >= 0 && r.x0 >= 0 && r.y0 <= r.y1 && r.x0 <= r.x1 && r.y1 < h && r.x1 < w;
}

// the blocks of 16 x 16 that start on multiples of 16 of the level and reach the region's last pixel
inline dim3 blocks_over(const Region &r)
{
    return dim3((r.x1 - (r.x0 & ~(TILE - 1))) / TILE + 1, (r.y1 - (r.y0 & ~(TILE - 1))) / TILE + 1);
}

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
    const char *bad = raster_params(params, h_s, w_s, p);
    IAMX_REQUIRE(!bad, bad);
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

// ---- mode multiband (the rules: imageanalysis_amd/ortho.py; restated by tests/ortho_multiband_restatement.py) ----
extern "C" int iamx_ortho_mb_owner(int S, const int32_t *X, const int32_t *Y, const uint8_t *used,
                                   const double *params, int image_index, int c0, int r0, int c1, int r1, int H,
                                   int W, double *metric, int32_t *index, uint16_t *count, void *stream)
{
    IAMX_REQUIRE(X && Y && used && params && metric && index && count, "null pointer");
    IAMX_REQUIRE(S >= 1 && S <= MAX_S, "grid steps out of range (1 .. 32)");
    IAMX_REQUIRE(level_side(H) && level_side(W), "raster sides out of range (1 .. 2^20)");
    if (c1 < c0 || r1 < r0) return 0;                  // covers nothing: no launch
    IAMX_REQUIRE(c0 >= 0 && r0 >= 0 && c1 < W && r1 < H, "the image's pixel box leaves the raster");
    RasterParams p;
    const char *bad = raster_params(params, 1, 1, p);
    IAMX_REQUIRE(!bad, bad);
    const Region b = {r0, c0, r1, c1};
    const dim3 grid = blocks_over(b);
    IAMX_REQUIRE(grid.y <= 65535, "the image's pixel box is too tall for one launch");
    hipLaunchKernelGGL(raster_kernel<MODE_OWNER>, grid, dim3(THREADS), 0, iamx::as_stream(stream), S, X, Y,
                       (const double *)nullptr, used, (const uint8_t *)nullptr, 1, 1, p, image_index,
                       c0 & ~(TILE - 1), r0 & ~(TILE - 1), H, W, metric, index, count, (uint8_t *)nullptr);
    return iamx::check_launch("iamx_ortho_mb_owner");
}

extern "C" int iamx_ortho_mb_layer(int S, const int32_t *X, const int32_t *Y, const double *uv, const uint8_t *used,
                                   const uint8_t *frame, int h_s, int w_s, const double *params, int image_index,
                                   int c0, int r0, int c1, int r1, int H, int W, const int32_t *index, float *layer,
                                   void *stream)
{
    IAMX_REQUIRE(X && Y && uv && used && frame && params && index && layer, "null pointer");
    IAMX_REQUIRE(S >= 1 && S <= MAX_S, "grid steps out of range (1 .. 32)");
    IAMX_REQUIRE(h_s >= 1 && w_s >= 1, "empty frame");
    IAMX_REQUIRE(level_side(H) && level_side(W), "raster sides out of range (1 .. 2^20)");
    IAMX_REQUIRE(aligned16(layer), "the layer must be 16-byte aligned");
    if (c1 < c0 || r1 < r0) return 0;                  // covers nothing: no launch
    IAMX_REQUIRE(c0 >= 0 && r0 >= 0 && c1 < W && r1 < H, "the image's pixel box leaves the raster");
    RasterParams p;
    const char *bad = raster_params(params, h_s, w_s, p);
    IAMX_REQUIRE(!bad, bad);
    const Region b = {r0, c0, r1, c1};
    const dim3 grid = blocks_over(b);
    IAMX_REQUIRE(grid.y <= 65535, "the image's pixel box is too tall for one launch");
    hipLaunchKernelGGL(mb_layer_kernel, grid, dim3(THREADS), 0, iamx::as_stream(stream), S, X, Y, uv, used, frame,
                       h_s, w_s, p, image_index, b, W, index, reinterpret_cast<float4 *>(layer));
    return iamx::check_launch("iamx_ortho_mb_layer");
}

extern "C" int iamx_ortho_mb_reduce(int h, int w, const float *src, int sy0, int sx0, int sy1, int sx1, float *dst,
                                    int dy0, int dx0, int dy1, int dx1, void *stream)
{
    IAMX_REQUIRE(src && dst, "null pointer");
    IAMX_REQUIRE(level_side(h) && level_side(w), "level sides out of range (1 .. 2^20)");
    IAMX_REQUIRE(aligned16(src) && aligned16(dst), "the layers must be 16-byte aligned");
    const Region sr = {sy0, sx0, sy1, sx1}, dr = {dy0, dx0, dy1, dx1};
    IAMX_REQUIRE(region_in(sr, h, w), "the source region leaves its level");
    IAMX_REQUIRE(region_in(dr, (h + 1) / 2, (w + 1) / 2), "the destination region leaves the coarser level");
    const dim3 grid((dx1 - dx0) / TILE + 1, (dy1 - dy0) / TILE + 1);
    IAMX_REQUIRE(grid.y <= 65535, "the region is too tall for one launch");
    hipLaunchKernelGGL(mb_reduce_kernel, grid, dim3(THREADS), 0, iamx::as_stream(stream),
                       reinterpret_cast<const float4 *>(src), sr, reinterpret_cast<float4 *>(dst), dr);
    return iamx::check_launch("iamx_ortho_mb_reduce");
}

extern "C" int iamx_ortho_mb_accumulate(int h, int w, const float *fine, int fy0, int fx0, int fy1, int fx1,
                                        const float *coarse, int cy0, int cx0, int cy1, int cx1, float *acc,
                                        void *stream)
{
    IAMX_REQUIRE(fine && acc, "null pointer");
    IAMX_REQUIRE(level_side(h) && level_side(w), "level sides out of range (1 .. 2^20)");
    IAMX_REQUIRE(aligned16(fine) && aligned16(coarse) && aligned16(acc), "layers and accumulator must be 16-byte aligned");
    const Region fr = {fy0, fx0, fy1, fx1}, cr = {cy0, cx0, cy1, cx1};
    IAMX_REQUIRE(region_in(fr, h, w), "the region leaves its level");
    IAMX_REQUIRE(!coarse || region_in(cr, (h + 1) / 2, (w + 1) / 2), "the coarser region leaves its level");
    const dim3 grid = blocks_over(fr);
    IAMX_REQUIRE(grid.y <= 65535, "the region is too tall for one launch");
    hipLaunchKernelGGL(mb_accumulate_kernel, grid, dim3(THREADS), 0, iamx::as_stream(stream),
                       reinterpret_cast<const float4 *>(fine), fr, reinterpret_cast<const float4 *>(coarse), cr,
                       reinterpret_cast<float4 *>(acc), w);
    return iamx::check_launch("iamx_ortho_mb_accumulate");
}

extern "C" int iamx_ortho_mb_collapse(int h, int w, float *acc, const float *up, const uint16_t *count, uint8_t *bgr,
                                      void *stream)
{
    IAMX_REQUIRE(acc && (!bgr || count), "null pointer");
    IAMX_REQUIRE(level_side(h) && level_side(w), "level sides out of range (1 .. 2^20)");
    IAMX_REQUIRE(aligned16(acc) && aligned16(up), "the accumulators must be 16-byte aligned");
    const Region ur = {0, 0, (h + 1) / 2 - 1, (w + 1) / 2 - 1};
    const dim3 grid((w - 1) / TILE + 1, (h - 1) / TILE + 1);
    IAMX_REQUIRE(grid.y <= 65535, "the level is too tall for one launch");
    hipLaunchKernelGGL(mb_collapse_kernel, grid, dim3(THREADS), 0, iamx::as_stream(stream),
                       reinterpret_cast<float4 *>(acc), h, w, reinterpret_cast<const float4 *>(up), ur, count, bgr);
    return iamx::check_launch("iamx_ortho_mb_collapse");
}
