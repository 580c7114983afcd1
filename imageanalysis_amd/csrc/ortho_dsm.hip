// True orthophoto (gfx950): the frames of a group draped over the dense DSM, occlusion tested.  The
// rules are stated in imageanalysis_amd/ortho.py's docstring ("THE TRUE-ORTHO RULES") and restated
// in numpy by tests/ortho_dense_restatement.py; this file follows them operation by operation
// (float64, every product and sum rounded on its own: the pragma below switches contraction off for
// the whole file, which is what -ffp-contract=off gives; build.sh's flag table is unchanged).
//
// dsm_kernel<MODE>: one launch per image, on the caller's stream, so every read-modify-write of the
// accumulators sees the images in group order; no atomics.  One thread per mosaic pixel of the
// image's work box, a workgroup is 16 x 16 pixels, a wave 16 x 4: neighbouring lanes march
// neighbouring DSM cells towards the same camera, so the height reads of a step fall into a few
// cache lines.  Per pixel, the cheap rejects first:
//   height     bilinear in the DSM at the pixel's centre (a tap of weight zero is not read);
//   project    the full camera model; most pixels of a box that is not the frame's footprint end here;
//   dh         the camera is above the point;
//   march      towards the camera's foot, one DSM cell of the major axis per step, until the ray
//              is above the highest cell, leaves the raster or meets a cell above it;
//   sample     bilinear in the frame, then mode best's or mode feather's composition, with the
//              accumulator layouts of csrc/ortho_raster.hip (its clear and resolve are reused).
//
// dsm_kernel<MODE_OWNER> and layer_kernel: the two passes that mode multiband's pyramid kernels
// (csrc/ortho_raster.hip) want over a dense surface.  The owner pass is mode best without frame and
// bgr: count, metric and index from the geometry alone.  The layer pass is height, project and sample
// without the march: the colour wherever the image covers the pixel, seen or not, and the ownership
// from `index`, as four floats per pixel of the work box, every pixel of the box written.
//
// fill_kernel: one round of the DSM hole fill per launch, one thread per cell, ping-pong.
#include <math.h>

#include "iamx_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int TILE = 16;
constexpr int MAX_SIDE = 1 << 20;
constexpr int PARAMS = IAMX_ORTHO_DSM_PARAMS;      // 26

enum { MODE_BEST = 0, MODE_FEATHER = 1, MODE_OWNER = 2 };    // (owner: no entry point takes it as a number)

struct DsmParams {
    double x0, y1, gsd, bias, zmax;
    double R[9], C[3], fx, fy, cx, cy, k1, k2, p1, p2, k3;
    double ss, g;             // the upsample as a double, the mosaic's pixel size gsd / ss
    double qx, qy;            // the camera's foot in DSM cell units
    double half;              // feather: 0.5 min(w_s - 1, h_s - 1)
};

__device__ __forceinline__ double lerp(double a, double b, double t) { return a + (b - a) * t; }

__device__ __forceinline__ uint8_t round_u8(double v) { return (uint8_t)(int)floor(v + 0.5); }

// the DSM at (row, gx): Z[xa] + (Z[xb] - Z[xa]) tx, Z[xa] alone when tx == 0
__device__ __forceinline__ double row_height(const float *__restrict__ row, int xa, int xb, double tx)
{
    const double a = (double)row[xa];
    if (tx == 0.0) return a;
    return a + ((double)row[xb] - a) * tx;
}

// the bilinear DSM height at the centre (pc, pr) of a mosaic pixel; NaN: a hole
__device__ __forceinline__ double pixel_height(const float *__restrict__ dsm, int H, int W, const DsmParams &p,
                                               double pc, double pr, double &px, double &py)
{
    px = pc / p.ss;
    py = pr / p.ss;
    const double gx = fmin(fmax(px - 0.5, 0.0), (double)(W - 1));
    const double gy = fmin(fmax(py - 0.5, 0.0), (double)(H - 1));
    const int xa = (int)gx, ya = (int)gy;
    const int xb = min(xa + 1, W - 1), yb = min(ya + 1, H - 1);
    const double tx = gx - (double)xa, ty = gy - (double)ya;
    const double top = row_height(dsm + (int64_t)ya * W, xa, xb, tx);
    double h = top;
    if (ty != 0.0) h = top + (row_height(dsm + (int64_t)yb * W, xa, xb, tx) - top) * ty;
    return h;
}

// the projection of the pixel at height h (dense.py's warp from D = Xw - Cn onward)
struct Projected {
    double dn, de, Z, fu, fv;
};

__device__ __forceinline__ void project(const DsmParams &p, double pc, double pr, double h, Projected &o)
{
    const double east = p.x0 + pc * p.g, north = p.y1 - pr * p.g;
    const double dn = north - p.C[0], de = east - p.C[1], dd = (-h) - p.C[2];
    const double X = (p.R[0] * dn + p.R[1] * de) + p.R[2] * dd;
    const double Y = (p.R[3] * dn + p.R[4] * de) + p.R[5] * dd;
    const double Z = (p.R[6] * dn + p.R[7] * de) + p.R[8] * dd;
    const double x = X / Z, y = Y / Z;
    const double r2 = x * x + y * y;
    const double rad = 1 + r2 * (p.k1 + r2 * (p.k2 + r2 * p.k3));
    const double xd = x * rad + 2 * p.p1 * x * y + p.p2 * (r2 + 2 * x * x);
    const double yd = y * rad + p.p1 * (r2 + 2 * y * y) + 2 * p.p2 * x * y;
    o.dn = dn;
    o.de = de;
    o.fu = p.fx * xd + p.cx;
    o.fv = p.fy * yd + p.cy;
    o.Z = Z;
}

// ortho.py's bilinear formula at (fu, fv), both inside the frame
__device__ __forceinline__ void frame_sample(const uint8_t *__restrict__ frame, int h_s, int w_s, double fu, double fv,
                                             double (&val)[3])
{
    const int sx0 = (int)fu, sy0 = (int)fv;
    const int sx1 = min(sx0 + 1, w_s - 1), sy1 = min(sy0 + 1, h_s - 1);
    const double stx = fu - (double)sx0, sty = fv - (double)sy0;
    const uint8_t *t00 = frame + ((int64_t)sy0 * w_s + sx0) * 3, *t01 = frame + ((int64_t)sy0 * w_s + sx1) * 3;
    const uint8_t *t10 = frame + ((int64_t)sy1 * w_s + sx0) * 3, *t11 = frame + ((int64_t)sy1 * w_s + sx1) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double a = lerp((double)t00[ch], (double)t01[ch], stx);
        const double b = lerp((double)t10[ch], (double)t11[ch], stx);
        val[ch] = lerp(a, b, sty);
    }
}

// MODE_OWNER is MODE_BEST without frame and bgr (both may be null): count, metric and index only
template <int MODE>
__global__ __launch_bounds__(THREADS) void dsm_kernel(const float *__restrict__ dsm, int H, int W, int ss, DsmParams p,
                                                      const uint8_t *__restrict__ frame, int h_s, int w_s,
                                                      int image_index, int c0, int r0, int c1, int r1,
                                                      double *__restrict__ acc, int32_t *__restrict__ index,
                                                      uint16_t *__restrict__ count, uint8_t *__restrict__ bgr)
{
    const int tid = threadIdx.x;
    const int col = c0 + TILE * (int)blockIdx.x + (tid & (TILE - 1));
    const int row = r0 + TILE * (int)blockIdx.y + (tid >> 4);
    if (col > c1 || row > r1) return;                  // (no barrier in this kernel)

    // ---- height, projection, cover ----
    const double pc = (double)col + 0.5, pr = (double)row + 0.5;
    double px, py;
    const double h = pixel_height(dsm, H, W, p, pc, pr, px, py);
    if (h != h) return;                                // a hole: uncovered for every image
    Projected v;
    project(p, pc, pr, h, v);
    const double dn = v.dn, de = v.de, Z = v.Z, fu = v.fu, fv = v.fv;
    if (!(Z > 0.0 && fu >= 0.0 && fu <= (double)(w_s - 1) && fv >= 0.0 && fv <= (double)(h_s - 1))) return;
    const double dh = (-p.C[2]) - h;
    if (!(dh > 0.0)) return;

    // ---- visibility: the height field between the point and the camera ----
    const double dx = p.qx - px, dy = p.qy - py;
    const double L = fmax(fabs(dx), fabs(dy));
    const int bound = max(H, W);
    for (int i = 1; i <= bound && (double)i <= L; ++i) {
        const double t = (double)i / L;
        const double cx_ = floor(px + dx * t), cy_ = floor(py + dy * t);
        if (!(cx_ >= 0.0 && cx_ <= (double)(W - 1) && cy_ >= 0.0 && cy_ <= (double)(H - 1))) break;
        const double hr = h + dh * t;
        if (hr > p.zmax) break;
        if ((double)dsm[(int64_t)(int)cy_ * W + (int)cx_] > hr + p.bias) return;       // occluded (false for a NaN)
    }

    // ---- composition ----
    const int64_t q = (int64_t)row * ((int64_t)W * ss) + col;
    const uint16_t seen = count[q];
    count[q] = (uint16_t)(seen < 65535 ? seen + 1 : 65535);
    if (MODE != MODE_FEATHER) {
        const double m = (dn * dn + de * de) / (dh * dh);
        if (!(m < acc[q])) return;                     // (a tie: the earlier image keeps the pixel)
        acc[q] = m;
        index[q] = image_index;
    }

    if (MODE == MODE_OWNER) return;

    // ---- sample ----
    double val[3];
    frame_sample(frame, h_s, w_s, fu, fv, val);

    if (MODE == MODE_BEST) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) bgr[3 * q + ch] = round_u8(val[ch]);
    } else {
        const double d = fmin(fmin(fu, (double)(w_s - 1) - fu), fmin(fv, (double)(h_s - 1) - fv));
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

// the layer of image k for mode multiband's pyramids: C_k where the image covers the pixel, seen or
// not (the owner already keeps an occluded view out of the full resolution; what its coarse bands
// bring across a seam is low-frequency colour, and a zero inside the occlusion shadow would take the
// blend out of the range of the inputs), A_k where it owns it; every pixel of the box is written
__global__ __launch_bounds__(THREADS) void layer_kernel(const float *__restrict__ dsm, int H, int W, int ss, DsmParams p,
                                                        const uint8_t *__restrict__ frame, int h_s, int w_s,
                                                        int image_index, int c0, int r0, int c1, int r1,
                                                        const int32_t *__restrict__ index, float4 *__restrict__ layer)
{
    const int tid = threadIdx.x;
    const int col = c0 + TILE * (int)blockIdx.x + (tid & (TILE - 1));
    const int row = r0 + TILE * (int)blockIdx.y + (tid >> 4);
    if (col > c1 || row > r1) return;

    const double pc = (double)col + 0.5, pr = (double)row + 0.5;
    double px, py;
    const double h = pixel_height(dsm, H, W, p, pc, pr, px, py);
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    Projected v;
    project(p, pc, pr, h, v);                          // (of a hole: NaN, which fails the frame test)
    if (v.Z > 0.0 && v.fu >= 0.0 && v.fu <= (double)(w_s - 1) && v.fv >= 0.0 && v.fv <= (double)(h_s - 1) &&
        (-p.C[2]) - h > 0.0) {
        double val[3];
        frame_sample(frame, h_s, w_s, v.fu, v.fv, val);
        out.x = (float)val[0];
        out.y = (float)val[1];
        out.z = (float)val[2];
    }
    out.w = index[(int64_t)row * ((int64_t)W * ss) + col] == image_index ? 1.0f : 0.0f;
    layer[(int64_t)(row - r0) * (c1 - c0 + 1) + (col - c0)] = out;
}

// one round of the hole fill (dense.py, "fill"); round 0 only sorts the cells into measured and empty
__global__ __launch_bounds__(THREADS) void fill_kernel(const float *__restrict__ src, const uint8_t *__restrict__ round_src,
                                                       int W, int H, int round, float *__restrict__ dst,
                                                       uint8_t *__restrict__ round_dst)
{
    const int64_t g = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (g >= (int64_t)W * H) return;
    const float v = src[g];
    if (round == 0) {
        dst[g] = v;
        round_dst[g] = isfinite(v) ? 0 : 255;
        return;
    }
    if (isfinite(v)) {
        dst[g] = v;
        round_dst[g] = round_src[g];
        return;
    }
    const int r = (int)(g / W), c = (int)(g - (int64_t)r * W);
    float sum = 0.0f;
    int n = 0;
    for (int dy = -1; dy <= 1; ++dy) {
        const int y = r + dy;
        if (y < 0 || y >= H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int x = c + dx;
            if (x < 0 || x >= W || (dx == 0 && dy == 0)) continue;
            const float u = src[(int64_t)y * W + x];
            if (!isfinite(u)) continue;
            sum = n ? sum + u : u;
            ++n;
        }
    }
    dst[g] = n ? (float)((double)sum / (double)n) : v;
    round_dst[g] = n ? (uint8_t)round : 255;
}

inline bool aligned32(const void *p) { return ((uintptr_t)p & 31) == 0; }

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// what the three per-image entry points share: sizes, the work box, the parameters -> the kernels'
// DsmParams and the grid.  Returns what is wrong, or null; `empty` for a box without a pixel.
const char *image_args(int H, int W, int ss, const double *params, int h_s, int w_s, int c0, int r0, int c1, int r1,
                       DsmParams &p, dim3 &grid, bool &empty)
{
    empty = false;
    if (!(ss >= 1 && ss <= IAMX_ORTHO_DSM_MAX_UPSAMPLE)) return "upsample out of range (1 .. 8)";
    if (!(H >= 1 && W >= 1 && (int64_t)H * ss <= MAX_SIDE && (int64_t)W * ss <= MAX_SIDE))
        return "mosaic sides out of range (1 .. 2^20)";
    if (!(h_s >= 2 && w_s >= 2)) return "a frame is at least 2 x 2";
    if (c1 < c0 || r1 < r0) {                          // an empty box: no launch
        empty = true;
        return nullptr;
    }
    if (!(c0 >= 0 && r0 >= 0 && c1 < W * ss && r1 < H * ss)) return "the image's work box leaves the mosaic";
    p.x0 = params[0]; p.y1 = params[1]; p.gsd = params[2]; p.bias = params[3]; p.zmax = params[4];
    for (int i = 0; i < 9; ++i) p.R[i] = params[5 + i];
    for (int i = 0; i < 3; ++i) p.C[i] = params[14 + i];
    p.fx = params[17]; p.fy = params[18]; p.cx = params[19]; p.cy = params[20];
    p.k1 = params[21]; p.k2 = params[22]; p.p1 = params[23]; p.p2 = params[24]; p.k3 = params[25];
    for (int i = 0; i < PARAMS; ++i)
        if (!isfinite(params[i])) return "a parameter is not finite";
    if (!(p.gsd > 0.0 && p.bias >= 0.0)) return "gsd > 0 and bias >= 0 wanted";
    p.ss = (double)ss;
    p.g = p.gsd / p.ss;
    p.qx = (p.C[1] - p.x0) / p.gsd;
    p.qy = (p.y1 - p.C[0]) / p.gsd;
    p.half = 0.5 * fmin((double)(w_s - 1), (double)(h_s - 1));
    grid = dim3((c1 - c0) / TILE + 1, (r1 - r0) / TILE + 1);
    if (grid.y > 65535) return "the image's work box is too tall for one launch";
    return nullptr;
}

}  // namespace

extern "C" int iamx_ortho_dsm_image(int mode, const float *dsm, int H, int W, int ss, const double *params,
                                    const uint8_t *frame, int h_s, int w_s, int image_index, int c0, int r0, int c1,
                                    int r1, double *acc, int32_t *index, uint16_t *count, uint8_t *bgr, void *stream)
{
    IAMX_REQUIRE(mode == MODE_BEST || mode == MODE_FEATHER, "mode must be 0 (best) or 1 (feather)");
    IAMX_REQUIRE(dsm && params && frame, "null pointer");
    IAMX_REQUIRE(acc && count && bgr && (mode == MODE_FEATHER || index), "null pointer");
    IAMX_REQUIRE(mode == MODE_BEST || aligned32(acc), "the feather accumulator must be 32-byte aligned");
    DsmParams p;
    dim3 grid;
    bool empty;
    const char *bad = image_args(H, W, ss, params, h_s, w_s, c0, r0, c1, r1, p, grid, empty);
    IAMX_REQUIRE(!bad, bad);
    if (empty) return IAMX_OK;
    hipStream_t st = iamx::as_stream(stream);
    if (mode == MODE_BEST)
        hipLaunchKernelGGL(dsm_kernel<MODE_BEST>, grid, dim3(THREADS), 0, st, dsm, H, W, ss, p, frame, h_s, w_s,
                           image_index, c0, r0, c1, r1, acc, index, count, bgr);
    else
        hipLaunchKernelGGL(dsm_kernel<MODE_FEATHER>, grid, dim3(THREADS), 0, st, dsm, H, W, ss, p, frame, h_s, w_s,
                           image_index, c0, r0, c1, r1, acc, index, count, bgr);
    return iamx::check_launch("iamx_ortho_dsm_image");
}

// ---- mode multiband over the dense surface (the rules: imageanalysis_amd/ortho.py) ----
extern "C" int iamx_ortho_dsm_owner(const float *dsm, int H, int W, int ss, const double *params, int h_s, int w_s,
                                    int image_index, int c0, int r0, int c1, int r1, double *metric, int32_t *index,
                                    uint16_t *count, void *stream)
{
    IAMX_REQUIRE(dsm && params && metric && index && count, "null pointer");
    DsmParams p;
    dim3 grid;
    bool empty;
    const char *bad = image_args(H, W, ss, params, h_s, w_s, c0, r0, c1, r1, p, grid, empty);
    IAMX_REQUIRE(!bad, bad);
    if (empty) return IAMX_OK;
    hipLaunchKernelGGL(dsm_kernel<MODE_OWNER>, grid, dim3(THREADS), 0, iamx::as_stream(stream), dsm, H, W, ss, p,
                       (const uint8_t *)nullptr, h_s, w_s, image_index, c0, r0, c1, r1, metric, index, count,
                       (uint8_t *)nullptr);
    return iamx::check_launch("iamx_ortho_dsm_owner");
}

extern "C" int iamx_ortho_dsm_layer(const float *dsm, int H, int W, int ss, const double *params, const uint8_t *frame,
                                    int h_s, int w_s, int image_index, int c0, int r0, int c1, int r1,
                                    const int32_t *index, float *layer, void *stream)
{
    IAMX_REQUIRE(dsm && params && frame && index && layer, "null pointer");
    IAMX_REQUIRE(aligned16(layer), "the layer must be 16-byte aligned");
    DsmParams p;
    dim3 grid;
    bool empty;
    const char *bad = image_args(H, W, ss, params, h_s, w_s, c0, r0, c1, r1, p, grid, empty);
    IAMX_REQUIRE(!bad, bad);
    if (empty) return IAMX_OK;
    hipLaunchKernelGGL(layer_kernel, grid, dim3(THREADS), 0, iamx::as_stream(stream), dsm, H, W, ss, p, frame, h_s, w_s,
                       image_index, c0, r0, c1, r1, index, reinterpret_cast<float4 *>(layer));
    return iamx::check_launch("iamx_ortho_dsm_layer");
}

extern "C" int iamx_dense_fill(const float *src, const uint8_t *round_src, int width, int height, int round,
                               float *dst, uint8_t *round_dst, void *stream)
{
    IAMX_REQUIRE(width >= 1 && height >= 1 && width <= IAMX_DENSE_MAX_RASTER && height <= IAMX_DENSE_MAX_RASTER,
                 "raster size out of range");
    IAMX_REQUIRE(round >= 0 && round <= 254, "round out of range (0 .. 254)");
    IAMX_REQUIRE(src && dst && round_dst && (round == 0 || round_src), "null pointer");
    IAMX_REQUIRE(src != dst && round_src != round_dst, "a round reads one raster and writes another");
    const int64_t cells = (int64_t)width * height;
    IAMX_REQUIRE(cells < ((int64_t)1 << 31) * THREADS, "too many cells for one launch");
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((cells + THREADS - 1) / THREADS)), dim3(THREADS), 0,
                       iamx::as_stream(stream), src, round_src, width, height, round, dst, round_dst);
    return iamx::check_launch("iamx_dense_fill");
}
