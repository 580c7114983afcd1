// Area downscale of interleaved uint8 images (gfx950): what the reference's texture step does with
//   cv2.resize(src, (0,0), fx, fy, interpolation=cv2.INTER_AREA)      (scripts/lib/panda3d.py:38-41)
// restated from OpenCV's published area algorithm for uint8 with a float work type; cv2 itself is
// absent, the restatement the kernel is held to bit for bit is tests/area_restatement.py.
//
// Per axis, scale = 1.0 / f (double).  Destination index d covers [d*scale, d*scale + scale):
// a partial first source sample, whole samples, a partial last one, each with a float32 weight
// (area_taps below).  Every contributing source row is first reduced along x into buf (float32,
// taps in order from 0, multiply and add rounded separately), then sum = beta*buf for the first
// row of a destination row and sum += beta*buf for the later ones; the result is sum rounded half
// to even and saturated.  When both scales are integers (within DBL_EPSILON) OpenCV's integer branch
// is taken instead: integer block sum times float32(1/area), (sum + 2) >> 2 for 2 x 2, and
// (float)sum / count for a block that hangs over the right or bottom edge.
//
// One workgroup makes TX destination pixels of one destination row.  The source rows it needs
// are staged in LDS with 16-byte loads (the whole byte range of the tile, so every fetched line
// is used) and the lanes take their taps from LDS: a lane per output (dx, c) reading straight
// from HBM would touch bytes ~3*scale apart across lanes.  The summation order above is kept:
// one lane owns one output from its first tap to its last.
#include <float.h>
#include <math.h>

#include "iamx_common.h"

// The tap arithmetic restates expressions evaluated operation by operation (d*scale, then + scale;
// ssize - d*scale): a contracted multiply-add rounds once where they round twice and moves a floor,
// a 1e-3 test or the last bit of a weight.  build.sh passes -ffp-contract=off for this file as well.
#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int LDS_BUDGET = 32 << 10;      // bytes of staged rows per workgroup (5 workgroups per CU)
constexpr double MAX_SCALE = 4096.0;      // per axis: one destination pixel's row segment fits the budget

struct Taps {
    int first;            // first source index
    int n;                // number of taps, consecutive source samples
    float w_first, w_mid, w_last;
    int has_first, has_last;
};

// computeResizeAreaTab for one destination index
__host__ __device__ __forceinline__ Taps area_taps(int d, double scale, int ssize)
{
    Taps t;
    const double fs1 = d * scale, fs2 = fs1 + scale;
    const double cell = fmin(scale, ssize - fs1);
    int s1 = (int)ceil(fs1), s2 = (int)floor(fs2);
    s2 = s2 < ssize - 1 ? s2 : ssize - 1;
    s1 = s1 < s2 ? s1 : s2;
    t.has_first = s1 - fs1 > 1e-3;
    t.has_last = fs2 - s2 > 1e-3;
    t.w_first = (float)((s1 - fs1) / cell);
    t.w_mid = (float)(1.0 / cell);
    t.w_last = (float)(fmin(fmin(fs2 - s2, 1.0), cell) / cell);
    t.first = t.has_first ? s1 - 1 : s1;
    t.n = t.has_first + (s2 - s1) + t.has_last;
    // (neither can happen for 1 <= scale and d < dsize; they keep every read inside the row)
    if (t.first < 0) { t.first = 0; t.n = 0; t.has_first = t.has_last = 0; }
    if (t.first + t.n > ssize) { t.n = ssize - t.first; t.has_last = 0; }
    return t;
}

__device__ __forceinline__ float tap_weight(const Taps t, int j)
{
    if (j == 0 && t.has_first) return t.w_first;
    if (j == t.n - 1 && t.has_last) return t.w_last;
    return t.w_mid;
}

// rows [y0, y0 + nr) x source columns [x0, x1) -> LDS, in whole 16-byte pieces of the image's memory;
// row r starts at lds + r * stride and its column x0 sits `lead` bytes in (the row's misalignment)
template <int CH>
__device__ __forceinline__ void stage_rows(const uint8_t *__restrict__ src, const uint8_t *src_end, int w,
                                           int y0, int nr, int x0, int x1, int stride, uint4 *lds)
{
    const int per_row = stride >> 4;
    const int seg = (x1 - x0) * CH;
    for (int i = threadIdx.x; i < nr * per_row; i += THREADS) {
        const int r = i / per_row, k = i - r * per_row;
        const uint8_t *p = src + ((int64_t)(y0 + r) * w + x0) * CH;
        const int lead = (int)((uintptr_t)p & 15);
        const uint8_t *q = p - lead + (k << 4);
        if (q >= p + seg) continue;                       // behind the tile's last byte
        uint4 v;
        if (q >= src && q + 16 <= src_end) {
            v = *reinterpret_cast<const uint4 *>(q);
        } else {                                          // the image's first / last piece
            uint32_t d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (q + j >= src && q + j < src_end) d[j >> 2] |= (uint32_t)q[j] << (8 * (j & 3));
            v = make_uint4(d[0], d[1], d[2], d[3]);
        }
        lds[r * per_row + k] = v;
    }
}

__device__ __forceinline__ uint8_t saturate_u8(float f)
{
    f = rintf(f);
    return (uint8_t)(f < 0.f ? 0.f : (f > 255.f ? 255.f : f));
}

template <int CH>
__global__ __launch_bounds__(THREADS) void area_kernel(const uint8_t *__restrict__ src, int h, int w,
                                                       int dh, int dw, double scale_x, double scale_y,
                                                       int tx, int ntiles, int stride, int rows,
                                                       uint8_t *__restrict__ dst)
{
    extern __shared__ uint4 lds[];
    const int tile = blockIdx.x % ntiles, dy = blockIdx.x / ntiles;
    const int dx0 = tile * tx;
    const int ndx = min(tx, dw - dx0);
    const uint8_t *src_end = src + (int64_t)h * w * CH;
    // source columns of the tile: from the first tap of dx0 to the last tap of its last pixel
    const Taps ta = area_taps(dx0, scale_x, w), tb = area_taps(dx0 + ndx - 1, scale_x, w);
    const int x0 = ta.first, x1 = min(w, max(tb.first + tb.n, x0 + 1));
    const Taps ty = area_taps(dy, scale_y, h);
    const int t = threadIdx.x;
    const bool active = t < ndx * CH;
    const int dx = dx0 + t / CH, c = t % CH;
    const Taps tq = area_taps(min(dx, dw - 1), scale_x, w);
    float sum = 0.f;
    for (int r0 = 0; r0 < ty.n; r0 += rows) {
        const int nr = min(rows, ty.n - r0);
        if (r0) __syncthreads();
        stage_rows<CH>(src, src_end, w, ty.first + r0, nr, x0, x1, stride, lds);
        __syncthreads();
        if (!active) continue;
        for (int r = 0; r < nr; ++r) {
            const uint8_t *p = src + ((int64_t)(ty.first + r0 + r) * w + x0) * CH;
            const int lead = (int)((uintptr_t)p & 15);
            const uint8_t *row = reinterpret_cast<const uint8_t *>(lds) + r * stride + lead
                                 + (tq.first - x0) * CH + c;
            float buf = 0.f;
            for (int j = 0; j < tq.n; ++j)
                buf = __fadd_rn(buf, __fmul_rn((float)row[j * CH], tap_weight(tq, j)));
            const float beta = tap_weight(ty, r0 + r);
            sum = r0 + r == 0 ? __fmul_rn(beta, buf) : __fadd_rn(sum, __fmul_rn(beta, buf));
        }
    }
    if (active) dst[((int64_t)dy * dw + dx) * CH + c] = saturate_u8(sum);
}

// both scales integers: integer block sums
template <int CH>
__global__ __launch_bounds__(THREADS) void area_int_kernel(const uint8_t *__restrict__ src, int h, int w,
                                                           int dh, int dw, int sx, int sy, int tx,
                                                           int ntiles, int stride, int rows,
                                                           uint8_t *__restrict__ dst)
{
    extern __shared__ uint4 lds[];
    const int tile = blockIdx.x % ntiles, dy = blockIdx.x / ntiles;
    const int dx0 = tile * tx;
    const int ndx = min(tx, dw - dx0);
    const uint8_t *src_end = src + (int64_t)h * w * CH;
    const int x0 = dx0 * sx, x1 = min(w, (dx0 + ndx) * sx);
    const int y0 = dy * sy, ny = min(sy, h - y0);
    const int t = threadIdx.x;
    const bool active = t < ndx * CH;
    const int dx = dx0 + t / CH, c = t % CH;
    const int nx = active ? min(sx, w - dx * sx) : 0;
    unsigned sum = 0;                                     // 4096 x 4096 x 255 < 2^32
    for (int r0 = 0; r0 < ny; r0 += rows) {
        const int nr = min(rows, ny - r0);
        if (r0) __syncthreads();
        stage_rows<CH>(src, src_end, w, y0 + r0, nr, x0, x1, stride, lds);
        __syncthreads();
        if (!active) continue;
        for (int r = 0; r < nr; ++r) {
            const uint8_t *p = src + ((int64_t)(y0 + r0 + r) * w + x0) * CH;
            const int lead = (int)((uintptr_t)p & 15);
            const uint8_t *row = reinterpret_cast<const uint8_t *>(lds) + r * stride + lead
                                 + (dx * sx - x0) * CH + c;
            for (int j = 0; j < nx; ++j) sum += row[j * CH];
        }
    }
    if (!active) return;
    uint8_t o;
    if (nx == sx && ny == sy) {
        if (sx == 2 && sy == 2) o = (uint8_t)((sum + 2) >> 2);
        else o = saturate_u8(__fmul_rn((float)sum, __fdiv_rn(1.f, (float)(sx * sy))));
    } else {                                              // the block hangs over the image's edge
        o = saturate_u8(__fdiv_rn((float)sum, (float)(nx * ny)));
    }
    dst[((int64_t)dy * dw + dx) * CH + c] = o;
}

inline bool is_integer_scale(double scale, int *iscale)
{
    *iscale = (int)lrint(scale);          // saturate_cast<int>(double)
    return fabs(scale - *iscale) < DBL_EPSILON;
}

// bytes of one staged row of a tile of tx destination pixels: its source bytes, the row's
// misalignment in front, rounded up to whole 16-byte pieces
inline int tile_stride(int tx, double scale, int ch)
{
    const int64_t px = (int64_t)ceil(tx * scale) + 4;
    const int64_t bytes = px * ch + 15;
    return (int)((bytes + 15) / 16 * 16);
}

}  // namespace

extern "C" int iamx_image_area_dims(int height, int width, double fx, double fy, int *out_h, int *out_w)
{
    IAMX_REQUIRE(out_h && out_w, "null pointer");
    IAMX_REQUIRE(height >= 1 && width >= 1 && fx > 0 && fy > 0, "bad size / factor");
    *out_h = (int)lrint(height * fy);
    *out_w = (int)lrint(width * fx);
    return IAMX_OK;
}

extern "C" int iamx_image_resize_area(const uint8_t *src, int height, int width, int channels, double fx,
                                      double fy, uint8_t *out, void *stream)
{
    IAMX_REQUIRE(src && out, "null pointer");
    IAMX_REQUIRE(channels == 1 || channels == 3, "channels must be 1 or 3");
    IAMX_REQUIRE(height >= 1 && width >= 1 && fx > 0 && fy > 0, "bad size / factor");
    const double scale_x = 1.0 / fx, scale_y = 1.0 / fy;
    IAMX_REQUIRE(scale_x >= 1.0 && scale_y >= 1.0, "upscaling is not supported (area downscale only)");
    IAMX_REQUIRE(scale_x <= MAX_SCALE && scale_y <= MAX_SCALE, "scale above 4096");
    int dh, dw;
    iamx_image_area_dims(height, width, fx, fy, &dh, &dw);
    IAMX_REQUIRE(dh >= 1 && dw >= 1, "scaled image is empty");
    IAMX_REQUIRE(dh <= height && dw <= width, "scaled image is larger than the source");
    hipStream_t st = iamx::as_stream(stream);
    int isx, isy;
    const bool fast = is_integer_scale(scale_x, &isx) && is_integer_scale(scale_y, &isy);
    // destination pixels per workgroup: a lane per (dx, c), fewer while one staged row is too long
    int tx = THREADS / channels;
    if (channels == 3) tx = 64;
    while (tx > 1 && tile_stride(tx, scale_x, channels) > LDS_BUDGET) tx >>= 1;
    const int stride = tile_stride(tx, scale_x, channels);
    IAMX_REQUIRE(stride <= LDS_BUDGET, "scale above what one workgroup stages");
    const int need_rows = fast ? isy : (int)ceil(scale_y) + 2;
    int rows = LDS_BUDGET / stride;
    rows = rows < need_rows ? rows : need_rows;
    const int ntiles = (dw + tx - 1) / tx;
    const int64_t grid = (int64_t)ntiles * dh;
    IAMX_REQUIRE(grid < (1ll << 31), "image too large");
    const size_t lds = (size_t)rows * stride;
    if (fast) {
        if (channels == 3)
            hipLaunchKernelGGL(area_int_kernel<3>, dim3((unsigned)grid), dim3(THREADS), lds, st, src, height,
                               width, dh, dw, isx, isy, tx, ntiles, stride, rows, out);
        else
            hipLaunchKernelGGL(area_int_kernel<1>, dim3((unsigned)grid), dim3(THREADS), lds, st, src, height,
                               width, dh, dw, isx, isy, tx, ntiles, stride, rows, out);
    } else {
        if (channels == 3)
            hipLaunchKernelGGL(area_kernel<3>, dim3((unsigned)grid), dim3(THREADS), lds, st, src, height,
                               width, dh, dw, scale_x, scale_y, tx, ntiles, stride, rows, out);
        else
            hipLaunchKernelGGL(area_kernel<1>, dim3((unsigned)grid), dim3(THREADS), lds, st, src, height,
                               width, dh, dw, scale_x, scale_y, tx, ntiles, stride, rows, out);
    }
    return iamx::check_launch("iamx_image_resize_area");
}
