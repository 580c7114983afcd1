// Colour tables of the explorer (gfx950): what the reference computes on the host with
//   scripts/lib/histogram.py   per-image B/G/R histograms, look-up tables applied at view time
//   scripts/99-vignette.py     the survey's mean frame, a radial a r^4 + b r^2 + c fit, the mask
// for interleaved uint8 frames [h][w][3] in the decoder's channel order.
//
// An interleaved frame is read 48 bytes (16 pixels, three 16-byte loads) per lane and step: byte k
// of such a piece belongs to channel k % 3 whatever the piece's number.  An image whose pointers
// are not 16-byte aligned, and the bytes behind the last whole piece, go through a byte-wise loop
// of the same kernel.
//
// Counters are integers everywhere (a float counter stops at 2^24; a flat 20 MP frame puts
// 19 961 856 pixels into one bin).  The floating-point sums (the radial moments) are doubles,
// reduced in a fixed order: a fixed grid, a fixed tree per workgroup, the workgroups' partials
// added in index order by one lane per value.  No floating-point atomics.
#include <math.h>

#include "iamx_common.h"

// The moments and the mask restate Python expressions operation by operation (dx*dx + dy*dy,
// a*x*x*x*x + b*x*x + c): build.sh passes -ffp-contract=off for this file as well.
#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int MAX_GRID = 2048;            // 8 workgroups per CU: every kernel here is a grid-stride loop

// ---- histogram -------------------------------------------------------------------------------
constexpr int HIST_COPIES = 16;           // one per 16 lanes: a flat image meets 16 lanes per address
constexpr int HIST_STRIDE = 3 * 256 + 1;  // (+1: the copies' equal bins fall on different banks)

constexpr int ACC_MAX_FRAMES = 8;
struct FrameList {
    const uint8_t *p[ACC_MAX_FRAMES];
};

constexpr int MOM_BLOCKS = 512;           // fixed: the summation order does not depend on the device
constexpr int MOM_VALUES = 14;            // s8 s6 s4 s2 n, then (s4 v, s2 v, v) per channel

struct MaskCoef {
    double c[3][3];                       // per channel a, b, c
};

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

inline int grid_for(int64_t items)
{
    int64_t g = (items + THREADS - 1) / THREADS;
    if (g < 1) g = 1;
    return (int)(g < MAX_GRID ? g : MAX_GRID);
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t *w, int k) { return (w[k >> 2] >> (8 * (k & 3))) & 255u; }

__device__ __forceinline__ void load48(const uint4 *p, int64_t g, uint32_t *w)
{
    const uint4 a = p[3 * g], b = p[3 * g + 1], c = p[3 * g + 2];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
    w[8] = c.x; w[9] = c.y; w[10] = c.z; w[11] = c.w;
}

__device__ __forceinline__ void store48(uint4 *p, int64_t g, const uint32_t *w)
{
    p[3 * g] = make_uint4(w[0], w[1], w[2], w[3]);
    p[3 * g + 1] = make_uint4(w[4], w[5], w[6], w[7]);
    p[3 * g + 2] = make_uint4(w[8], w[9], w[10], w[11]);
}

// n_pieces whole 48-byte pieces (0 for an unaligned image), then bytes [48 n_pieces, n_values)
__global__ __launch_bounds__(THREADS) void hist_kernel(const uint8_t *__restrict__ img, int64_t n_pieces,
                                                       int64_t n_values, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t bins[HIST_COPIES * HIST_STRIDE];
    for (int i = threadIdx.x; i < HIST_COPIES * HIST_STRIDE; i += THREADS) bins[i] = 0u;
    __syncthreads();
    uint32_t *mine = bins + (threadIdx.x >> 4) * HIST_STRIDE;
    const int64_t tid = (int64_t)blockIdx.x * THREADS + threadIdx.x, step = (int64_t)gridDim.x * THREADS;
    const uint4 *p = reinterpret_cast<const uint4 *>(img);
    for (int64_t g = tid; g < n_pieces; g += step) {
        uint32_t w[12];
        load48(p, g, w);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // equal neighbours are counted first and added once
            uint32_t prev = byte_of(w, c), run = 1u;
#pragma unroll
            for (int j = 1; j < 16; ++j) {
                const uint32_t v = byte_of(w, 3 * j + c);
                if (v == prev) {
                    ++run;
                } else {
                    atomicAdd(mine + c * 256 + prev, run);
                    prev = v;
                    run = 1u;
                }
            }
            atomicAdd(mine + c * 256 + prev, run);
        }
    }
    for (int64_t i = 48 * n_pieces + tid; i < n_values; i += step)
        atomicAdd(mine + (int)(i % 3) * 256 + img[i], 1u);
    __syncthreads();
    for (int b = threadIdx.x; b < 3 * 256; b += THREADS) {
        uint32_t s = 0u;
#pragma unroll
        for (int k = 0; k < HIST_COPIES; ++k) s += bins[k * HIST_STRIDE + b];
        if (s) atomicAdd(hist + b, s);
    }
}

// ---- frame accumulation and mean -------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void accumulate_kernel(FrameList fl, int n_frames, int64_t n_pieces,
                                                             int64_t n_values, uint32_t *__restrict__ sum)
{
    const int64_t tid = (int64_t)blockIdx.x * THREADS + threadIdx.x, step = (int64_t)gridDim.x * THREADS;
    uint4 *s4 = reinterpret_cast<uint4 *>(sum);
    for (int64_t g = tid; g < n_pieces; g += step) {          // 16 values: 16 bytes per frame, 64 of the sum
        uint4 acc[4] = {s4[4 * g], s4[4 * g + 1], s4[4 * g + 2], s4[4 * g + 3]};
#pragma unroll
        for (int k = 0; k < ACC_MAX_FRAMES; ++k) {
            if (k < n_frames) {
                const uint4 v = reinterpret_cast<const uint4 *>(fl.p[k])[g];
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc[q].x += w[q] & 255u;
                    acc[q].y += (w[q] >> 8) & 255u;
                    acc[q].z += (w[q] >> 16) & 255u;
                    acc[q].w += w[q] >> 24;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) s4[4 * g + q] = acc[q];
    }
    for (int64_t i = 16 * n_pieces + tid; i < n_values; i += step) {
        uint32_t a = sum[i];
#pragma unroll
        for (int k = 0; k < ACC_MAX_FRAMES; ++k)
            if (k < n_frames) a += fl.p[k][i];
        sum[i] = a;
    }
}

__device__ __forceinline__ uint32_t mean_of(uint32_t s, float count)
{
    // numpy: (float32(sum) / float32(count)).astype(uint8) -- one correctly rounded division, truncation
    const float q = __fdiv_rn((float)s, count);
    return (uint32_t)(int)q & 255u;
}

__global__ __launch_bounds__(THREADS) void mean_kernel(const uint32_t *__restrict__ sum, int64_t n_pieces,
                                                       int64_t n_values, float count, uint8_t *__restrict__ avg)
{
    const int64_t tid = (int64_t)blockIdx.x * THREADS + threadIdx.x, step = (int64_t)gridDim.x * THREADS;
    const uint4 *s4 = reinterpret_cast<const uint4 *>(sum);
    for (int64_t g = tid; g < n_pieces; g += step) {
        uint32_t o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 v = s4[4 * g + q];
            o[q] = mean_of(v.x, count) | mean_of(v.y, count) << 8 | mean_of(v.z, count) << 16
                   | mean_of(v.w, count) << 24;
        }
        reinterpret_cast<uint4 *>(avg)[g] = make_uint4(o[0], o[1], o[2], o[3]);
    }
    for (int64_t i = 16 * n_pieces + tid; i < n_values; i += step) avg[i] = (uint8_t)mean_of(sum[i], count);
}

// ---- radial moments --------------------------------------------------------------------------
// the reference's radius table is float32: r = double(float(sqrt(dx*dx + dy*dy)))
__host__ __device__ __forceinline__ double radius_f32(double dx, double dy)
{
    return (double)(float)sqrt(dx * dx + dy * dy);
}

__global__ __launch_bounds__(THREADS) void moments_kernel(const uint8_t *__restrict__ img, int h, int w,
                                                          double cu, double cv, double R,
                                                          double *__restrict__ partials)
{
    __shared__ double red[THREADS];
    double a[MOM_VALUES];
#pragma unroll
    for (int k = 0; k < MOM_VALUES; ++k) a[k] = 0.0;
    const int64_t n = (int64_t)h * w;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)MOM_BLOCKS * THREADS) {
        const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
        const double s = radius_f32(x - cu, y - cv) / R;
        const double s2 = s * s, s4 = s2 * s2;
        a[0] += s4 * s4;
        a[1] += s4 * s2;
        a[2] += s4;
        a[3] += s2;
        a[4] += 1.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = (double)img[3 * i + c];
            a[5 + 3 * c] += s4 * v;
            a[6 + 3 * c] += s2 * v;
            a[7 + 3 * c] += v;
        }
    }
#pragma unroll
    for (int k = 0; k < MOM_VALUES; ++k) {
        __syncthreads();
        red[threadIdx.x] = a[k];
        __syncthreads();
        for (int half = THREADS / 2; half > 0; half >>= 1) {
            if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
            __syncthreads();
        }
        if (threadIdx.x == 0) partials[blockIdx.x * MOM_VALUES + k] = red[0];
    }
}

__global__ void moments_finish_kernel(const double *__restrict__ partials, double *__restrict__ out)
{
    __shared__ double tot[MOM_VALUES];
    if (threadIdx.x < MOM_VALUES) {
        double s = 0.0;
        for (int b = 0; b < MOM_BLOCKS; ++b) s += partials[b * MOM_VALUES + threadIdx.x];
        tot[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x < 24) {
        const int c = threadIdx.x >> 3, k = threadIdx.x & 7;
        out[threadIdx.x] = k < 5 ? tot[k] : tot[5 + 3 * c + (k - 5)];
    }
}

// ---- fitted mask -----------------------------------------------------------------------------
// a*x*x*x*x + b*x*x + c as Python evaluates it, left to right
__host__ __device__ __forceinline__ double f4(double x, double a, double b, double c)
{
    return a * x * x * x * x + b * x * x + c;
}

// uniform in [0, 1) from (seed, value index): splitmix64's finaliser over a Weyl step, 53 bits
__device__ __forceinline__ double uniform01(uint64_t seed, uint64_t index)
{
    uint64_t z = seed + (index + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1.0p-53;
}

__global__ __launch_bounds__(THREADS) void fit_mask_kernel(int h, int w, double cu, double cv, MaskCoef k,
                                                           uint64_t seed, uint8_t *__restrict__ out)
{
    const int64_t n = (int64_t)h * w;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
        const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
        const double dx = x - cu, dy = y - cv;
        const double rad = sqrt(dx * dx + dy * dy);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = f4(rad, k.c[c][0], k.c[c][1], k.c[c][2]);
            // the reference's dither: int(x), plus one with probability x - int(x)
            int q = (int)v;
            if (uniform01(seed, (uint64_t)(3 * i + c)) < v - (double)q) ++q;
            out[3 * i + c] = (uint8_t)(q < 0 ? 0 : (q > 255 ? 255 : q));    // (the host refused what leaves 0..255)
        }
    }
}

// ---- mask finish -----------------------------------------------------------------------------
// m = 255 - v, m -= min(m)  ==  max(v) - v per channel
__global__ __launch_bounds__(THREADS) void channel_max_kernel(const uint8_t *__restrict__ img, int64_t n_pixels,
                                                              uint32_t *__restrict__ chan_max)
{
    __shared__ uint32_t top[3];
    if (threadIdx.x < 3) top[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t m[3] = {0u, 0u, 0u};
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n_pixels; i += (int64_t)gridDim.x * THREADS) {
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = max(m[c], (uint32_t)img[3 * i + c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) atomicMax(top + c, m[c]);
    __syncthreads();
    if (threadIdx.x < 3) atomicMax(chan_max + threadIdx.x, top[threadIdx.x]);
}

__global__ __launch_bounds__(THREADS) void mask_finish_kernel(const uint8_t *__restrict__ img, int64_t n_pixels,
                                                              const uint32_t *__restrict__ chan_max,
                                                              uint8_t *__restrict__ out)
{
    const uint32_t m0 = chan_max[0], m1 = chan_max[1], m2 = chan_max[2];
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n_pixels; i += (int64_t)gridDim.x * THREADS) {
        out[3 * i] = (uint8_t)(m0 - img[3 * i]);
        out[3 * i + 1] = (uint8_t)(m1 - img[3 * i + 1]);
        out[3 * i + 2] = (uint8_t)(m2 - img[3 * i + 2]);
    }
}

// ---- look-up ---------------------------------------------------------------------------------
template <bool MASK>
__global__ __launch_bounds__(THREADS) void lut_kernel(const uint8_t *__restrict__ img, int64_t n_pieces,
                                                      int64_t n_values, const uint8_t *__restrict__ lut,
                                                      const uint8_t *__restrict__ mask, uint8_t *__restrict__ out)
{
    __shared__ uint8_t table[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += THREADS) table[i] = lut[i];
    __syncthreads();
    const int64_t tid = (int64_t)blockIdx.x * THREADS + threadIdx.x, step = (int64_t)gridDim.x * THREADS;
    for (int64_t g = tid; g < n_pieces; g += step) {
        uint32_t w[12], m[12], o[12];
        load48(reinterpret_cast<const uint4 *>(img), g, w);
        if (MASK) load48(reinterpret_cast<const uint4 *>(mask), g, m);
#pragma unroll
        for (int q = 0; q < 12; ++q) o[q] = 0u;
#pragma unroll
        for (int k = 0; k < 48; ++k) {
            uint32_t v = table[(k % 3) * 256 + byte_of(w, k)];
            if (MASK) v = min(v + byte_of(m, k), 255u);
            o[k >> 2] |= v << (8 * (k & 3));
        }
        store48(reinterpret_cast<uint4 *>(out), g, o);
    }
    for (int64_t i = 48 * n_pieces + tid; i < n_values; i += step) {
        uint32_t v = table[(int)(i % 3) * 256 + img[i]];
        if (MASK) v = min(v + (uint32_t)mask[i], 255u);
        out[i] = (uint8_t)v;
    }
}

}  // namespace

extern "C" int iamx_colour_histogram(const uint8_t *img, int64_t n_pixels, uint32_t *hist, void *stream)
{
    IAMX_REQUIRE(img && hist, "null pointer");
    IAMX_REQUIRE(n_pixels >= 1 && n_pixels < (1ll << 32), "pixel count out of range (a bin is 32 bits)");
    const int64_t n_values = 3 * n_pixels;
    const int64_t n_pieces = aligned16(img) ? n_values / 48 : 0;
    const int64_t lanes = n_pieces ? n_pieces + (n_values - 48 * n_pieces) : n_values;
    hipLaunchKernelGGL(hist_kernel, dim3(grid_for(lanes)), dim3(THREADS), 0, iamx::as_stream(stream), img,
                       n_pieces, n_values, hist);
    return iamx::check_launch("iamx_colour_histogram");
}

extern "C" int iamx_colour_accumulate_max_frames(void) { return ACC_MAX_FRAMES; }

extern "C" int iamx_colour_accumulate(const uint8_t *const *frames, int n_frames, int64_t n_values,
                                      uint32_t *sum, void *stream)
{
    IAMX_REQUIRE(frames && sum, "null pointer");
    IAMX_REQUIRE(n_frames >= 1 && n_frames <= ACC_MAX_FRAMES, "1 to 8 frames per launch");
    IAMX_REQUIRE(n_values >= 1, "empty image");
    FrameList fl;
    bool wide = aligned16(sum);
    for (int k = 0; k < ACC_MAX_FRAMES; ++k) {
        fl.p[k] = k < n_frames ? frames[k] : nullptr;
        if (k < n_frames) {
            IAMX_REQUIRE(frames[k], "null frame pointer");
            wide = wide && aligned16(frames[k]);
        }
    }
    const int64_t n_pieces = wide ? n_values / 16 : 0;
    hipLaunchKernelGGL(accumulate_kernel, dim3(grid_for(wide ? n_pieces + 16 : n_values)), dim3(THREADS), 0,
                       iamx::as_stream(stream), fl, n_frames, n_pieces, n_values, sum);
    return iamx::check_launch("iamx_colour_accumulate");
}

extern "C" int iamx_colour_mean(const uint32_t *sum, int64_t n_values, int count, uint8_t *avg, void *stream)
{
    IAMX_REQUIRE(sum && avg, "null pointer");
    IAMX_REQUIRE(n_values >= 1, "empty image");
    // 255 * count < 2^24: the reference's float32 sum is exact up to there, and so is float(sum) here
    IAMX_REQUIRE(count >= 1 && count <= 65793, "count must be 1 .. 65793 (255 * count < 2^24)");
    const int64_t n_pieces = aligned16(sum) && aligned16(avg) ? n_values / 16 : 0;
    hipLaunchKernelGGL(mean_kernel, dim3(grid_for(n_pieces ? n_pieces + 16 : n_values)), dim3(THREADS), 0,
                       iamx::as_stream(stream), sum, n_pieces, n_values, (float)count, avg);
    return iamx::check_launch("iamx_colour_mean");
}

extern "C" int iamx_colour_moments_workspace_doubles(void) { return MOM_BLOCKS * MOM_VALUES; }

extern "C" int iamx_colour_moments(const uint8_t *img, int height, int width, double cu, double cv,
                                   double *radius, double *partials, double *out, void *stream)
{
    IAMX_REQUIRE(img && radius && partials && out, "null pointer");
    IAMX_REQUIRE(height >= 1 && width >= 1, "empty image");
    IAMX_REQUIRE(isfinite(cu) && isfinite(cv), "principal point is not finite");
    double R = 0.0;
    for (int k = 0; k < 4; ++k) {
        const double r = radius_f32((k & 1 ? width - 1 : 0) - cu, (k & 2 ? height - 1 : 0) - cv);
        R = r > R ? r : R;
    }
    IAMX_REQUIRE(R > 0.0, "a one-pixel image at the principal point has no radius");
    *radius = R;
    hipStream_t st = iamx::as_stream(stream);
    hipLaunchKernelGGL(moments_kernel, dim3(MOM_BLOCKS), dim3(THREADS), 0, st, img, height, width, cu, cv, R,
                       partials);
    hipLaunchKernelGGL(moments_finish_kernel, dim3(1), dim3(64), 0, st, partials, out);
    return iamx::check_launch("iamx_colour_moments");
}

extern "C" int iamx_colour_fit_mask(int height, int width, double cu, double cv, const double *coef,
                                    uint64_t seed, uint8_t *out, void *stream)
{
    IAMX_REQUIRE(coef && out, "null pointer");
    IAMX_REQUIRE(height >= 1 && width >= 1, "empty image");
    IAMX_REQUIRE(isfinite(cu) && isfinite(cv), "principal point is not finite");
    MaskCoef k;
    // the extremes of a t^2 + b t + c over t = r^2 in [tmin, tmax]: the ends and the vertex
    double rmax = 0.0;
    for (int q = 0; q < 4; ++q) {
        const double dx = (q & 1 ? width - 1 : 0) - cu, dy = (q & 2 ? height - 1 : 0) - cv;
        const double r = sqrt(dx * dx + dy * dy);
        rmax = r > rmax ? r : rmax;
    }
    const double nx = fmin(fmax(rint(cu), 0.0), width - 1.0) - cu, ny = fmin(fmax(rint(cv), 0.0), height - 1.0) - cv;
    const double rmin = sqrt(nx * nx + ny * ny);
    for (int c = 0; c < 3; ++c) {
        const double a = coef[3 * c], b = coef[3 * c + 1], c0 = coef[3 * c + 2];
        IAMX_REQUIRE(isfinite(a) && isfinite(b) && isfinite(c0), "coefficient is not finite");
        double lo = fmin(f4(rmin, a, b, c0), f4(rmax, a, b, c0)), hi = fmax(f4(rmin, a, b, c0), f4(rmax, a, b, c0));
        if (a != 0.0) {
            const double t = -b / (2.0 * a);
            if (t > rmin * rmin && t < rmax * rmax) {
                const double v = f4(sqrt(t), a, b, c0);
                lo = fmin(lo, v);
                hi = fmax(hi, v);
            }
        }
        if (lo < 0.0 || hi > 255.0)
            return iamx::fail(IAMX_EINVAL, "iamx_colour_fit_mask: channel %d's polynomial leaves [0, 255] "
                              "inside the image (%.3f .. %.3f)", c, lo, hi);
        k.c[c][0] = a; k.c[c][1] = b; k.c[c][2] = c0;
    }
    hipLaunchKernelGGL(fit_mask_kernel, dim3(grid_for((int64_t)height * width)), dim3(THREADS), 0,
                       iamx::as_stream(stream), height, width, cu, cv, k, seed, out);
    return iamx::check_launch("iamx_colour_fit_mask");
}

extern "C" int iamx_colour_mask_finish(const uint8_t *img, int64_t n_pixels, uint32_t *chan_max, uint8_t *out,
                                       void *stream)
{
    IAMX_REQUIRE(img && chan_max && out, "null pointer");
    IAMX_REQUIRE(n_pixels >= 1, "empty image");
    hipStream_t st = iamx::as_stream(stream);
    if (hipMemsetAsync(chan_max, 0, 3 * sizeof(uint32_t), st) != hipSuccess)
        return iamx::check_launch("iamx_colour_mask_finish");
    hipLaunchKernelGGL(channel_max_kernel, dim3(grid_for(n_pixels)), dim3(THREADS), 0, st, img, n_pixels, chan_max);
    hipLaunchKernelGGL(mask_finish_kernel, dim3(grid_for(n_pixels)), dim3(THREADS), 0, st, img, n_pixels, chan_max,
                       out);
    return iamx::check_launch("iamx_colour_mask_finish");
}

extern "C" int iamx_colour_lut(const uint8_t *img, int64_t n_pixels, const uint8_t *lut, const uint8_t *mask,
                               uint8_t *out, void *stream)
{
    IAMX_REQUIRE(img && lut && out, "null pointer");
    IAMX_REQUIRE(n_pixels >= 1, "empty image");
    const int64_t n_values = 3 * n_pixels;
    const bool wide = aligned16(img) && aligned16(out) && (!mask || aligned16(mask));
    const int64_t n_pieces = wide ? n_values / 48 : 0;
    const dim3 grid(grid_for(wide ? n_pieces + 48 : n_values));
    hipStream_t st = iamx::as_stream(stream);
    if (mask)
        hipLaunchKernelGGL(lut_kernel<true>, grid, dim3(THREADS), 0, st, img, n_pieces, n_values, lut, mask, out);
    else
        hipLaunchKernelGGL(lut_kernel<false>, grid, dim3(THREADS), 0, st, img, n_pieces, n_values, lut, mask, out);
    return iamx::check_launch("iamx_colour_lut");
}
