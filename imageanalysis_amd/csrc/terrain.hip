// Terrain under the survey (scripts/lib/srtm.py): the NED elevation grid that srtm.make_interpolator
// builds, read the way scipy.interpolate.RegularGridInterpolator(method='linear', bounds_error=False,
// fill_value=-32768) reads it, and srtm.interpolate_vector (:277-314) for a batch of rays.
//
// Compiled with -ffp-contract=off: the f64 expressions below restate the host's, operation by
// operation (separately rounded multiply and add), so tests/terrain_restatement.py is this file in
// numpy.  A ray that ends at the cap of 25 rounds oscillates and amplifies a last-bit difference; with
// contraction its count and flags could part from the reference's.
//
// One thread per query / per ray.  The terrain of a survey (201 x 201 doubles = 323 KB) stays in L2;
// a look-up is four 8-byte gathers plus the four axis values, and a ray is a chain of up to 26
// dependent look-ups: latency-bound, hidden by occupancy alone.  No LDS, no atomics.
#include <math.h>

#include "iamx_common.h"

namespace {

constexpr int THREADS = 256;
constexpr double FILL = -32768.0;

struct Terrain {
    const double *axis_n;        // [rows] ascending
    const double *axis_e;        // [cols] ascending
    const double *grid;          // [rows][cols]
    int rows, cols;
};

// The interval i with a[i] <= x < a[i + 1] (the last one closed), for x inside [a[0], a[n - 1]].
// linspace axes are not exactly uniform: the guess of a uniform axis, corrected against the values.
__device__ inline int find_interval(const double *__restrict__ a, int n, double x)
{
    const double a0 = a[0];
    const double f = (x - a0) * ((double)(n - 1) / (a[n - 1] - a0));
    int i = f > 0.0 ? (f < (double)(n - 2) ? (int)f : n - 2) : 0;
    while (i > 0 && x < a[i]) --i;
    while (i < n - 2 && x >= a[i + 1]) ++i;
    return i;
}

// RegularGridInterpolator.__call__ for one point: NaN for a NaN coordinate, the fill value outside
// [a[0], a[-1]] on either axis (*outside = 1), else the bilinear blend in scipy's order of operations.
__device__ inline double look_up(const Terrain &T, double n, double e, int *outside)
{
    if (!(n == n) || !(e == e)) return NAN;
    if (n < T.axis_n[0] || n > T.axis_n[T.rows - 1] || e < T.axis_e[0] || e > T.axis_e[T.cols - 1]) {
        *outside = 1;
        return FILL;
    }
    const int i = find_interval(T.axis_n, T.rows, n);
    const int j = find_interval(T.axis_e, T.cols, e);
    const double y0 = (n - T.axis_n[i]) / (T.axis_n[i + 1] - T.axis_n[i]);
    const double y1 = (e - T.axis_e[j]) / (T.axis_e[j + 1] - T.axis_e[j]);
    const double *g = T.grid + (int64_t)i * T.cols + j;
    return g[0] * (1.0 - y0) * (1.0 - y1) + g[1] * (1.0 - y0) * y1 + g[T.cols] * y0 * (1.0 - y1) +
           g[T.cols + 1] * y0 * y1;
}

__global__ __launch_bounds__(THREADS) void heights_kernel(Terrain T, const double *__restrict__ pts, int64_t n,
                                                          double *__restrict__ z)
{
    const int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (q >= n) return;
    int outside = 0;
    z[q] = look_up(T, pts[2 * q], pts[2 * q + 1], &outside);
}

struct RayArgs {
    const double *M;             // [I][9]   body2ned . cam2body . IK   (FROM_UV)
    const double *uv;            // [n][2]   the shared pixel grid       (FROM_UV)
    const double *v;             // [I][n][3] ready vectors              (!FROM_UV)
    const double *ned;           // [I][3]
    int n;
    int64_t total;               // I * n
    double *pts;                 // [I][n][3]
    uint8_t *iters;              // [I][n]
    uint8_t *flags;              // [I][n]
};

template <bool FROM_UV>
__global__ __launch_bounds__(THREADS) void rays_kernel(Terrain T, RayArgs A)
{
    const int64_t g = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (g >= A.total) return;
    const int64_t im = g / A.n;
    const double ned0 = A.ned[im * 3], ned1 = A.ned[im * 3 + 1], ned2 = A.ned[im * 3 + 2];
    double v0, v1, v2;
    if (FROM_UV) {
        // render_panda3d.unit_rays: M . [u, v, 1] over its length
        const int vx = (int)(g - im * A.n);
        const double *M = A.M + im * 9;
        const double u = A.uv[2 * vx], w = A.uv[2 * vx + 1];
        const double q0 = M[0] * u + M[1] * w + M[2] * 1.0;
        const double q1 = M[3] * u + M[4] * w + M[5] * 1.0;
        const double q2 = M[6] * u + M[7] * w + M[8] * 1.0;
        const double len = sqrt(q0 * q0 + q1 * q1 + q2 * q2);
        v0 = q0 / len; v1 = q1 / len; v2 = q2 / len;
    } else {
        v0 = A.v[g * 3]; v1 = A.v[g * 3 + 1]; v2 = A.v[g * 3 + 2];
    }

    double p0 = ned0, p1 = ned1, p2 = ned2;
    int count = 0, outside = 0;
    uint8_t fl = 0;
    if (v2 <= 0.0) {
        fl |= IAMX_TERRAIN_SKY;                       // "always assume camera pose is above ground"
    } else {
        // srtm.interpolate_vector, as written
        double tmp = look_up(T, p0, p1, &outside);
        double ground = (tmp == tmp && tmp > FILL) ? tmp : 0.0;
        double error = fabs(p2 + ground);
        while (error > 0.01 && count < 25) {
            const double d_proj = -(ned2 + ground);
            const double factor = d_proj / v2;
            const double n_proj = v0 * factor;
            const double e_proj = v1 * factor;
            p0 = ned0 + n_proj;
            p1 = ned1 + e_proj;
            p2 = ned2 + d_proj;
            tmp = look_up(T, p0, p1, &outside);
            if (tmp == tmp && tmp > FILL) ground = tmp;
            error = fabs(p2 + ground);
            ++count;
        }
        if (count >= 25 && error > 0.01) fl |= IAMX_TERRAIN_CAPPED;
        if (outside) fl |= IAMX_TERRAIN_LEFT_GRID;
    }
    A.pts[g * 3] = p0;
    A.pts[g * 3 + 1] = p1;
    A.pts[g * 3 + 2] = p2;
    A.iters[g] = (uint8_t)count;
    A.flags[g] = fl;
}

int make_terrain(Terrain *T, const double *axis_n, int rows, const double *axis_e, int cols, const double *grid)
{
    T->axis_n = axis_n;
    T->axis_e = axis_e;
    T->grid = grid;
    T->rows = rows;
    T->cols = cols;
    return 0;
}

template <bool FROM_UV>
int launch_rays(const Terrain &T, const double *M, const double *uv, const double *v, const double *ned,
                int num_images, int num_rays, double *pts, uint8_t *iters, uint8_t *flags, void *stream,
                const char *what)
{
    RayArgs A;
    A.M = M;
    A.uv = uv;
    A.v = v;
    A.ned = ned;
    A.n = num_rays;
    A.total = (int64_t)num_images * num_rays;
    A.pts = pts;
    A.iters = iters;
    A.flags = flags;
    const unsigned blocks = (unsigned)((A.total + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(rays_kernel<FROM_UV>, dim3(blocks), dim3(THREADS), 0, iamx::as_stream(stream), T, A);
    return iamx::check_launch(what);
}

}  // namespace

#define TERRAIN_REQUIRE_GRID()                                                                    \
    IAMX_REQUIRE(axis_n && axis_e && grid, "null pointer");                                       \
    IAMX_REQUIRE(rows >= 2 && cols >= 2 && rows <= IAMX_TERRAIN_MAX_AXIS && cols <= IAMX_TERRAIN_MAX_AXIS, \
                 "a terrain axis has 2 to IAMX_TERRAIN_MAX_AXIS nodes")

extern "C" int iamx_terrain_heights(const double *axis_n, int rows, const double *axis_e, int cols,
                                    const double *grid, const double *pts, int64_t num_points, double *z,
                                    void *stream)
{
    TERRAIN_REQUIRE_GRID();
    IAMX_REQUIRE(num_points >= 0 && num_points < ((int64_t)1 << 31) * THREADS, "bad point count");
    if (num_points == 0) return IAMX_OK;
    IAMX_REQUIRE(pts && z, "null pointer");
    Terrain T;
    make_terrain(&T, axis_n, rows, axis_e, cols, grid);
    const unsigned blocks = (unsigned)((num_points + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(heights_kernel, dim3(blocks), dim3(THREADS), 0, iamx::as_stream(stream), T, pts,
                       num_points, z);
    return iamx::check_launch("iamx_terrain_heights");
}

extern "C" int iamx_terrain_rays(const double *axis_n, int rows, const double *axis_e, int cols,
                                 const double *grid, const double *M, const double *ned, int num_images,
                                 const double *uv, int num_rays, double *pts, uint8_t *iters, uint8_t *flags,
                                 void *stream)
{
    TERRAIN_REQUIRE_GRID();
    IAMX_REQUIRE(num_images >= 0 && num_rays >= 1, "bad size");
    IAMX_REQUIRE((int64_t)num_images * num_rays < ((int64_t)1 << 31), "too many rays for one call");
    if (num_images == 0) return IAMX_OK;
    IAMX_REQUIRE(M && ned && uv && pts && iters && flags, "null pointer");
    Terrain T;
    make_terrain(&T, axis_n, rows, axis_e, cols, grid);
    return launch_rays<true>(T, M, uv, nullptr, ned, num_images, num_rays, pts, iters, flags, stream,
                             "iamx_terrain_rays");
}

extern "C" int iamx_terrain_rays_vec(const double *axis_n, int rows, const double *axis_e, int cols,
                                     const double *grid, const double *v, const double *ned, int num_images,
                                     int num_rays, double *pts, uint8_t *iters, uint8_t *flags, void *stream)
{
    TERRAIN_REQUIRE_GRID();
    IAMX_REQUIRE(num_images >= 0 && num_rays >= 1, "bad size");
    IAMX_REQUIRE((int64_t)num_images * num_rays < ((int64_t)1 << 31), "too many rays for one call");
    if (num_images == 0) return IAMX_OK;
    IAMX_REQUIRE(v && ned && pts && iters && flags, "null pointer");
    Terrain T;
    make_terrain(&T, axis_n, rows, axis_e, cols, grid);
    return launch_rays<false>(T, nullptr, nullptr, v, ned, num_images, num_rays, pts, iters, flags, stream,
                              "iamx_terrain_rays_vec");
}
