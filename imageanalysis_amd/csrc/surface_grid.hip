// Step 5 ("Create the map") on the device: piecewise-linear interpolation over a host Delaunay
// triangulation (scipy.interpolate.LinearNDInterpolator's rule) and the ray / surface intersection of
// scripts/lib/render_panda3d.py:25-78 + project.projectVectors for a batch of images.
//
// Compiled with -ffp-contract=off: the f64 expressions below restate the host's, operation by
// operation (separately rounded multiply and add).
//
// Everything here is a walk: a query visits one 128-byte record per step (the triangle's inverse
// transform, its neighbours and its vertices), and the vertex values are read only once the walk has
// ended.  The walks are latency-bound and lanes diverge in walk length and in round count; what
// keeps the step cheap is that the records of a survey's surface (600 k triangles = 77 MB) stay in
// the Infinity Cache.  DESIGN.md section 4 has the figures.
#include <float.h>
#include <math.h>

#include "iamx_common.h"

namespace {

constexpr int THREADS = 256;

// One triangle: rows 0 and 1 of scipy's transform[s] (the inverse of the edge matrix), row 2 (the
// offset r), neighbours (-1 at the hull) and vertices.  72 bytes of payload; 128-byte records are
// one cache line each, so a step of the walk is one line whatever the triangle's index.
struct __attribute__((aligned(128))) TriRec {
    double t00, t01, t10, t11, r0, r1;
    int nbr[3];
    int vtx[3];
    int pad[14];
};
static_assert(sizeof(TriRec) == IAMX_SURFACE_RECORD_BYTES, "record size is part of the ABI");

struct Surface {
    const TriRec *rec;
    const double *z;
    const int *seed;
    int T, P, G, max_steps;
    double x0, y0, sx, sy;       // seed grid: cell = (int)((x - x0) * sx), clamped
};

enum { LOOK_INSIDE = 0, LOOK_OUTSIDE = 1, LOOK_FALLBACK = 2 };

__device__ inline int seed_triangle(const Surface &S, double x, double y)
{
    // (a NaN or far-away coordinate: the comparisons below clamp it into the table)
    double fx = (x - S.x0) * S.sx, fy = (y - S.y0) * S.sy;
    int ix = fx >= 0.0 ? (fx < (double)S.G ? (int)fx : S.G - 1) : 0;
    int iy = fy >= 0.0 ? (fy < (double)S.G ? (int)fy : S.G - 1) : 0;
    return S.seed[iy * S.G + ix];
}

// Walks from triangle *tri to the one that holds (x, y); *tri is left at the last triangle visited,
// where the next look-up of the same ray starts.  *steps counts the records read.
__device__ inline int look_up(const Surface &S, double x, double y, int *tri, double *value, int *steps)
{
    const double eps = 100.0 * DBL_EPSILON;
    int s = *tri;
    if (!(x == x) || !(y == y) || s < 0 || s >= S.T) return LOOK_FALLBACK;
    for (int k = 0; k < S.max_steps; ++k) {
        const TriRec &r = S.rec[s];
        const double dx = x - r.r0, dy = y - r.r1;
        const double c0 = r.t00 * dx + r.t01 * dy;
        const double c1 = r.t10 * dx + r.t11 * dy;
        const double c2 = 1.0 - (c0 + c1);
        ++*steps;
        *tri = s;
        if (!(c0 == c0) || !(c1 == c1)) return LOOK_FALLBACK;      // a degenerate simplex
        int j = 0;
        double cm = c0;
        if (c1 < cm) { cm = c1; j = 1; }
        if (c2 < cm) { cm = c2; j = 2; }
        if (cm >= -eps) {
            const int v0 = r.vtx[0], v1 = r.vtx[1], v2 = r.vtx[2];
            if ((unsigned)v0 >= (unsigned)S.P || (unsigned)v1 >= (unsigned)S.P || (unsigned)v2 >= (unsigned)S.P)
                return LOOK_FALLBACK;
            *value = c0 * S.z[v0] + c1 * S.z[v1] + c2 * S.z[v2];
            return LOOK_INSIDE;
        }
        const int next = r.nbr[j];
        if (next < 0) return LOOK_OUTSIDE;
        if (next >= S.T) return LOOK_FALLBACK;                      // (a damaged table: never an address)
        s = next;
    }
    return LOOK_FALLBACK;
}

__global__ __launch_bounds__(THREADS) void pack_kernel(const int *__restrict__ simplices,
                                                       const int *__restrict__ neighbors,
                                                       const double *__restrict__ transform, int T,
                                                       TriRec *__restrict__ rec)
{
    const int s = blockIdx.x * THREADS + threadIdx.x;
    if (s >= T) return;
    const double *t = transform + (int64_t)s * 6;
    TriRec r;
    r.t00 = t[0]; r.t01 = t[1]; r.t10 = t[2]; r.t11 = t[3]; r.r0 = t[4]; r.r1 = t[5];
    for (int k = 0; k < 3; ++k) {
        r.nbr[k] = neighbors[(int64_t)s * 3 + k];
        r.vtx[k] = simplices[(int64_t)s * 3 + k];
    }
    for (int k = 0; k < 14; ++k) r.pad[k] = 0;
    rec[s] = r;
}

__global__ __launch_bounds__(THREADS) void interp_kernel(Surface S, const double *__restrict__ xy, int64_t n,
                                                         double *__restrict__ out, uint8_t *__restrict__ flag,
                                                         int *__restrict__ steps_out)
{
    const int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (q >= n) return;
    const double x = xy[2 * q], y = xy[2 * q + 1];
    int tri = seed_triangle(S, x, y), steps = 0;
    double value = NAN;
    const int rc = look_up(S, x, y, &tri, &value, &steps);
    out[q] = rc == LOOK_INSIDE ? value : NAN;
    flag[q] = rc == LOOK_FALLBACK ? 1 : 0;
    if (steps_out) steps_out[q] = steps;
}

struct GridArgs {
    const double *M;             // [I][9]   body2ned . cam2body . IK
    const double *ned;           // [I][3]
    const double *avg_ground;    // [I]      -z_avg
    const double *uv;            // [n][2]   the shared pixel grid
    int n;
    int64_t total;               // I * n
    int no_extrapolate;
    int ground_mode;
    double ground_m;
    double *pts;                 // [I][n][3]
    int *rounds;                 // [I][n]
    uint8_t *flags;              // [I][n]
    int *steps;                  // [I][n] or null
};

__global__ __launch_bounds__(THREADS) void grid_kernel(Surface S, GridArgs A)
{
    const int64_t g = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (g >= A.total) return;
    const int64_t im = g / A.n;
    const int vx = (int)(g - im * A.n);
    const double *M = A.M + im * 9;
    const double ned0 = A.ned[im * 3], ned1 = A.ned[im * 3 + 1], ned2 = A.ned[im * 3 + 2];
    const double u = A.uv[2 * vx], w = A.uv[2 * vx + 1];
    // project.projectVectors: M . [u, v, 1], then transformations.unit_vector
    const double q0 = M[0] * u + M[1] * w + M[2] * 1.0;
    const double q1 = M[3] * u + M[4] * w + M[5] * 1.0;
    const double q2 = M[6] * u + M[7] * w + M[8] * 1.0;
    const double len = sqrt(q0 * q0 + q1 * q1 + q2 * q2);
    const double v0 = q0 / len, v1 = q1 / len, v2 = q2 / len;

    double p0 = ned0, p1 = ned1, p2 = ned2;
    int count = 0, steps = 0;
    uint8_t fl = 0;
    if (A.ground_mode) {
        // project.intersectVectorsWithGroundPlane
        if (v2 > 0.0) {
            const double d_proj = -(ned2 + A.ground_m);
            const double factor = d_proj / v2;
            p0 = ned0 + v0 * factor;
            p1 = ned1 + v1 * factor;
            p2 = ned2 + d_proj;
        } else {
            fl |= IAMX_SURFACE_SKY;
        }
    } else if (v2 <= 0.0) {
        fl |= IAMX_SURFACE_SKY;                       // intersect2d: "always assume camera pose is above ground"
    } else {
        // render_panda3d.intersect2d, as written
        int tri = seed_triangle(S, p1, p0);
        double tmp = NAN, surface;
        int rc = look_up(S, p1, p0, &tri, &tmp, &steps);
        if (rc == LOOK_FALLBACK) fl |= IAMX_SURFACE_FALLBACK;
        if (rc != LOOK_INSIDE) tmp = NAN;
        if (A.no_extrapolate || tmp == tmp) surface = tmp;
        else surface = A.avg_ground[im];
        double error = fabs(p2 - surface);
        while (error > 0.01 && count < 25 && !(fl & IAMX_SURFACE_FALLBACK)) {
            const double d_proj = -(ned2 - surface);
            const double factor = d_proj / v2;
            const double n_proj = v0 * factor;
            const double e_proj = v1 * factor;
            p0 = ned0 + n_proj;
            p1 = ned1 + e_proj;
            p2 = ned2 + d_proj;
            tmp = NAN;
            rc = look_up(S, p1, p0, &tri, &tmp, &steps);
            if (rc == LOOK_FALLBACK) fl |= IAMX_SURFACE_FALLBACK;
            if (rc != LOOK_INSIDE) tmp = NAN;
            if (A.no_extrapolate || tmp == tmp) surface = tmp;
            error = fabs(p2 - surface);
            ++count;
        }
        const double dy = ned0 - p0, dx = ned1 - p1, dz = ned2 - p2;
        const double dist = sqrt(dx * dx + dy * dy);
        const double angle = atan2(-dz, dist) * (180.0 / 3.14159265358979323846);
        if (angle < 30.0) {
            fl |= IAMX_SURFACE_HIGH_ANGLE;
            p0 = p1 = p2 = NAN;
        }
    }
    A.pts[g * 3] = p0;
    A.pts[g * 3 + 1] = p1;
    A.pts[g * 3 + 2] = p2;
    A.rounds[g] = count;
    A.flags[g] = fl;
    if (A.steps) A.steps[g] = steps;
}

int make_surface(Surface *S, const void *records, int num_triangles, const double *values, int num_points,
                 const int *seed,
                 int seed_g, const double *bbox, int max_steps)
{
    S->rec = static_cast<const TriRec *>(records);
    S->z = values;
    S->seed = seed;
    S->T = num_triangles;
    S->P = num_points;
    S->G = seed_g;
    S->max_steps = max_steps > 0 ? max_steps : num_triangles + 16;
    S->x0 = bbox[0];
    S->y0 = bbox[1];
    // (a flat bounding box -- one column of cells does for it)
    S->sx = bbox[2] > bbox[0] ? seed_g / (bbox[2] - bbox[0]) : 0.0;
    S->sy = bbox[3] > bbox[1] ? seed_g / (bbox[3] - bbox[1]) : 0.0;
    return 0;
}

}  // namespace

extern "C" int iamx_surface_pack(const int *simplices, const int *neighbors, const double *transform,
                                 int num_triangles, void *records, void *stream)
{
    IAMX_REQUIRE(simplices && neighbors && transform && records, "null pointer");
    IAMX_REQUIRE(num_triangles >= 1 && num_triangles <= IAMX_SURFACE_MAX_TRIANGLES, "bad triangle count");
    IAMX_REQUIRE(((uintptr_t)records & (IAMX_SURFACE_RECORD_BYTES - 1)) == 0, "records must be 128-byte aligned");
    const unsigned blocks = (unsigned)((num_triangles + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(pack_kernel, dim3(blocks), dim3(THREADS), 0, iamx::as_stream(stream), simplices,
                       neighbors, transform, num_triangles, static_cast<TriRec *>(records));
    return iamx::check_launch("iamx_surface_pack");
}

extern "C" int iamx_surface_interp(const void *records, int num_triangles, const double *values,
                                   int num_points, const int *seed, int seed_g, const double *bbox,
                                   const double *xy, int64_t num_queries, int max_steps, double *out,
                                   uint8_t *flags, int *steps, void *stream)
{
    IAMX_REQUIRE(records && values && seed && bbox && xy && out && flags, "null pointer");
    IAMX_REQUIRE(num_triangles >= 1 && num_triangles <= IAMX_SURFACE_MAX_TRIANGLES, "bad triangle count");
    IAMX_REQUIRE(num_points >= 3, "a surface needs 3 points");
    IAMX_REQUIRE(seed_g >= 1 && seed_g <= IAMX_SURFACE_MAX_SEED_GRID, "bad seed grid");
    IAMX_REQUIRE(num_queries >= 0 && num_queries < ((int64_t)1 << 31) * THREADS, "bad query count");
    IAMX_REQUIRE(max_steps >= 0, "bad step bound");
    IAMX_REQUIRE(((uintptr_t)records & (IAMX_SURFACE_RECORD_BYTES - 1)) == 0, "records must be 128-byte aligned");
    if (num_queries == 0) return IAMX_OK;
    Surface S;
    make_surface(&S, records, num_triangles, values, num_points, seed, seed_g, bbox, max_steps);
    const unsigned blocks = (unsigned)((num_queries + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(interp_kernel, dim3(blocks), dim3(THREADS), 0, iamx::as_stream(stream), S, xy,
                       num_queries, out, flags, steps);
    return iamx::check_launch("iamx_surface_interp");
}

extern "C" int iamx_surface_grid(const void *records, int num_triangles, const double *values, int num_points,
                                 const int *seed, int seed_g, const double *bbox, const double *M,
                                 const double *ned, const double *avg_ground, int num_images,
                                 const double *uv, int num_vertices, int no_extrapolate, int ground_mode,
                                 double ground_m, int max_steps, double *pts, int *rounds, uint8_t *flags,
                                 int *steps, void *stream)
{
    IAMX_REQUIRE(M && ned && uv && pts && rounds && flags, "null pointer");
    IAMX_REQUIRE(num_images >= 0 && num_vertices >= 1, "bad size");
    IAMX_REQUIRE((int64_t)num_images * num_vertices < ((int64_t)1 << 31), "too many rays for one call");
    IAMX_REQUIRE(max_steps >= 0, "bad step bound");
    Surface S;
    memset(&S, 0, sizeof(S));
    if (!ground_mode) {
        IAMX_REQUIRE(records && values && seed && bbox && avg_ground, "null pointer");
        IAMX_REQUIRE(num_triangles >= 1 && num_triangles <= IAMX_SURFACE_MAX_TRIANGLES, "bad triangle count");
        IAMX_REQUIRE(num_points >= 3, "a surface needs 3 points");
        IAMX_REQUIRE(seed_g >= 1 && seed_g <= IAMX_SURFACE_MAX_SEED_GRID, "bad seed grid");
        IAMX_REQUIRE(((uintptr_t)records & (IAMX_SURFACE_RECORD_BYTES - 1)) == 0,
                     "records must be 128-byte aligned");
        make_surface(&S, records, num_triangles, values, num_points, seed, seed_g, bbox, max_steps);
    }
    if (num_images == 0) return IAMX_OK;
    GridArgs A;
    A.M = M;
    A.ned = ned;
    A.avg_ground = avg_ground;
    A.uv = uv;
    A.n = num_vertices;
    A.total = (int64_t)num_images * num_vertices;
    A.no_extrapolate = no_extrapolate ? 1 : 0;
    A.ground_mode = ground_mode ? 1 : 0;
    A.ground_m = ground_m;
    A.pts = pts;
    A.rounds = rounds;
    A.flags = flags;
    A.steps = steps;
    const unsigned blocks = (unsigned)((A.total + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(grid_kernel, dim3(blocks), dim3(THREADS), 0, iamx::as_stream(stream), S, A);
    return iamx::check_launch("iamx_surface_grid");
}
