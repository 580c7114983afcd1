// Chain geometry between optimiser passes (gfx950) -- the loops of the reference's
// scripts/3c-match-triangulation.py (--method triangulate), scripts/4b-colocated-feats.py and
// lib/project.py:257-296 (undistort_uvlist / undistort_image_keypoints), one thread per point or
// per chain, f64 in stored order.  Built with -ffp-contract=off: every product and sum below is
// rounded on its own, in the order the numpy restatements (tests/undistort_restatement.py,
// tests/chain_tools_common.py) write them.
//
//   undistort     cv2.undistortPoints(src, K, dist, P=K) with OpenCV's default criteria as
//                 published: x = (u-cx)/fx, y = (v-cy)/fy, five rounds of
//                     r2 = x*x + y*y;  icdist = 1/(1 + ((k3*r2 + k2)*r2 + k1)*r2)
//                     dx = 2*p1*x*y + p2*(r2 + 2*x*x);  dy = p1*(r2 + 2*y*y) + 2*p2*x*y
//                     x = (x0 - dx)*icdist;  y = (y0 - dy)*icdist
//                 (icdist < 0: back to x0, y0 and stop), out = x*fx + cx, y*fy + cy as float32.
//                 Parity with cv2 itself is unpinned (cv2 is not available to the tests).
//   triangulate   per chain of the group with >= 2 members in the group: member uv -> float32 ->
//                 undistort -> float32, v = unit(unit(M [u, v, 1])), r += I - v v^T,
//                 q += (I - v v^T) p, r x = q by LU with partial pivoting
//                 (lib/line_solver.py ls_lines_intersection).
//   pair angles   per chain of the group, members i < j both in the group: the angle at the chain
//                 position between the two camera positions, below min_angle -> member i's count
//                 goes up (the reference's mark_list holds [chain, i] once per such pair).
#include "iamx_common.h"

namespace {

struct Lens {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
};

__device__ __forceinline__ void undistort_one(const Lens &L, float u_in, float v_in, float *u_out,
                                              float *v_out)
{
    const double x0 = ((double)u_in - L.cx) / L.fx, y0 = ((double)v_in - L.cy) / L.fy;
    double x = x0, y = y0;
    for (int it = 0; it < 5; ++it) {
        const double r2 = x * x + y * y;
        const double icdist = 1.0 / (1.0 + ((L.k3 * r2 + L.k2) * r2 + L.k1) * r2);
        if (icdist < 0.0) {
            x = x0;
            y = y0;
            break;
        }
        const double dx = 2.0 * L.p1 * x * y + L.p2 * (r2 + 2.0 * x * x);
        const double dy = L.p1 * (r2 + 2.0 * y * y) + 2.0 * L.p2 * x * y;
        x = (x0 - dx) * icdist;
        y = (y0 - dy) * icdist;
    }
    *u_out = (float)(x * L.fx + L.cx);
    *v_out = (float)(y * L.fy + L.cy);
}

__global__ __launch_bounds__(256) void undistort_points_kernel(const float *__restrict__ src, int64_t n,
                                                               Lens L, float *__restrict__ dst)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    float u, v;
    undistort_one(L, src[2 * k], src[2 * k + 1], &u, &v);
    dst[2 * k] = u;
    dst[2 * k + 1] = v;
}

// members of chain [b, e): 0 when every image index is inside [0, n_images), else 1; *n_in = the
// members whose image is in the group (in_group is only read at valid indices)
__device__ __forceinline__ int scan_members(const int32_t *__restrict__ img, int64_t b, int64_t e,
                                            const uint8_t *__restrict__ in_group, int n_images, int *n_in)
{
    int cnt = 0;
    for (int64_t o = b; o < e; ++o) {
        const int im = img[o];
        if (im < 0 || im >= n_images) return 1;
        cnt += in_group[im] ? 1 : 0;
    }
    *n_in = cnt;
    return 0;
}

__global__ __launch_bounds__(256) void chain_triangulate_kernel(
    const int64_t *__restrict__ ptr, const int32_t *__restrict__ img, const double *__restrict__ uv,
    const int32_t *__restrict__ group, int64_t n_chains, int group_index, const double *__restrict__ M,
    const double *__restrict__ pos, const uint8_t *__restrict__ in_group, int n_images, Lens L,
    double *__restrict__ ned, int32_t *__restrict__ status)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_chains) return;
    status[c] = IAMX_CHAIN_UNTOUCHED;
    if (group[c] != group_index) return;
    const int64_t b = ptr[c], e = ptr[c + 1];
    int n_in = 0;
    if (scan_members(img, b, e, in_group, n_images, &n_in)) {
        status[c] = IAMX_CHAIN_BAD_IMAGE;
        return;
    }
    if (n_in < 2) return;
    double r[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, q[3] = {0, 0, 0};
    for (int64_t o = b; o < e; ++o) {
        const int im = img[o];
        if (!in_group[im]) continue;
        float uf, vf;
        undistort_one(L, (float)uv[2 * o], (float)uv[2 * o + 1], &uf, &vf);
        const double u = (double)uf, v = (double)vf;
        const double *m = M + (int64_t)im * 9, *p = pos + (int64_t)im * 3;
        double d[3];
        d[0] = (m[0] * u + m[1] * v) + m[2];
        d[1] = (m[3] * u + m[4] * v) + m[5];
        d[2] = (m[6] * u + m[7] * v) + m[8];
        // project.projectVectors' unit_vector, then the line solver's v / norm(v)
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const double nrm = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
            d[0] = d[0] / nrm;
            d[1] = d[1] / nrm;
            d[2] = d[2] / nrm;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double ri[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) ri[j] = (i == j ? 1.0 : 0.0) - d[i] * d[j];
            const double qi = (ri[0] * p[0] + ri[1] * p[1]) + ri[2] * p[2];
#pragma unroll
            for (int j = 0; j < 3; ++j) r[i][j] = r[i][j] + ri[j];
            q[i] = q[i] + qi;
        }
    }
    // LU with partial pivoting (the first of equal magnitudes, as LAPACK's idamax), then the two
    // triangular solves
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int piv = k;
        double best = fabs(r[k][k]);
#pragma unroll
        for (int i = k + 1; i < 3; ++i) {
            if (fabs(r[i][k]) > best) {
                best = fabs(r[i][k]);
                piv = i;
            }
        }
#pragma unroll
        for (int i = k + 1; i < 3; ++i) {
            if (piv == i) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double t = r[k][j];
                    r[k][j] = r[i][j];
                    r[i][j] = t;
                }
                const double t = q[k];
                q[k] = q[i];
                q[i] = t;
            }
        }
        if (r[k][k] == 0.0) {                          // zero pivot: numpy raises LinAlgError
            status[c] = IAMX_CHAIN_SINGULAR;
            return;
        }
#pragma unroll
        for (int i = k + 1; i < 3; ++i) {
            const double l = r[i][k] / r[k][k];
#pragma unroll
            for (int j = k + 1; j < 3; ++j) r[i][j] = r[i][j] - l * r[k][j];
            q[i] = q[i] - l * q[k];
        }
    }
    const double x2 = q[2] / r[2][2];
    const double x1 = (q[1] - r[1][2] * x2) / r[1][1];
    const double x0 = ((q[0] - r[0][1] * x1) - r[0][2] * x2) / r[0][0];
    ned[3 * c] = x0;
    ned[3 * c + 1] = x1;
    ned[3 * c + 2] = x2;
    status[c] = x2 > 0.0 ? IAMX_CHAIN_WRITTEN_BELOW : IAMX_CHAIN_WRITTEN;
}

__global__ __launch_bounds__(256) void chain_pair_angles_kernel(
    const int64_t *__restrict__ ptr, const int32_t *__restrict__ img, const int32_t *__restrict__ group,
    const double *__restrict__ ned, int64_t n_chains, int group_index, const double *__restrict__ pos,
    const uint8_t *__restrict__ in_group, int n_images, double min_angle_deg,
    int32_t *__restrict__ count, unsigned long long *__restrict__ total, int32_t *__restrict__ status)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_chains) return;
    const int64_t b = ptr[c], e = ptr[c + 1];
    for (int64_t o = b; o < e; ++o) count[o] = 0;
    status[c] = IAMX_CHAIN_UNTOUCHED;
    if (group[c] != group_index) return;
    int n_in = 0;
    if (scan_members(img, b, e, in_group, n_images, &n_in)) {
        status[c] = IAMX_CHAIN_BAD_IMAGE;
        return;
    }
    status[c] = IAMX_CHAIN_WRITTEN;
    if (n_in < 2) return;
    const double f0 = ned[3 * c], f1 = ned[3 * c + 1], f2 = ned[3 * c + 2];
    const double r2d = 180.0 / 3.14159265358979323846;
    unsigned long long sum = 0;
    for (int64_t i = b; i < e; ++i) {
        const int ia = img[i];
        if (!in_group[ia]) continue;
        const double *pa = pos + (int64_t)ia * 3;
        const double a0 = f0 - pa[0], a1 = f1 - pa[1], a2 = f2 - pa[2];
        const double na = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
        int cnt = 0;
        for (int64_t j = i + 1; j < e; ++j) {
            const int ib = img[j];
            if (!in_group[ib]) continue;
            const double *pb = pos + (int64_t)ib * 3;
            const double b0 = f0 - pb[0], b1 = f1 - pb[1], b2 = f2 - pb[2];
            const double nb = sqrt((b0 * b0 + b1 * b1) + b2 * b2);
            const double denom = na * nb;
            // denom exactly 0.000001 is the reference's 0; a NaN denom goes on to a NaN angle
            double angle = 0.0;
            if (fabs(denom - 0.000001) > 0.0 || denom != denom) {
                double tmp = ((a0 * b0 + a1 * b1) + a2 * b2) / denom;
                if (tmp > 1.0) tmp = 1.0;
                // below -1: math.acos raises and the reference's except path returns 0; NaN stays
                // NaN and compares false
                angle = tmp < -1.0 ? 0.0 : acos(tmp);
            }
            if (angle * r2d < min_angle_deg) ++cnt;
        }
        count[i] = cnt;
        sum += (unsigned long long)cnt;
    }
    if (sum) atomicAdd(total, sum);
}

Lens make_lens(const double *K4, const double *dist5)
{
    Lens L;
    L.fx = K4[0]; L.fy = K4[1]; L.cx = K4[2]; L.cy = K4[3];
    L.k1 = dist5[0]; L.k2 = dist5[1]; L.p1 = dist5[2]; L.p2 = dist5[3]; L.k3 = dist5[4];
    return L;
}

}  // namespace

extern "C" int iamx_undistort_points(const float *src, int64_t n, const double *K4, const double *dist5,
                                     float *dst, void *stream)
{
    IAMX_REQUIRE(K4 && dist5, "null pointer");
    IAMX_REQUIRE(n >= 0, "bad size");
    if (n == 0) return IAMX_OK;
    IAMX_REQUIRE(src && dst, "null pointer");
    IAMX_REQUIRE(K4[0] != 0.0 && K4[1] != 0.0, "zero focal length");
    IAMX_REQUIRE((n + 255) / 256 <= 0x7fffffffLL, "too many points");
    hipLaunchKernelGGL(undistort_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       iamx::as_stream(stream), src, n, make_lens(K4, dist5), dst);
    return iamx::check_launch("iamx_undistort_points");
}

extern "C" int iamx_chain_triangulate(const int64_t *ptr, const int32_t *img, const double *uv,
                                      const int32_t *group, int64_t n_chains, int group_index,
                                      const double *M, const double *pos, const uint8_t *in_group,
                                      int n_images, const double *K4, const double *dist5, double *ned,
                                      int32_t *status, void *stream)
{
    IAMX_REQUIRE(K4 && dist5, "null pointer");
    IAMX_REQUIRE(n_chains >= 0 && n_images >= 0, "bad size");
    if (n_chains == 0) return IAMX_OK;
    IAMX_REQUIRE(ptr && img && uv && group && ned && status, "null pointer");
    IAMX_REQUIRE(n_images == 0 || (M && pos && in_group), "null pointer");
    IAMX_REQUIRE(K4[0] != 0.0 && K4[1] != 0.0, "zero focal length");
    IAMX_REQUIRE((n_chains + 255) / 256 <= 0x7fffffffLL, "too many chains");
    hipLaunchKernelGGL(chain_triangulate_kernel, dim3((unsigned)((n_chains + 255) / 256)), dim3(256), 0,
                       iamx::as_stream(stream), ptr, img, uv, group, n_chains, group_index, M, pos,
                       in_group, n_images, make_lens(K4, dist5), ned, status);
    return iamx::check_launch("iamx_chain_triangulate");
}

extern "C" int iamx_chain_pair_angles(const int64_t *ptr, const int32_t *img, const int32_t *group,
                                      const double *ned, int64_t n_chains, int group_index,
                                      const double *pos, const uint8_t *in_group, int n_images,
                                      double min_angle_deg, int32_t *count, int64_t *total,
                                      int32_t *status, void *stream)
{
    IAMX_REQUIRE(n_chains >= 0 && n_images >= 0, "bad size");
    if (n_chains == 0) return IAMX_OK;
    IAMX_REQUIRE(ptr && img && group && ned && count && total && status, "null pointer");
    IAMX_REQUIRE(n_images == 0 || (pos && in_group), "null pointer");
    IAMX_REQUIRE((n_chains + 255) / 256 <= 0x7fffffffLL, "too many chains");
    const hipError_t cleared = hipMemsetAsync(total, 0, sizeof(int64_t), iamx::as_stream(stream));
    if (cleared != hipSuccess)
        return iamx::fail(IAMX_ELAUNCH, "iamx_chain_pair_angles: clearing the total: %s",
                          hipGetErrorString(cleared));
    hipLaunchKernelGGL(chain_pair_angles_kernel, dim3((unsigned)((n_chains + 255) / 256)), dim3(256), 0,
                       iamx::as_stream(stream), ptr, img, group, ned, n_chains, group_index, pos,
                       in_group, n_images, min_angle_deg, count,
                       reinterpret_cast<unsigned long long *>(total), status);
    return iamx::check_launch("iamx_chain_pair_angles");
}
