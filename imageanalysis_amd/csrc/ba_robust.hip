// Robust loss functions for the device bundle adjustment (gfx950), float64.
//
// scipy.optimize.least_squares(loss=, f_scale=) -- scipy/optimize/_lsq/least_squares.py
// construct_loss_function and _lsq/common.py scale_for_robust_loss_function -- applied per scalar
// residual component f (u and v separately) with C = f_scale, z = (f / C)^2:
//
//     cost    = 0.5 C^2 sum rho(z)
//     J_scale = max(rho' + 2 rho'' z, EPS),  EPS = 2^-52
//     f      <- f rho' / sqrt(J_scale),      row of J <- row of J . sqrt(J_scale)
//
// after which the Gauss-Newton model of the scaled (f, J) has the gradient and the Triggs
// approximation of the Hessian of the robust cost.  J_scale in closed form (SciPy evaluates
// rho' + 2 rho'' z, which cancels):
//
//     huber    1 for z <= 1, else 0 -> EPS           rho = z | 2 sqrt(z) - 1     rho' = 1 | z^-1/2
//     soft_l1  (1 + z)^-3/2                          rho = 2 (sqrt(1 + z) - 1)   rho' = (1 + z)^-1/2
//     cauchy   (1 - z) / (1 + z)^2                   rho = log1p(z)              rho' = 1 / (1 + z)
//     arctan   (1 - 3 z^2) / (1 + z^2)^2             rho = atan(z)               rho' = 1 / (1 + z^2)
//
// Two kernels, both streams:
//   robust_cost_kernel   sum rho(z) over a residual vector: the fixed grid and fixed tree of
//                        trf_vec.hip's dots_kernel / final_kernel (256 partials, no atomics)
//   robust_scale_kernel  one in-place pass over r [O][2], Jc [O][2][7], Jp [O][2][3] and Jk [O][2][8]:
//                        224 B read + 224 B written per observation (480 B with Jk)
// tests/robust_loss_restatement.py states the same expressions in numpy, operation by operation
// (this file is compiled with -ffp-contract=off).
#include "iamx_common.h"
#include <math.h>

namespace {

constexpr int RB_BLOCKS = 256;        // partial results of the cost reduction
constexpr int RB_TILE = 256;          // observations per workgroup of the scale pass
constexpr double RB_EPS = 2.220446049250313e-16;      // 2^-52, np.finfo(float).eps

template <int LOSS>
__device__ __forceinline__ double rho_of(double z)
{
    if (LOSS == IAMX_LOSS_HUBER) return z <= 1.0 ? z : 2.0 * sqrt(z) - 1.0;
    if (LOSS == IAMX_LOSS_SOFT_L1) return 2.0 * (z / (sqrt(1.0 + z) + 1.0));     // = 2 (sqrt(1 + z) - 1)
    if (LOSS == IAMX_LOSS_CAUCHY) return log1p(z);
    return atan(z);
}

// (factor of f, factor of the row of J) of one residual component
template <int LOSS>
__device__ __forceinline__ void row_factors(double f, double c, double &ff, double &fj)
{
    const double s = f / c;
    const double z = s * s;
    double d1, js;                      // rho', J_scale before the clip
    if (LOSS == IAMX_LOSS_HUBER) {
        d1 = z <= 1.0 ? 1.0 : 1.0 / sqrt(z);
        js = z <= 1.0 ? 1.0 : 0.0;
    } else if (LOSS == IAMX_LOSS_SOFT_L1) {
        const double t = 1.0 + z, q = sqrt(t);
        d1 = 1.0 / q;
        js = 1.0 / (t * q);
    } else if (LOSS == IAMX_LOSS_CAUCHY) {
        const double t = 1.0 + z;
        d1 = 1.0 / t;
        js = (1.0 - z) / (t * t);
    } else {
        const double z2 = z * z, t = 1.0 + z2;
        d1 = 1.0 / t;
        js = (1.0 - 3.0 * z2) / (t * t);
    }
    js = js < RB_EPS ? RB_EPS : js;
    fj = sqrt(js);
    ff = d1 / fj;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

template <int LOSS>
__global__ __launch_bounds__(256) void robust_cost_kernel(int64_t n, const double *__restrict__ r,
                                                          double c, double *__restrict__ partial)
{
    __shared__ double sh[4];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double s = r[i] / c;
        acc += rho_of<LOSS>(s * s);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ __launch_bounds__(256) void robust_final_kernel(const double *__restrict__ partial,
                                                           double *__restrict__ out)
{
    __shared__ double sh[4];
    double v = wave_sum(partial[threadIdx.x]);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// `count` (even) doubles at `a`, W per row, rows numbered from the start of `a`: every entry times
// the J factor of its row.  16 bytes per lane, K x 256 lanes: all loads are issued before the first
// product (W is even only for Jk: the two entries of a lane may sit in two rows).
template <int W, int K>
__device__ __forceinline__ void scale_rows(double *__restrict__ a, int count, const double *fj)
{
    double2 v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = 2 * (k * 256 + (int)threadIdx.x);
        if (e < count) v[k] = *reinterpret_cast<const double2 *>(a + e);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = 2 * (k * 256 + (int)threadIdx.x);
        if (e < count) {
            v[k].x *= fj[e / W];
            v[k].y *= fj[(e + 1) / W];
            *reinterpret_cast<double2 *>(a + e) = v[k];
        }
    }
}

// One workgroup per RB_TILE observations: thread t forms the factors of observation t from the
// UNSCALED residuals (nobody else touches the tile's r), then the workgroup streams the tile's
// Jacobian blocks.  An observation owns an even number of doubles in every array, so every
// 16-byte access is aligned whatever n_obs is.
template <int LOSS>
__global__ __launch_bounds__(256) void robust_scale_kernel(double *__restrict__ r, double *__restrict__ Jc,
                                                           double *__restrict__ Jp, double *__restrict__ Jk,
                                                           int64_t n_obs, double c)
{
    __shared__ double fj[2 * RB_TILE];
    const int64_t first = (int64_t)blockIdx.x * RB_TILE;
    const int64_t left = n_obs - first;
    const int nt = (int)(left < RB_TILE ? left : RB_TILE);           // observations of this tile
    const int t = threadIdx.x;
    if (t < nt) {
        double2 f = *reinterpret_cast<const double2 *>(r + 2 * (first + t));
        double fu, fv, ju, jv;
        row_factors<LOSS>(f.x, c, fu, ju);
        row_factors<LOSS>(f.y, c, fv, jv);
        f.x *= fu;
        f.y *= fv;
        *reinterpret_cast<double2 *>(r + 2 * (first + t)) = f;
        fj[2 * t] = ju;
        fj[2 * t + 1] = jv;
    }
    __syncthreads();
    scale_rows<7, 7>(Jc + 14 * first, 14 * nt, fj);
    scale_rows<3, 3>(Jp + 6 * first, 6 * nt, fj);
    if (Jk) scale_rows<8, 8>(Jk + 16 * first, 16 * nt, fj);
}

bool loss_ok(int loss) { return loss >= IAMX_LOSS_HUBER && loss <= IAMX_LOSS_ARCTAN; }

}  // namespace

extern "C" int iamx_ba_robust_cost(const double *r, int64_t m, int loss, double f_scale, double *out,
                                   double *scratch, void *stream)
{
    IAMX_REQUIRE(r && out && scratch, "null pointer");
    IAMX_REQUIRE(m >= 0, "bad size");
    IAMX_REQUIRE(loss_ok(loss), "unknown loss (huber, soft_l1, cauchy, arctan)");
    IAMX_REQUIRE(isfinite(f_scale) && f_scale > 0, "f_scale must be positive and finite");
    hipStream_t st = iamx::as_stream(stream);
    const dim3 g(RB_BLOCKS), b(256);
    switch (loss) {
    case IAMX_LOSS_HUBER: hipLaunchKernelGGL(robust_cost_kernel<IAMX_LOSS_HUBER>, g, b, 0, st, m, r, f_scale, scratch); break;
    case IAMX_LOSS_SOFT_L1: hipLaunchKernelGGL(robust_cost_kernel<IAMX_LOSS_SOFT_L1>, g, b, 0, st, m, r, f_scale, scratch); break;
    case IAMX_LOSS_CAUCHY: hipLaunchKernelGGL(robust_cost_kernel<IAMX_LOSS_CAUCHY>, g, b, 0, st, m, r, f_scale, scratch); break;
    default: hipLaunchKernelGGL(robust_cost_kernel<IAMX_LOSS_ARCTAN>, g, b, 0, st, m, r, f_scale, scratch); break;
    }
    hipLaunchKernelGGL(robust_final_kernel, dim3(1), dim3(256), 0, st, scratch, out);
    return iamx::check_launch("iamx_ba_robust_cost");
}

extern "C" int iamx_ba_robust_scale(double *r, double *Jc, double *Jp, double *Jk, int64_t n_obs, int loss,
                                    double f_scale, void *stream)
{
    IAMX_REQUIRE(r && Jc && Jp, "null pointer");
    IAMX_REQUIRE(n_obs >= 0 && n_obs <= (int64_t)0x7fffffff * RB_TILE, "bad size");
    IAMX_REQUIRE(loss_ok(loss), "unknown loss (huber, soft_l1, cauchy, arctan)");
    IAMX_REQUIRE(isfinite(f_scale) && f_scale > 0, "f_scale must be positive and finite");
    IAMX_REQUIRE((((uintptr_t)r | (uintptr_t)Jc | (uintptr_t)Jp | (uintptr_t)Jk) & 15) == 0,
                 "r, Jc, Jp, Jk must be 16-byte aligned");
    if (n_obs == 0) return IAMX_OK;
    hipStream_t st = iamx::as_stream(stream);
    const dim3 g((unsigned)((n_obs + RB_TILE - 1) / RB_TILE)), b(256);
    switch (loss) {
    case IAMX_LOSS_HUBER: hipLaunchKernelGGL(robust_scale_kernel<IAMX_LOSS_HUBER>, g, b, 0, st, r, Jc, Jp, Jk, n_obs, f_scale); break;
    case IAMX_LOSS_SOFT_L1: hipLaunchKernelGGL(robust_scale_kernel<IAMX_LOSS_SOFT_L1>, g, b, 0, st, r, Jc, Jp, Jk, n_obs, f_scale); break;
    case IAMX_LOSS_CAUCHY: hipLaunchKernelGGL(robust_scale_kernel<IAMX_LOSS_CAUCHY>, g, b, 0, st, r, Jc, Jp, Jk, n_obs, f_scale); break;
    default: hipLaunchKernelGGL(robust_scale_kernel<IAMX_LOSS_ARCTAN>, g, b, 0, st, r, Jc, Jp, Jk, n_obs, f_scale); break;
    }
    return iamx::check_launch("iamx_ba_robust_scale");
}
