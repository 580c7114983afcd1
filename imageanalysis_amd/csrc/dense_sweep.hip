// Dense surface (gfx950): plane-sweep depth maps, their cross-view consistency check and the DSM
// splat.  The rules are stated in imageanalysis_amd/dense.py's docstring and restated in numpy by
// tests/dense_restatement.py; this file follows them operation by operation (float64 geometry,
// float32 photometry, every product and sum rounded on its own: the pragma below switches contraction
// off for the whole file, which is what -ffp-contract=off gives; build.sh's flag table is unchanged).
//
// sweep_kernel<R>: one launch per reference image does the whole sweep, the cost volume never
// reaches memory.  A workgroup of 256 threads owns a 32 x 16 tile of reference pixels, thread
// (tx, ty) the two pixels (2 tx, ty) and (2 tx + 1, ty).  It walks planes x neighbours; per step
//   warp       the tile plus its halo of R pixels, (32 + 2R) x (16 + 2R) positions spread over the
//              256 threads (the positions of a thread are the same at every step, so their ray
//              coordinates stay in registers): float64 projection into the neighbour, bilinear
//              gather through L2, one float32 into LDS -- NaN for an invalid sample or a position
//              outside the reference image, so that a window that holds one sums to NaN;
//   barrier    one: the warped tile is double-buffered;
//   correlate  each thread reads (2R + 1) rows of 2R + 2 floats as R + 1 ds_read_b64 (the two
//              pixels share 2R of the 2R + 1 columns), once for the mean and once, beside the
//              reference tile, for the centred sums.
// The LDS pitch is 96 floats: 96 = 32 mod 64 puts the two rows of a 32-lane half on opposite
// halves of the 64 banks a ds_read_b64 sees, so the reads are conflict-free.  Three tiles of
// 30 x 96 floats = 34 560 bytes: four workgroups per CU by LDS.  The mean and the centred sum
// of the reference window do not depend on the step and are computed once.  The running winner and
// the scores before and after it stay in registers.  No atomics.
//
// sweep_kernel<R, true> (iamx_dense_sweep_volume) is the same kernel with the emission compiled in: each
// aggregate score also leaves as the uint8 cost of dense.py's SEMI-GLOBAL RULES, volume [h][w][planes],
// for csrc/dense_sgm.hip.  A thread gathers four planes of a pixel into one dword store where planes is a
// multiple of 4 and stores bytes otherwise.  sweep_kernel<R, false> never reads its volume argument and
// compiles to the instructions of the kernel before the emission existed.
//
// sweep_kernel<R, false, true> (iamx_dense_sweep_guided) is the same kernel again with the plane loop's
// bounds read from a table (dense.py's REFINEMENT RULES): the workgroup of tile (bx, by) walks the planes
// first <= d < first + count of entry by tiles_x + bx, out of planes_total global planes.  Every lane loads
// the same two ints, so the bounds, and with them every barrier, are uniform in the workgroup; a window of
// no planes runs the loop zero times and the workgroup writes its empty pixels at the end like any other.
// The plane index, the depths, the winner and the parabola are the global d's; a winner on a rim of its
// window that is not a rim of the plane set loses its depth (the window-edge rule).  No volume in this form.
//
// check_kernel: one thread per pixel of every depth map.  splat_kernel: one thread per point,
// integer atomics only (a 32-bit count and a 64-bit sum of rint(up 1024) per cell), so the result
// does not depend on scheduling.  resolve_kernel: sum / 1024 / count.
#include <math.h>

#include <vector>

#include "iamx_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int TILE_W = IAMX_DENSE_TILE_W;          // 32
constexpr int TILE_H = IAMX_DENSE_TILE_H;          // 16
constexpr int MAX_R = IAMX_DENSE_MAX_RADIUS;       // 7
constexpr int PITCH = 96;                          // floats; = 32 (mod 64), >= TILE_W + 2 MAX_R
constexpr int LDS_ROWS = TILE_H + 2 * MAX_R;       // 30
constexpr int CAM = IAMX_DENSE_CAM_DOUBLES;        // 21: R[9] row-major, C[3], fx, fy, cx, cy, k1, k2, p1, p2, k3

static_assert(TILE_W + 2 * MAX_R <= PITCH && PITCH % 64 == 32, "LDS pitch");
static_assert(TILE_W == 32 && TILE_H == 16 && THREADS == 256, "thread (tx, ty) owns two pixels");

__device__ __forceinline__ float qnan() { return __int_as_float(0x7fc00000); }

struct Cam {
    double R[9], C[3], fx, fy, cx, cy, k1, k2, p1, p2, k3;
};

__device__ __forceinline__ Cam load_cam(const double *__restrict__ p)
{
    Cam c;
    for (int i = 0; i < 9; ++i) c.R[i] = p[i];
    for (int i = 0; i < 3; ++i) c.C[i] = p[9 + i];
    c.fx = p[12]; c.fy = p[13]; c.cx = p[14]; c.cy = p[15];
    c.k1 = p[16]; c.k2 = p[17]; c.p1 = p[18]; c.p2 = p[19]; c.k3 = p[20];
    return c;
}

// a point of camera c -> NED: R^T X + C, summed from the left
__device__ __forceinline__ void to_world(const double *__restrict__ R, const double *__restrict__ C, double x,
                                         double y, double z, double &n, double &e, double &d)
{
    n = ((R[0] * x + R[3] * y) + R[6] * z) + C[0];
    e = ((R[1] * x + R[4] * y) + R[7] * z) + C[1];
    d = ((R[2] * x + R[5] * y) + R[8] * z) + C[2];
}

// a NED point -> pixel of camera c (synth.project's expression order) and its depth there
__device__ __forceinline__ void project(const Cam &c, double n, double e, double d, double &u, double &v, double &zc)
{
    const double dn = n - c.C[0], de = e - c.C[1], dd = d - c.C[2];
    const double X = (c.R[0] * dn + c.R[1] * de) + c.R[2] * dd;
    const double Y = (c.R[3] * dn + c.R[4] * de) + c.R[5] * dd;
    zc = (c.R[6] * dn + c.R[7] * de) + c.R[8] * dd;
    const double x = X / zc, y = Y / zc;
    const double r2 = x * x + y * y;
    const double rad = 1 + r2 * (c.k1 + r2 * (c.k2 + r2 * c.k3));
    const double xd = x * rad + 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x);
    const double yd = y * rad + c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y;
    u = c.fx * xd + c.cx;
    v = c.fy * yd + c.cy;
}

struct SweepArgs {
    const float *ref;            // [h][w]
    const double *rays;          // [h][w][2]  (xn, yn)
    const float *nbr;            // [n][h][w]
    const double *ref_pose;      // [12]  R, C
    const double *nbr_cam;       // [n][CAM]
    int w, h, n, planes;
    double w_far, step;
    float gate;                  // min_var * N
    float min_score;
    int32_t *plane;              // [h][w]
    float *score;                // [h][w]
    float *depth;                // [h][w]
    float *around;               // [h][w][3]
};

// one row of 2R + 2 floats at an even LDS offset, as R + 1 ds_read_b64
template <int R>
__device__ __forceinline__ void read_row(const float *__restrict__ s, float (&a)[2 * R + 2])
{
#pragma unroll
    for (int j = 0; j <= R; ++j) {
        const float2 t = *reinterpret_cast<const float2 *>(s + 2 * j);
        a[2 * j] = t.x;
        a[2 * j + 1] = t.y;
    }
}

// the running winner of one pixel
struct Winner {
    int best;
    float s0, sm, sp, prev;
    __device__ __forceinline__ void init() { best = -1; s0 = sm = sp = prev = qnan(); }
    __device__ __forceinline__ void step(int d, float S)
    {
        if (S == S && (best < 0 || S > s0)) {
            best = d; s0 = S; sm = prev; sp = qnan();
        } else if (best >= 0 && best == d - 1) {
            sp = S;
        }
        prev = S;
    }
};

// clipped: the winner stands on a rim of its tile's window that is not a rim of the plane set (the guided form)
__device__ __forceinline__ void write_pixel(const SweepArgs &A, int g, const Winner &W, bool clipped = false)
{
    float off = 0.0f;
    if (W.best >= 0 && W.sm == W.sm && W.sp == W.sp) {
        const float den = (W.sm - 2.0f * W.s0) + W.sp;
        if (den < 0.0f) {
            off = (0.5f * (W.sm - W.sp)) / den;
            off = off < -0.5f ? -0.5f : (off > 0.5f ? 0.5f : off);
        }
    }
    float depth = qnan();
    if (W.best >= 0 && W.s0 >= A.min_score && !clipped)
        depth = (float)(1.0 / (A.w_far + ((double)W.best + (double)off) * A.step));
    A.plane[g] = W.best;
    A.score[g] = W.s0;
    A.depth[g] = depth;
    A.around[3 * (int64_t)g] = W.sm;
    A.around[3 * (int64_t)g + 1] = W.s0;
    A.around[3 * (int64_t)g + 2] = W.sp;
}

// the cost of SEMI-GLOBAL RULES: uint8, 255 for an invalid score, the clamp after the rounding
__device__ __forceinline__ uint32_t cost_of(float S)
{
    if (!(S == S)) return 255u;
    float c = rintf((1.0f - S) * 127.0f);
    c = c < 0.0f ? 0.0f : (c > 254.0f ? 254.0f : c);
    return (uint32_t)c;
}

// VOL: the costs of the thread's two pixels go to volume [h][w][planes] as well, four planes to a
// dword store where planes is a multiple of 4 (pixel g's row then starts on a dword), bytes otherwise
// GUIDED: the planes walked are the tile's window of `windows` [tiles_y][tiles_x][2] = (first, count),
// A.planes is the size of the global plane set, and the window-edge rule applies
template <int R, bool VOL, bool GUIDED = false>
__global__ __launch_bounds__(THREADS) void sweep_kernel(SweepArgs A, uint8_t *__restrict__ volume,
                                                        const int32_t *__restrict__ windows)
{
    static_assert(!(VOL && GUIDED), "the guided form emits no volume");
    constexpr int K = 2 * R + 1;                         // window side
    constexpr int TW = TILE_W + 2 * R, TH = TILE_H + 2 * R;
    constexpr int NPOS = (TW * TH + THREADS - 1) / THREADS;
    constexpr float N = (float)(K * K);
    constexpr int UY = R <= 2 ? K : 1;                   // rows of a window in flight: registers against latency

    __shared__ __attribute__((aligned(16))) float s_ref[LDS_ROWS * PITCH];
    __shared__ __attribute__((aligned(16))) float s_warp[2][LDS_ROWS * PITCH];

    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int w = A.w, h = A.h;
    const int ox = blockIdx.x * TILE_W - R, oy = blockIdx.y * TILE_H - R;   // image position of LDS (0, 0)

    // ---- the thread's warp positions: LDS offset (-1: none), image offset (-1: outside), rays ----
    int pos_lds[NPOS], pos_img[NPOS];
    double pos_xn[NPOS], pos_yn[NPOS];
#pragma unroll
    for (int k = 0; k < NPOS; ++k) {
        const int i = tid + k * THREADS;
        pos_lds[k] = -1;
        pos_img[k] = -1;
        pos_xn[k] = 0.0;
        pos_yn[k] = 0.0;
        if (i < TW * TH) {
            const int ly = i / TW, lx = i - ly * TW;
            const int gx = ox + lx, gy = oy + ly;
            pos_lds[k] = ly * PITCH + lx;
            float a = qnan();
            if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
                const int g = gy * w + gx;
                pos_img[k] = g;
                pos_xn[k] = A.rays[2 * (int64_t)g];
                pos_yn[k] = A.rays[2 * (int64_t)g + 1];
                a = A.ref[g];
            }
            s_ref[pos_lds[k]] = a;
        }
    }
    __syncthreads();

    // ---- the two pixels of the thread: mean and centred sum of the reference window, once ----
    const int px = blockIdx.x * TILE_W + 2 * tx, py = blockIdx.y * TILE_H + ty;
    const int base = ty * PITCH + 2 * tx;               // LDS offset of the first pixel's window corner
    float ma0, ma1, saa0 = 0.0f, saa1 = 0.0f;
    {
        float sa0 = 0.0f, sa1 = 0.0f;
#pragma unroll UY
        for (int dy = 0; dy < K; ++dy) {
            float a[2 * R + 2];
            read_row<R>(s_ref + base + dy * PITCH, a);
#pragma unroll
            for (int dx = 0; dx < K; ++dx) {
                sa0 = sa0 + a[dx];
                sa1 = sa1 + a[dx + 1];
            }
        }
        ma0 = sa0 / N;
        ma1 = sa1 / N;
#pragma unroll UY
        for (int dy = 0; dy < K; ++dy) {
            float a[2 * R + 2];
            read_row<R>(s_ref + base + dy * PITCH, a);
#pragma unroll
            for (int dx = 0; dx < K; ++dx) {
                const float c0 = a[dx] - ma0, c1 = a[dx + 1] - ma1;
                saa0 = saa0 + c0 * c0;
                saa1 = saa1 + c1 * c1;
            }
        }
    }
    // (a window that leaves the image holds a NaN, and the comparison fails)
    const bool live0 = px < w && py < h && saa0 >= A.gate;
    const bool live1 = px + 1 < w && py < h && saa1 >= A.gate;
    const bool live = live0 || live1;

    double Rr[9], Cr[3];
    for (int i = 0; i < 9; ++i) Rr[i] = A.ref_pose[i];
    for (int i = 0; i < 3; ++i) Cr[i] = A.ref_pose[9 + i];

    Winner W0, W1;
    W0.init();
    W1.init();
    const double wmax = (double)(w - 1), hmax = (double)(h - 1);
    const int64_t plane_px = (int64_t)w * h;
    const bool in0 = px < w && py < h, in1 = px + 1 < w && py < h;
    const bool packed = (A.planes & 3) == 0;
    uint8_t *__restrict__ vol0 = VOL ? volume + ((int64_t)py * w + px) * A.planes : nullptr;
    uint32_t pk0 = 0, pk1 = 0;
    int buf = 0;
    int d_first = 0, d_end = A.planes;
    if constexpr (GUIDED) {
        const int32_t *__restrict__ e = windows + 2 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x);
        d_first = e[0];
        d_end = d_first + e[1];
    }
    for (int d = d_first; d < d_end; ++d) {
        const double z = 1.0 / (A.w_far + (double)d * A.step);
        float sum0 = 0.0f, sum1 = 0.0f;
        int cnt0 = 0, cnt1 = 0;
        for (int n = 0; n < A.n; ++n) {
            // ---- warp ----
            const Cam c = load_cam(A.nbr_cam + (int64_t)n * CAM);
            const float *__restrict__ G = A.nbr + n * plane_px;
            float *__restrict__ sw = s_warp[buf];
#pragma unroll
            for (int k = 0; k < NPOS; ++k) {
                if (pos_lds[k] < 0) continue;
                float val = qnan();
                if (pos_img[k] >= 0) {
                    double wn, we, wd, u, v, zc;
                    to_world(Rr, Cr, pos_xn[k] * z, pos_yn[k] * z, z, wn, we, wd);
                    project(c, wn, we, wd, u, v, zc);
                    if (zc > 0.0 && u >= 0.0 && u <= wmax && v >= 0.0 && v <= hmax) {
                        const double fx0 = floor(u), fy0 = floor(v);
                        const int x0 = (int)fx0, y0 = (int)fy0;
                        const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
                        const float tx_ = (float)(u - fx0), ty_ = (float)(v - fy0);
                        const float g00 = G[y0 * w + x0], g01 = G[y0 * w + x1];
                        const float g10 = G[y1 * w + x0], g11 = G[y1 * w + x1];
                        const float top = g00 + (g01 - g00) * tx_;
                        const float bot = g10 + (g11 - g10) * tx_;
                        val = top + (bot - top) * ty_;
                    }
                }
                sw[pos_lds[k]] = val;
            }
            __syncthreads();
            // ---- correlate ----
            if (live) {
                float sb0 = 0.0f, sb1 = 0.0f;
#pragma unroll UY
                for (int dy = 0; dy < K; ++dy) {
                    float b[2 * R + 2];
                    read_row<R>(sw + base + dy * PITCH, b);
#pragma unroll
                    for (int dx = 0; dx < K; ++dx) {
                        sb0 = sb0 + b[dx];
                        sb1 = sb1 + b[dx + 1];
                    }
                }
                const float mb0 = sb0 / N, mb1 = sb1 / N;
                float sbb0 = 0.0f, sbb1 = 0.0f, sab0 = 0.0f, sab1 = 0.0f;
#pragma unroll UY
                for (int dy = 0; dy < K; ++dy) {
                    float a[2 * R + 2], b[2 * R + 2];
                    read_row<R>(s_ref + base + dy * PITCH, a);
                    read_row<R>(sw + base + dy * PITCH, b);
#pragma unroll
                    for (int dx = 0; dx < K; ++dx) {
                        const float ca0 = a[dx] - ma0, cb0 = b[dx] - mb0;
                        const float ca1 = a[dx + 1] - ma1, cb1 = b[dx + 1] - mb1;
                        sbb0 = sbb0 + cb0 * cb0;
                        sab0 = sab0 + ca0 * cb0;
                        sbb1 = sbb1 + cb1 * cb1;
                        sab1 = sab1 + ca1 * cb1;
                    }
                }
                if (live0) {
                    const float den = (float)sqrt((double)(saa0 * sbb0));
                    const float s = sab0 / den;
                    if (den != 0.0f && s == s) { sum0 = sum0 + s; ++cnt0; }
                }
                if (live1) {
                    const float den = (float)sqrt((double)(saa1 * sbb1));
                    const float s = sab1 / den;
                    if (den != 0.0f && s == s) { sum1 = sum1 + s; ++cnt1; }
                }
            }
            buf ^= 1;
        }
        const float S0 = cnt0 > 0 ? sum0 / (float)cnt0 : qnan();
        W0.step(d, S0);
        const float S1 = cnt1 > 0 ? sum1 / (float)cnt1 : qnan();
        W1.step(d, S1);
        if constexpr (VOL) {
            const uint32_t c0 = cost_of(S0), c1 = cost_of(S1);
            if (packed) {
                pk0 |= c0 << (8 * (d & 3));
                pk1 |= c1 << (8 * (d & 3));
                if ((d & 3) == 3) {
                    if (in0) *reinterpret_cast<uint32_t *>(vol0 + (d - 3)) = pk0;
                    if (in1) *reinterpret_cast<uint32_t *>(vol0 + A.planes + (d - 3)) = pk1;
                    pk0 = pk1 = 0;
                }
            } else {
                if (in0) vol0[d] = (uint8_t)c0;
                if (in1) vol0[A.planes + d] = (uint8_t)c1;
            }
        }
    }
    if constexpr (GUIDED) {
        const int lo = d_first > 0 ? d_first : -2, hi = d_end < A.planes ? d_end - 1 : -2;   // (-2: a rim of the set)
        if (py < h) {
            if (px < w) write_pixel(A, py * w + px, W0, W0.best == lo || W0.best == hi);
            if (px + 1 < w) write_pixel(A, py * w + px + 1, W1, W1.best == lo || W1.best == hi);
        }
        return;
    }
    if (py < h) {
        if (px < w) write_pixel(A, py * w + px, W0);
        if (px + 1 < w) write_pixel(A, py * w + px + 1, W1);
    }
}

template <int R>
int launch_sweep(const SweepArgs &A, uint8_t *volume, const int32_t *windows, void *stream)
{
    const dim3 grid((A.w + TILE_W - 1) / TILE_W, (A.h + TILE_H - 1) / TILE_H);
    if (windows) {
        hipLaunchKernelGGL((sweep_kernel<R, false, true>), grid, dim3(THREADS), 0, iamx::as_stream(stream), A,
                           (uint8_t *)nullptr, windows);
        return iamx::check_launch("iamx_dense_sweep_guided");
    }
    if (volume) {
        hipLaunchKernelGGL((sweep_kernel<R, true>), grid, dim3(THREADS), 0, iamx::as_stream(stream), A, volume,
                           (const int32_t *)nullptr);
        return iamx::check_launch("iamx_dense_sweep_volume");
    }
    hipLaunchKernelGGL((sweep_kernel<R, false>), grid, dim3(THREADS), 0, iamx::as_stream(stream), A, (uint8_t *)nullptr,
                       (const int32_t *)nullptr);
    return iamx::check_launch("iamx_dense_sweep");
}

// ---- consistency ----
struct CheckArgs {
    const float *depth;          // [V][h][w]
    const double *rays;          // [V][h][w][2]
    const double *cams;          // [V][CAM]
    const int32_t *nbr;          // [V][M], -1: none
    int V, M, w, h;
    double eps;
    int min_agree;
    uint8_t *keep;               // [V][h][w]
    double *ned;                 // [V][h][w][3]
};

__global__ __launch_bounds__(THREADS) void check_kernel(CheckArgs A)
{
    const int64_t per = (int64_t)A.w * A.h;
    const int64_t g = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (g >= per * A.V) return;
    const int i = (int)(g / per);
    const float zf = A.depth[g];
    const double nan = (double)qnan();
    double pn = nan, pe = nan, pd = nan;
    uint8_t keep = 0;
    if (zf == zf) {
        const double z = (double)zf;
        const double *ci = A.cams + (int64_t)i * CAM;
        to_world(ci, ci + 9, A.rays[2 * g] * z, A.rays[2 * g + 1] * z, z, pn, pe, pd);
        int have = 0, agree = 0;
        for (int m = 0; m < A.M; ++m) {
            const int j = A.nbr[i * A.M + m];
            if (j < 0 || j >= A.V) continue;
            ++have;
            const Cam c = load_cam(A.cams + (int64_t)j * CAM);
            double u, v, zc;
            project(c, pn, pe, pd, u, v, zc);
            if (!(zc > 0.0)) continue;
            const double ru = rint(u), rv = rint(v);
            if (!(ru >= 0.0 && ru <= (double)(A.w - 1) && rv >= 0.0 && rv <= (double)(A.h - 1))) continue;
            const float zj = A.depth[j * per + (int64_t)rv * A.w + (int64_t)ru];
            if (!(zj == zj)) continue;
            if (fabs(zc - (double)zj) <= A.eps * zc) ++agree;
        }
        const int need = min(A.min_agree, have);
        keep = (have > 0 && agree >= need) ? 1 : 0;
    }
    A.keep[g] = keep;
    A.ned[3 * g] = pn;
    A.ned[3 * g + 1] = pe;
    A.ned[3 * g + 2] = pd;
}

// ---- fusion ----
__global__ __launch_bounds__(THREADS) void splat_kernel(const double *__restrict__ ned, const uint8_t *__restrict__ keep,
                                                        int64_t n, double x0, double y1, double gsd, int W, int H,
                                                        int32_t *__restrict__ count, int64_t *__restrict__ sum)
{
    const int64_t g = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (g >= n) return;
    if (keep && !keep[g]) return;
    const double north = ned[3 * g], east = ned[3 * g + 1], up = -ned[3 * g + 2];
    const double r = floor((y1 - north) / gsd), c = floor((east - x0) / gsd);
    const double q = rint(up * 1024.0);
    if (!(r >= 0.0 && r <= (double)(H - 1) && c >= 0.0 && c <= (double)(W - 1))) return;
    if (!(fabs(q) <= 1e15)) return;                   // (NaN too)
    const int64_t cell = (int64_t)r * W + (int64_t)c;
    atomicAdd(reinterpret_cast<int *>(count + cell), 1);
    atomicAdd(reinterpret_cast<unsigned long long *>(sum + cell), (unsigned long long)(long long)q);
}

__global__ __launch_bounds__(THREADS) void resolve_kernel(const int32_t *__restrict__ count, const int64_t *__restrict__ sum,
                                                          int64_t cells, float *__restrict__ dsm)
{
    const int64_t g = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (g >= cells) return;
    const int32_t c = count[g];
    dsm[g] = c > 0 ? (float)((double)sum[g] / 1024.0 / (double)c) : qnan();
}

}  // namespace

static int dense_sweep_entry(const float *ref, const double *rays, const float *nbr, const double *ref_pose,
                                const double *nbr_cam, int width, int height, int num_nbr, int planes,
                                double w_far, double w_near, int radius, float min_var, float min_score,
                                int32_t *plane, float *score, float *depth, float *around, uint8_t *volume,
                                const int32_t *windows, void *stream)
{
    if (windows)
        IAMX_REQUIRE(planes >= 2 && planes <= IAMX_DENSE_GUIDED_MAX_PLANES, "planes_total out of range");
    else
        IAMX_REQUIRE(planes >= 1 && planes <= IAMX_DENSE_MAX_PLANES, "planes out of range");
    IAMX_REQUIRE(radius >= 1 && radius <= IAMX_DENSE_MAX_RADIUS, "radius out of range");
    IAMX_REQUIRE(num_nbr >= 1 && num_nbr <= IAMX_DENSE_MAX_NEIGHBOURS, "neighbour count out of range");
    IAMX_REQUIRE(width >= 1 && height >= 1 && width <= IAMX_DENSE_MAX_SIDE && height <= IAMX_DENSE_MAX_SIDE,
                 "image size out of range");
    IAMX_REQUIRE(w_far > 0.0 && w_near > w_far && w_near < INFINITY, "0 < w_far < w_near wanted");
    IAMX_REQUIRE(ref && rays && nbr && ref_pose && nbr_cam && plane && score && depth && around, "null pointer");
    if (windows) {
        // the table is small (8 bytes per tile): read it back and refuse an entry outside the plane set
        const size_t tiles = (size_t)((width + TILE_W - 1) / TILE_W) * (size_t)((height + TILE_H - 1) / TILE_H);
        std::vector<int32_t> tab(2 * tiles);
        hipStream_t s = iamx::as_stream(stream);
        if (hipMemcpyAsync(tab.data(), windows, tab.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) {
            (void)hipGetLastError();
            return iamx::fail(IAMX_ELAUNCH, "%s: the window table could not be read", "iamx_dense_sweep_guided");
        }
        for (size_t t = 0; t < tiles; ++t) {
            const int64_t first = tab[2 * t], count = tab[2 * t + 1];
            if (first < 0 || count < 0 || first + count > planes)
                return iamx::fail(IAMX_EINVAL, "%s: window %zu = (%d, %d) leaves the %d planes", "iamx_dense_sweep_guided",
                                  t, (int)first, (int)count, planes);
        }
    }
    SweepArgs A;
    A.ref = ref; A.rays = rays; A.nbr = nbr; A.ref_pose = ref_pose; A.nbr_cam = nbr_cam;
    A.w = width; A.h = height; A.n = num_nbr; A.planes = planes;
    A.w_far = w_far;
    A.step = planes > 1 ? (w_near - w_far) / (double)(planes - 1) : 0.0;
    const int side = 2 * radius + 1;
    A.gate = min_var * (float)(side * side);
    A.min_score = min_score;
    A.plane = plane; A.score = score; A.depth = depth; A.around = around;
    switch (radius) {
        case 1: return launch_sweep<1>(A, volume, windows, stream);
        case 2: return launch_sweep<2>(A, volume, windows, stream);
        case 3: return launch_sweep<3>(A, volume, windows, stream);
        case 4: return launch_sweep<4>(A, volume, windows, stream);
        case 5: return launch_sweep<5>(A, volume, windows, stream);
        case 6: return launch_sweep<6>(A, volume, windows, stream);
        default: return launch_sweep<7>(A, volume, windows, stream);
    }
}

extern "C" int iamx_dense_sweep(const float *ref, const double *rays, const float *nbr, const double *ref_pose,
                                const double *nbr_cam, int width, int height, int num_nbr, int planes,
                                double w_far, double w_near, int radius, float min_var, float min_score,
                                int32_t *plane, float *score, float *depth, float *around, void *stream)
{
    return dense_sweep_entry(ref, rays, nbr, ref_pose, nbr_cam, width, height, num_nbr, planes, w_far, w_near, radius,
                             min_var, min_score, plane, score, depth, around, nullptr, nullptr, stream);
}

extern "C" int iamx_dense_sweep_guided(const float *ref, const double *rays, const float *nbr, const double *ref_pose,
                                       const double *nbr_cam, int width, int height, int num_nbr, int planes_total,
                                       double w_far, double w_near, int radius, float min_var, float min_score,
                                       const int32_t *windows, int32_t *plane, float *score, float *depth, float *around,
                                       void *stream)
{
    IAMX_REQUIRE(windows, "null pointer");
    return dense_sweep_entry(ref, rays, nbr, ref_pose, nbr_cam, width, height, num_nbr, planes_total, w_far, w_near,
                             radius, min_var, min_score, plane, score, depth, around, nullptr, windows, stream);
}

extern "C" int iamx_dense_sweep_volume(const float *ref, const double *rays, const float *nbr, const double *ref_pose,
                                       const double *nbr_cam, int width, int height, int num_nbr, int planes,
                                       double w_far, double w_near, int radius, float min_var, float min_score,
                                       int32_t *plane, float *score, float *depth, float *around, uint8_t *volume,
                                       void *stream)
{
    IAMX_REQUIRE(planes >= 2 && planes <= IAMX_DENSE_SGM_MAX_PLANES, "planes out of range for a cost volume");
    IAMX_REQUIRE(volume, "null pointer");
    IAMX_REQUIRE(((uintptr_t)volume & 3) == 0, "the volume is aligned to 4 bytes");
    return dense_sweep_entry(ref, rays, nbr, ref_pose, nbr_cam, width, height, num_nbr, planes, w_far, w_near, radius,
                             min_var, min_score, plane, score, depth, around, volume, nullptr, stream);
}

extern "C" int iamx_dense_check(const float *depth, const double *rays, const double *cams, const int32_t *nbr,
                                int num_views, int max_nbr, int width, int height, double eps, int min_agree,
                                uint8_t *keep, double *ned, void *stream)
{
    IAMX_REQUIRE(num_views >= 0 && max_nbr >= 1 && max_nbr <= IAMX_DENSE_MAX_NEIGHBOURS, "bad count");
    IAMX_REQUIRE(width >= 1 && height >= 1 && width <= IAMX_DENSE_MAX_SIDE && height <= IAMX_DENSE_MAX_SIDE,
                 "image size out of range");
    IAMX_REQUIRE(eps >= 0.0 && min_agree >= 1, "eps >= 0 and min_agree >= 1 wanted");
    const int64_t total = (int64_t)num_views * width * height;
    IAMX_REQUIRE(total < ((int64_t)1 << 31) * THREADS, "too many pixels for one call");
    if (num_views == 0) return IAMX_OK;
    IAMX_REQUIRE(depth && rays && cams && nbr && keep && ned, "null pointer");
    CheckArgs A;
    A.depth = depth; A.rays = rays; A.cams = cams; A.nbr = nbr;
    A.V = num_views; A.M = max_nbr; A.w = width; A.h = height;
    A.eps = eps; A.min_agree = min_agree; A.keep = keep; A.ned = ned;
    hipLaunchKernelGGL(check_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0,
                       iamx::as_stream(stream), A);
    return iamx::check_launch("iamx_dense_check");
}

extern "C" int iamx_dense_splat(const double *ned, const uint8_t *keep, int64_t num_points, double x0, double y1,
                                double gsd, int width, int height, int32_t *count, int64_t *sum, void *stream)
{
    IAMX_REQUIRE(num_points >= 0 && num_points < ((int64_t)1 << 31) * THREADS, "bad point count");
    IAMX_REQUIRE(width >= 1 && height >= 1 && width <= IAMX_DENSE_MAX_RASTER && height <= IAMX_DENSE_MAX_RASTER,
                 "raster size out of range");
    IAMX_REQUIRE(gsd > 0.0 && gsd < INFINITY && x0 == x0 && y1 == y1, "bad raster frame");
    if (num_points == 0) return IAMX_OK;
    IAMX_REQUIRE(ned && count && sum, "null pointer");
    hipLaunchKernelGGL(splat_kernel, dim3((unsigned)((num_points + THREADS - 1) / THREADS)), dim3(THREADS), 0,
                       iamx::as_stream(stream), ned, keep, num_points, x0, y1, gsd, width, height, count, sum);
    return iamx::check_launch("iamx_dense_splat");
}

extern "C" int iamx_dense_resolve(const int32_t *count, const int64_t *sum, int width, int height, float *dsm,
                                  void *stream)
{
    IAMX_REQUIRE(width >= 1 && height >= 1 && width <= IAMX_DENSE_MAX_RASTER && height <= IAMX_DENSE_MAX_RASTER,
                 "raster size out of range");
    IAMX_REQUIRE(count && sum && dsm, "null pointer");
    const int64_t cells = (int64_t)width * height;
    hipLaunchKernelGGL(resolve_kernel, dim3((unsigned)((cells + THREADS - 1) / THREADS)), dim3(THREADS), 0,
                       iamx::as_stream(stream), count, sum, cells, dsm);
    return iamx::check_launch("iamx_dense_resolve");
}
