// The 'bruteforce' strategy on the device (gfx950) -- scripts/lib/matcher.py:696-850
// bruteforce_pair_matches(), ONE direction of an image pair, one workgroup per pair:
//
//   matcher.py:711-754   per query row, over its <= 3 neighbours: break at distance >= 290, break at
//                        ratio < match_ratio, skip size_diff > 1.25, the smallest
//                        metric = size_diff / ratio (the first survivor always taken); the choice's
//                        image-space motion v = kp2.pt - kp1.pt gives raw_dist and vangle
//   matcher.py:756-773   41 distance bins of step int(diag * 0.55) / 40, a row in its bin and both
//                        neighbours; a row past bin 40 is in none
//   matcher.py:776-795   per distance bin 21 angle bins of step 2 pi / 20, a row in its bin and both
//                        neighbours, bins 0 and 20 wrapping the way the reference wraps them
//   matcher.py:796-797   a cell below min_pairs is not looked at
//   matcher.py:798-807   src / dst = kp.pt of the cell's matches -> cv2.findHomography(RANSAC, tol)
//   matcher.py:808-817   strictly more fitted inliers than the best so far (0 at the start) wins
//   matcher.py:833       after a distance bin: stop at best > 50 and best_of_bin < 10
//   matcher.py:839-850   len(best) >= min_pairs, filter_duplicates, >= min_pairs again
//
// iamx_brute_bins materialises the looked-at cells in query-row order (points in the layout
// iamx_verify_pairs reads), the caller runs iamx_verify_pairs over the n_pairs * 861 segments,
// iamx_brute_select walks the masks with the early exit.  The consensus is this package's rule
// (csrc/verify_rule.h), not cv2's: parity UNPINNED there.
//
// No contraction anywhere in this file: every expression rounds as the Python it restates.  The
// pragma below is this source's -ffp-contract=off (the build's table of per-file flags stays as it is).
#include "iamx_common.h"
#include "bin_select.h"

// (It covers what follows it in THIS file.  The headers above hold no floating-point arithmetic.)
#pragma clang fp contract(off)

namespace {

using namespace iamx_bs;          // NT = 256, gate(), WorkSlice, take_list(), scan_and_pack()
constexpr int ND = IAMX_BRUTE_DIST_BINS, NA = IAMX_BRUTE_ANGLE_BINS, NC = IAMX_BRUTE_CELLS;
constexpr int CHUNK = 2048;                // rows whose cell codes are held in LDS at a time
constexpr int OWN = (NC + NT - 1) / NT;    // cells a thread of the fill kernel owns
static_assert(ND == 41 && NA == 21 && NC == ND * NA, "41 distance bins x 21 angle bins");

struct BinArgs {
    const int32_t *idx, *d2;           // [rows][3] iamx_knn3_l2_pairs
    const int64_t *row_off;            // [n_pairs + 1]
    const int32_t *pairs;              // [n_pairs][2] image slots (query, train)
    const int64_t *kp_off;
    const float *xy, *size;            // kp.pt [total kp][2], kp.size [total kp]
    double match_ratio, min_pairs, step_d, step_a;
    int64_t cap;
    int32_t *bin_cnt, *seg_cnt;        // [n_pairs][NC]
    const int64_t *seg_off;
    float *pts;
    int32_t *rows;
    int32_t *flag;
};

// matcher.py:711-795 for query row i: (distance bin << 8 | angle bin) of the row's choice and its
// train row; -1 where no neighbour survives or the choice lies past the last distance bin.
// zero: the nearest distance is 0.
__device__ __forceinline__ int choose(const int32_t *__restrict__ nn, const int32_t *__restrict__ dd,
                                      int i, const float *__restrict__ xq, const float *__restrict__ xt,
                                      const float *__restrict__ sq, const float *__restrict__ st,
                                      const BinArgs &A, int &train, bool &zero)
{
    train = -1;
    const int d0 = dd[0];
    zero = d0 == 0;
    if (zero) return -1;                   // python divides 0.0 by 0.0 at j = 0: ZeroDivisionError
    // cv2's DMatch.distance: float32 sqrt of the exact squared distance (csrc/match_knn2.hip)
    const float f0 = (float)sqrt((double)d0);
    const float x1 = xq[2 * i], y1 = xq[2 * i + 1];
    const double s1 = (double)sq[i];
    int best = -1;
    double best_metric = 0.0;
    float best_raw = 0.0f, bvx = 0.0f, bvy = 0.0f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int dj = dd[j];
        if (dj >= 84100) break;            // m[j].distance >= 290 (a missing neighbour too)
        const double ratio = (double)f0 / (double)(float)sqrt((double)dj);
        if (ratio < A.match_ratio) break;
        const int t = nn[j];
        const float vx = xt[2 * t] - x1, vy = xt[2 * t + 1] - y1;
        const float raw = (float)sqrt((double)(vx * vx + vy * vy));     // np.linalg.norm of float32
        const double s2 = (double)st[t];
        const double size_diff = s1 > s2 ? s1 / s2 : s2 / s1;
        if (size_diff > 1.25) continue;
        const double metric = size_diff / ratio;
        if (best < 0 || metric < best_metric) {
            best = j;
            best_metric = metric;
            best_raw = raw;
            bvx = vx;
            bvy = vy;
            train = t;
        }
    }
    if (best < 0) return -1;
    // NumPy 1.20 (the reference's): np.float32 / float is a float64 quotient
    const double qd = rint((double)best_raw / A.step_d);
    if (!(qd <= (double)(ND - 1))) return -1;                           // bin < len(dist_bins); a NaN
    double vangle = atan2((double)bvy, (double)bvx);
    if (vangle < 0.0) vangle += 2.0 * 3.141592653589793;
    const double qa = rint(vangle / A.step_a);
    if (!(qa >= 0.0 && qa <= (double)(NA - 1))) return -1;              // (never for finite points)
    return ((int)qd << 8) | (int)qa;
}

// is a row whose choice has angle bin `ra` in angle bin `ca`?  (matcher.py:785-795, wraps included)
__device__ __forceinline__ bool in_angle(int ra, int ca)
{
    if (ra == 0) return ca == NA - 1 || ca == 0 || ca == 1;
    if (ra == NA - 1) return ca == NA - 2 || ca == NA - 1 || ca == 0;
    return ca >= ra - 1 && ca <= ra + 1;
}

struct PairCtx {
    int64_t b0;
    int n;
    bool oversize;
    const float *xq, *xt, *sq, *st;
};

__device__ __forceinline__ PairCtx pair_ctx(const BinArgs &A, int p)
{
    PairCtx c;
    c.b0 = A.row_off[p];
    const int64_t n64 = A.row_off[p + 1] - c.b0;
    c.oversize = n64 < 0 || n64 > MAX_ROWS;
    c.n = c.oversize ? 0 : (int)n64;
    const int64_t oq = A.kp_off[A.pairs[2 * p]], ot = A.kp_off[A.pairs[2 * p + 1]];
    c.xq = A.xy + 2 * oq; c.xt = A.xy + 2 * ot;
    c.sq = A.size + oq; c.st = A.size + ot;
    return c;
}

__global__ __launch_bounds__(NT) void brute_count_kernel(BinArgs A)
{
    __shared__ int hist[NC];
    const int p = blockIdx.x;
    const PairCtx c = pair_ctx(A, p);
    for (int k = threadIdx.x; k < NC; k += NT) hist[k] = 0;
    __syncthreads();
    int zd = 0;
    for (int i = threadIdx.x; i < c.n; i += NT) {
        bool zero;
        int t;
        const int code = choose(A.idx + 3 * (c.b0 + i), A.d2 + 3 * (c.b0 + i), i, c.xq, c.xt, c.sq, c.st,
                                A, t, zero);
        zd += zero ? 1 : 0;
        if (code < 0) continue;
        const int rd = code >> 8, ra = code & 255;
        const int a0 = ra == 0 ? NA - 1 : ra - 1, a2 = ra == NA - 1 ? 0 : ra + 1;
        for (int cd = rd > 0 ? rd - 1 : 0; cd <= (rd < ND - 1 ? rd + 1 : ND - 1); ++cd) {
            atomicAdd(&hist[cd * NA + a0], 1);
            atomicAdd(&hist[cd * NA + ra], 1);
            atomicAdd(&hist[cd * NA + a2], 1);
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) zd += __shfl_xor(zd, s);
    if ((threadIdx.x & 63) == 0 && zd) atomicAdd(A.flag, zd);
    if (threadIdx.x == 0 && c.oversize) atomicAdd(A.flag + 1, 1);
    __syncthreads();
    for (int k = threadIdx.x; k < NC; k += NT) {
        const int m = hist[k];
        A.bin_cnt[(int64_t)p * NC + k] = m;
        A.seg_cnt[(int64_t)p * NC + k] = gate(m, A.min_pairs) ? m : 0;
    }
}

// Query-row order within every cell by construction: a chunk's cell codes go to LDS, then every
// thread walks the chunk in row order for the (up to four) cells it owns, alone.
__global__ __launch_bounds__(NT) void brute_fill_kernel(BinArgs A)
{
    __shared__ int code[CHUNK], trn[CHUNK];
    const int p = blockIdx.x;
    int cd[OWN], ca[OWN], pos[OWN];
    int64_t first[OWN];
    unsigned on = 0;
#pragma unroll
    for (int k = 0; k < OWN; ++k) {
        const int cell = threadIdx.x + k * NT;
        cd[k] = cell / NA;
        ca[k] = cell % NA;
        pos[k] = 0;
        first[k] = 0;
        if (cell < NC && A.seg_cnt[(int64_t)p * NC + cell] > 0) {
            on |= 1u << k;
            first[k] = A.seg_off[(int64_t)p * NC + cell];
        }
    }
    if (!__syncthreads_or((int)on)) return;
    const PairCtx c = pair_ctx(A, p);
    for (int s = 0; s < c.n; s += CHUNK) {
        const int m = c.n - s < CHUNK ? c.n - s : CHUNK;
        for (int r = threadIdx.x; r < m; r += NT) {
            const int i = s + r;
            bool zero;
            int t;
            code[r] = choose(A.idx + 3 * (c.b0 + i), A.d2 + 3 * (c.b0 + i), i, c.xq, c.xt, c.sq, c.st, A,
                             t, zero);
            trn[r] = t;
        }
        __syncthreads();
        if (on) {
            for (int r = 0; r < m; ++r) {
                const int cr = code[r];                     // (an LDS broadcast: every lane reads row r)
                if (cr < 0) continue;
                const int rd = cr >> 8, ra = cr & 255;
#pragma unroll
                for (int k = 0; k < OWN; ++k) {
                    if (!((on >> k) & 1) || cd[k] < rd - 1 || cd[k] > rd + 1 || !in_angle(ra, ca[k])) continue;
                    const int64_t o = first[k] + pos[k]++;
                    if (o < 0 || o >= A.cap) continue;      // (never: cap >= 9 * rows)
                    const int i = s + r, t = trn[r];
                    *reinterpret_cast<float4 *>(A.pts + 4 * o) =
                        make_float4(c.xq[2 * i], c.xq[2 * i + 1], c.xt[2 * t], c.xt[2 * t + 1]);
                    *reinterpret_cast<v2i *>(A.rows + 2 * o) = v2i{i, t};
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------
// the walk over the cells
// ---------------------------------------------------------------------------------
struct SelArgs {
    const int32_t *pairs;              // [n_pairs][2] image slots (query, train)
    const int64_t *kp_off;
    const int32_t *key2;               // [total kp][2] round-half-even(100 * kp.pt) ("%.2f")
    double min_pairs;
    const int32_t *seg_cnt;            // [n_pairs][NC]
    const int64_t *seg_off;            // [n_pairs * NC + 1]
    const int32_t *rows;               // [cap][2]
    const uint8_t *mask;               // [cap] iamx_verify_pairs
    const int32_t *vstatus;            // [n_pairs * NC]
    int64_t cap;
    int stride, tab_size;
    int32_t *work;                     // [n_pairs][6 * stride + 2 * tab_size]
    int32_t *out_slots;                // [n_pairs][stride][2]
    int32_t *out_cnt, *chosen, *stats; // [n_pairs], [n_pairs], [n_pairs][4]
    int32_t *fit_cnt;                  // [n_pairs][NC]
    int32_t *flag;
};

__global__ __launch_bounds__(NT) void brute_select_kernel(SelArgs A)
{
    __shared__ int red[NT / 64];
    __shared__ int fit[NA];
    const int p = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WorkSlice W(A.work, p, A.stride, A.tab_size);
    const PairKeys K(A.key2, A.kp_off, A.pairs, p);
    int32_t *out = A.out_slots + (int64_t)p * A.stride * 2;
    int32_t *fc = A.fit_cnt + (int64_t)p * NC;
    for (int k = threadIdx.x; k < NC; k += NT) fc[k] = -1;              // not looked at, or not reached
    int best = 0, chosen = -1, walked = 0, looked = 0;
    bool refused = false;
    for (int d = 0; d < ND; ++d) {
        // the fitted inliers of the distance bin's cells, a wave per cell
        for (int a = wave; a < NA; a += NT / 64) {
            const int64_t seg = (int64_t)p * NC + d * NA + a;
            const int n = A.seg_cnt[seg];
            const int64_t o = A.seg_off[seg];
            int c = -1;
            if (n > 0) {
                if (n > A.stride || o < 0 || o + n > A.cap) {
                    c = -2;                                 // (never: the caller sizes stride and cap)
                } else {
                    c = 0;
                    // a cell without a model (IAMX_VERIFY_NO_MODEL) has no inliers
                    if (A.vstatus[seg] == IAMX_VERIFY_OK)
                        for (int i = lane; i < n; i += 64) c += A.mask[o + i] != 0;
#pragma unroll
                    for (int s = 32; s >= 1; s >>= 1) c += __shfl_xor(c, s);
                }
            }
            if (lane == 0) fit[a] = c;
        }
        __syncthreads();
        int best_of_bin = 0;
        for (int a = 0; a < NA; ++a) {
            const int nf = fit[a];
            if (nf == -2) refused = true;
            if (nf < 0) continue;
            ++looked;
            if (nf > best_of_bin) best_of_bin = nf;
            if (nf > best) {                                // strictly more fitted (matcher.py:810)
                best = nf;
                chosen = d * NA + a;
            }
        }
        if (threadIdx.x < NA && fit[threadIdx.x] >= 0) fc[d * NA + threadIdx.x] = fit[threadIdx.x];
        __syncthreads();
        walked = d + 1;
        if (best > 50 && best_of_bin < 10) break;           // matcher.py:833
    }
    // matcher.py:839-850: the fitted list, then the de-duplicated one, against min_pairs
    int uniq = -1, cnt = 0;
    if (!refused && chosen >= 0 && (double)best >= A.min_pairs) {
        const int64_t o = A.seg_off[(int64_t)p * NC + chosen];
        const int n = A.seg_cnt[(int64_t)p * NC + chosen];
        const auto enough = [&](int u) { return (double)u >= A.min_pairs; };
        uniq = take_list(red, A.mask + o, A.rows + 2 * o, n, K, W, out, enough).y;
        if (enough(uniq)) cnt = uniq;
    }
    if (threadIdx.x == 0) {
        A.out_cnt[p] = cnt;
        A.chosen[p] = refused ? -1 : chosen;
        A.stats[4 * p] = best;
        A.stats[4 * p + 1] = uniq;
        A.stats[4 * p + 2] = walked;
        A.stats[4 * p + 3] = looked;
        if (refused) atomicAdd(A.flag + 1, 1);
    }
}

}  // namespace

extern "C" int iamx_brute_bins(const int32_t *idx, const int32_t *d2, const int64_t *row_off,
                               const int32_t *pairs, const int64_t *kp_off, const float *xy,
                               const float *size, int n_pairs, double match_ratio, double min_pairs,
                               double step_d, double step_a, int64_t cap, int32_t *bin_cnt,
                               int32_t *seg_cnt, int64_t *seg_off, float *pts, int32_t *rows,
                               int32_t *flag, void *stream)
{
    IAMX_REQUIRE(idx && d2 && row_off && pairs && kp_off && xy && size && bin_cnt && seg_cnt && seg_off &&
                     pts && rows && flag,
                 "null pointer");
    IAMX_REQUIRE(n_pairs >= 0 && cap >= 0, "negative count");
    IAMX_REQUIRE((int64_t)n_pairs * NC < (1ll << 31), "too many segments");
    IAMX_REQUIRE(((uintptr_t)pts & 15) == 0, "pts must be 16-byte aligned");
    IAMX_REQUIRE(match_ratio == match_ratio, "match_ratio is not a number");
    IAMX_REQUIRE(step_d > 0.0 && step_d <= 1.7e308 && step_a > 0.0 && step_a <= 1.7e308,
                 "the bin steps must be positive and finite");
    if (n_pairs == 0) return IAMX_OK;
    hipStream_t st = iamx::as_stream(stream);
    BinArgs A{idx, d2, row_off, pairs, kp_off, xy, size, match_ratio, min_pairs, step_d, step_a, cap,
              bin_cnt, seg_cnt, seg_off, pts, rows, flag};
    hipLaunchKernelGGL(brute_count_kernel, dim3((unsigned)n_pairs), dim3(NT), 0, st, A);
    int rc = iamx::check_launch("iamx_brute_bins");
    if (rc != IAMX_OK) return rc;
    rc = iamx_exclusive_scan_i32(seg_cnt, (int64_t)n_pairs * NC, seg_off, stream);
    if (rc != IAMX_OK) return rc;
    hipLaunchKernelGGL(brute_fill_kernel, dim3((unsigned)n_pairs), dim3(NT), 0, st, A);
    return iamx::check_launch("iamx_brute_bins");
}

extern "C" int iamx_brute_select(const int32_t *pairs, const int64_t *kp_off, const int32_t *key2,
                                 int n_pairs, double min_pairs, const int32_t *seg_cnt,
                                 const int64_t *seg_off, const int32_t *rows, const uint8_t *mask,
                                 const int32_t *vstatus, int64_t cap, int stride, int tab_size,
                                 int32_t *work, int32_t *out_slots, int32_t *out_cnt, int64_t *out_off,
                                 int32_t *out_rows, int64_t out_cap, int32_t *chosen, int32_t *stats,
                                 int32_t *fit_cnt, int32_t *flag, void *stream)
{
    IAMX_REQUIRE(pairs && kp_off && key2 && seg_cnt && seg_off && rows && mask && vstatus && work &&
                     out_slots && out_cnt && out_off && out_rows && chosen && stats && fit_cnt && flag,
                 "null pointer");
    IAMX_REQUIRE(n_pairs >= 0 && cap >= 0 && out_cap >= 0, "negative count");
    IAMX_REQUIRE((int64_t)n_pairs * NC < (1ll << 31), "too many segments");
    IAMX_REQUIRE_WORK_SLICE(stride, tab_size);
    if (n_pairs == 0) return IAMX_OK;                       // (nothing is written, out_off[0] included)
    hipStream_t st = iamx::as_stream(stream);
    SelArgs A{pairs, kp_off, key2, min_pairs, seg_cnt, seg_off, rows, mask, vstatus, cap, stride,
              tab_size, work, out_slots, out_cnt, chosen, stats, fit_cnt, flag};
    hipLaunchKernelGGL(brute_select_kernel, dim3((unsigned)n_pairs), dim3(NT), 0, st, A);
    const int rc = iamx::check_launch("iamx_brute_select");
    if (rc != IAMX_OK) return rc;
    return scan_and_pack("iamx_brute_select", n_pairs, out_cnt, out_off, out_slots, stride, out_rows,
                         out_cap, stream);
}
