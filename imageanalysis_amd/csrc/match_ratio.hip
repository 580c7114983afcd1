// The 'bestratio' strategy on the device (gfx950) -- scripts/lib/matcher.py:595-694
// ratio_pair_matches(), ONE direction of an image pair, one workgroup per pair:
//
//   matcher.py:618-620   ratio = m[0].distance / m[1].distance (float32 distances, f64 division)
//   matcher.py:622-630   eight nested bins, ratio <= cutoff, in query-row order
//   matcher.py:634       a bin below min_pairs is not looked at
//   matcher.py:635-637   src / dst = kp.pt of the bin's matches -> cv2.findHomography(RANSAC, tol)
//   matcher.py:638-645   the inliers in order, count_unique() = len(filter_duplicates())
//   matcher.py:647-659   strictly more unique inliers than the best so far (20 at the start) wins
//   matcher.py:683-694   len(best) >= min_pairs, filter_duplicates, >= min_pairs again
//
// iamx_ratio_bins materialises the bins (points in the layout iamx_verify_pairs reads), the caller
// runs iamx_verify_pairs over the n_pairs * n_bins segments, iamx_ratio_select reads the masks.
// The consensus is this package's rule (csrc/verify_rule.h), not cv2's: parity UNPINNED there.
//
// There is no clip on this path: a list is as long as the query image has rows.  Nothing of a
// pair is therefore kept in LDS; the de-duplication's key tables and work lists are per-pair
// slices of a global scratch the caller sizes (stride = rows of the largest query image of the
// launch, tab_size = a power of two >= 2 * stride).
#include "iamx_common.h"
#include "bin_select.h"

namespace {

using namespace iamx_bs;          // NT = 256, gate(), the bin kernels, walk_bins(), scan_and_pack()
constexpr int MAXB = 8;

struct Cut { double c[MAXB]; };

// the bins a row belongs to (bit b: ratio <= cutoff b); zero: the second distance is 0
__device__ __forceinline__ unsigned bin_mask(v2i dd, const Cut &C, int nb, bool &zero)
{
    // cv2's DMatch.distance: float32 sqrt of the exact squared distance (csrc/match_knn2.hip)
    const float d0 = (float)sqrt((double)dd.x), d1 = (float)sqrt((double)dd.y);
    zero = d1 == 0.0f;
    if (zero) return 0u;                   // python raises ZeroDivisionError at this row
    const double ratio = (double)d0 / (double)d1;
    unsigned m = 0;
#pragma unroll
    for (int b = 0; b < MAXB; ++b)
        if (b < nb && ratio <= C.c[b]) m |= 1u << b;
    return m;
}

struct BinArgs {
    const int32_t *idx, *d2;           // [rows][2] iamx_knn2_l2_pairs
    const int64_t *row_off;            // [n_pairs + 1]
    const int32_t *pairs;              // [n_pairs][2] image slots (query, train)
    const int64_t *kp_off;
    const float *xy;                   // kp.pt [total kp][2]
    int nb;
    Cut C;
    double min_pairs;
    int64_t cap;
    int32_t *bin_cnt, *seg_cnt;        // [n_pairs][nb]
    const int64_t *seg_off;
    float *pts;
    int32_t *rows;
    int32_t *flag;
};

// the row rule of bin_select.h's bin kernels (idx is read for a row in a looked-at bin only)
struct RatioRule {
    typedef BinArgs Args;
    static __device__ __forceinline__ int n_bins(const BinArgs &A) { return A.nb; }
    const BinArgs &A;
    int64_t b0;
    int n;
    bool oversize;
    const float *xq, *xt;
    __device__ __forceinline__ RatioRule(const BinArgs &A_, int p) : A(A_)
    {
        b0 = A.row_off[p];
        const int64_t n64 = A.row_off[p + 1] - b0;
        oversize = n64 < 0 || n64 > MAX_ROWS;
        n = oversize ? 0 : (int)n64;
        xq = A.xy + 2 * A.kp_off[A.pairs[2 * p]];
        xt = A.xy + 2 * A.kp_off[A.pairs[2 * p + 1]];
    }
    __device__ __forceinline__ unsigned bins(int i, bool &zero, int &) const
    {
        return bin_mask(*reinterpret_cast<const v2i *>(A.d2 + 2 * (b0 + i)), A.C, A.nb, zero);
    }
    __device__ __forceinline__ float4 point(int i, int &t) const
    {
        t = A.idx[2 * (b0 + i)];
        return make_float4(xq[2 * i], xq[2 * i + 1], xt[2 * t], xt[2 * t + 1]);
    }
};

struct SelArgs {
    const int32_t *pairs;              // [n_pairs][2] image slots (query, train)
    const int64_t *kp_off;             // [n_images] first keypoint of every image slot
    const int32_t *key2;               // [total kp][2] round-half-even(100 * kp.pt) ("%.2f")
    int nb;
    double min_pairs;
    int min_unique;                    // best_fitted_matches of matcher.py:603
    Segments S;
    int tab_size;
    int32_t *work;                     // [n_pairs][6 * stride + 2 * tab_size]
    int32_t *out_slots;                // [n_pairs][stride][2]
    int32_t *out_cnt, *chosen, *stats; // [n_pairs], [n_pairs], [n_pairs][nb][3]
    int32_t *flag;
};

// matcher.py:647-659: the walk starts at min_unique
__global__ __launch_bounds__(NT) void ratio_select_kernel(SelArgs A)
{
    __shared__ int red[NT / 64];
    const int p = blockIdx.x;
    const Walked w = walk_bins(red, A.S, p, A.nb, A.min_pairs, PairKeys(A.key2, A.kp_off, A.pairs, p),
                               WorkSlice(A.work, p, A.S.stride, A.tab_size),
                               A.out_slots + (int64_t)p * A.S.stride * 2, A.stats + (int64_t)p * A.nb * 3,
                               A.min_unique, 0);
    if (threadIdx.x == 0) {
        // matcher.py:683-694: the fitted list, then the de-duplicated one, against min_pairs
        const bool ok = !w.refused && w.taken && (double)w.best_fit >= A.min_pairs && (double)w.best >= A.min_pairs;
        A.out_cnt[p] = ok ? w.best : 0;
        A.chosen[p] = w.refused ? -1 : w.taken - 1;
        if (w.refused) atomicAdd(A.flag + 1, 1);
    }
}

bool cut_ok(const double *cutoffs, int nb, Cut &C)
{
    for (int b = 0; b < MAXB; ++b) C.c[b] = b < nb ? cutoffs[b] : 0.0;
    for (int b = 0; b < nb; ++b)
        if (!(C.c[b] == C.c[b]) || (b && C.c[b] < C.c[b - 1])) return false;
    return true;
}

}  // namespace

extern "C" int iamx_ratio_bins(const int32_t *idx, const int32_t *d2, const int64_t *row_off,
                               const int32_t *pairs, const int64_t *kp_off, const float *xy,
                               int n_pairs, int n_bins, const double *cutoffs, double min_pairs,
                               int64_t cap, int32_t *bin_cnt, int32_t *seg_cnt, int64_t *seg_off,
                               float *pts, int32_t *rows, int32_t *flag, void *stream)
{
    IAMX_REQUIRE(idx && d2 && row_off && pairs && kp_off && xy && cutoffs && bin_cnt && seg_cnt &&
                     seg_off && pts && rows && flag,
                 "null pointer");
    IAMX_REQUIRE(n_pairs >= 0 && cap >= 0, "negative count");
    IAMX_REQUIRE(n_bins >= 1 && n_bins <= MAXB, "n_bins outside 1..8");
    IAMX_REQUIRE((int64_t)n_pairs * n_bins < (1ll << 31), "too many segments");
    IAMX_REQUIRE(((uintptr_t)pts & 15) == 0, "pts must be 16-byte aligned");
    Cut C;
    IAMX_REQUIRE(cut_ok(cutoffs, n_bins, C), "cutoffs must ascend");
    if (n_pairs == 0) return IAMX_OK;
    hipStream_t st = iamx::as_stream(stream);
    BinArgs A{idx, d2, row_off, pairs, kp_off, xy, n_bins, C, min_pairs, cap, bin_cnt, seg_cnt, seg_off,
              pts, rows, flag};
    hipLaunchKernelGGL((bin_count_kernel<MAXB, RatioRule>), dim3((unsigned)n_pairs), dim3(NT), 0, st, A);
    int rc = iamx::check_launch("iamx_ratio_bins");
    if (rc != IAMX_OK) return rc;
    rc = iamx_exclusive_scan_i32(seg_cnt, (int64_t)n_pairs * n_bins, seg_off, stream);
    if (rc != IAMX_OK) return rc;
    hipLaunchKernelGGL((bin_fill_kernel<MAXB, RatioRule>), dim3((unsigned)n_pairs), dim3(NT), 0, st, A);
    return iamx::check_launch("iamx_ratio_bins");
}

extern "C" int iamx_ratio_select(const int32_t *pairs, const int64_t *kp_off, const int32_t *key2,
                                 int n_pairs, int n_bins, double min_pairs, int min_unique,
                                 const int32_t *bin_cnt, const int32_t *seg_cnt,
                                 const int64_t *seg_off, const int32_t *rows, const uint8_t *mask,
                                 const int32_t *vstatus, int64_t cap, int stride, int tab_size,
                                 int32_t *work, int32_t *out_slots, int32_t *out_cnt,
                                 int64_t *out_off, int32_t *out_rows, int64_t out_cap,
                                 int32_t *chosen, int32_t *stats, int32_t *flag, void *stream)
{
    IAMX_REQUIRE(pairs && kp_off && key2 && bin_cnt && seg_cnt && seg_off && rows && mask && vstatus &&
                     work && out_slots && out_cnt && out_off && out_rows && chosen && stats && flag,
                 "null pointer");
    IAMX_REQUIRE(n_pairs >= 0 && cap >= 0 && out_cap >= 0 && min_unique >= 0, "negative count");
    IAMX_REQUIRE(n_bins >= 1 && n_bins <= MAXB, "n_bins outside 1..8");
    IAMX_REQUIRE_WORK_SLICE(stride, tab_size);
    if (n_pairs) {
        SelArgs A{pairs, kp_off, key2, n_bins, min_pairs, min_unique,
                  {bin_cnt, seg_cnt, seg_off, rows, mask, vstatus, cap, stride},
                  tab_size, work, out_slots, out_cnt, chosen, stats, flag};
        hipLaunchKernelGGL(ratio_select_kernel, dim3((unsigned)n_pairs), dim3(NT), 0,
                           iamx::as_stream(stream), A);
        const int rc = iamx::check_launch("iamx_ratio_select");
        if (rc != IAMX_OK) return rc;
    }
    return scan_and_pack("iamx_ratio_select", n_pairs, out_cnt, out_off, out_slots, stride, out_rows,
                         out_cap, stream);
}
