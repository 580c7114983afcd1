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
#include "key_dedupe.h"

namespace {

using namespace iamx_kd;          // NT = 256, compact(), dedupe(), block_sum()
constexpr int MAXB = 8;
constexpr int MAX_ROWS = 1 << 24;

struct Cut { double c[MAXB]; };

typedef int v2i __attribute__((ext_vector_type(2)));

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

// is a bin of `len` members looked at?  (matcher.py:634, and the four points a homography needs)
__device__ __forceinline__ bool gate(int len, double min_pairs)
{
    return (double)len >= min_pairs && len >= 4;
}

__global__ __launch_bounds__(NT) void ratio_count_kernel(const int32_t *__restrict__ d2,
                                                         const int64_t *__restrict__ row_off, int nb,
                                                         Cut C, double min_pairs,
                                                         int32_t *__restrict__ bin_cnt,
                                                         int32_t *__restrict__ seg_cnt,
                                                         int32_t *__restrict__ flag)
{
    __shared__ int wsum[NT / 64][MAXB];
    const int p = blockIdx.x;
    const int64_t b0 = row_off[p];
    const int64_t n64 = row_off[p + 1] - b0;
    const int n = n64 < 0 || n64 > MAX_ROWS ? 0 : (int)n64;
    int cnt[MAXB], zd = 0;
#pragma unroll
    for (int b = 0; b < MAXB; ++b) cnt[b] = 0;
    for (int i = threadIdx.x; i < n; i += NT) {
        bool zero;
        const unsigned m = bin_mask(*reinterpret_cast<const v2i *>(d2 + 2 * (b0 + i)), C, nb, zero);
        zd += zero ? 1 : 0;
#pragma unroll
        for (int b = 0; b < MAXB; ++b) cnt[b] += (m >> b) & 1;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        zd += __shfl_xor(zd, s);
#pragma unroll
        for (int b = 0; b < MAXB; ++b) cnt[b] += __shfl_xor(cnt[b], s);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int b = 0; b < MAXB; ++b) wsum[threadIdx.x >> 6][b] = cnt[b];
        if (zd) atomicAdd(flag, zd);
    }
    if (threadIdx.x == 0 && n64 != (int64_t)n) atomicAdd(flag + 1, 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        // a bin with as many members as the last bin that was looked at IS that bin (the bins are
        // nested): its consensus would be the same and cannot win under `>`, so it gets no segment
        int prev = -1;
        for (int b = 0; b < nb; ++b) {
            const int c = wsum[0][b] + wsum[1][b] + wsum[2][b] + wsum[3][b];
            bin_cnt[p * nb + b] = c;
            const bool g = gate(c, min_pairs);
            seg_cnt[p * nb + b] = g && c != prev ? c : 0;
            if (g) prev = c;
        }
    }
}

__global__ __launch_bounds__(NT) void ratio_fill_kernel(
    const int32_t *__restrict__ idx, const int32_t *__restrict__ d2,
    const int64_t *__restrict__ row_off, const int32_t *__restrict__ pairs,
    const int64_t *__restrict__ kp_off, const float *__restrict__ xy, int nb, Cut C,
    const int32_t *__restrict__ seg_cnt, const int64_t *__restrict__ seg_off, int64_t cap,
    float *__restrict__ pts, int32_t *__restrict__ rows)
{
    __shared__ int wcnt[NT / 64][MAXB];
    const int p = blockIdx.x;
    const int64_t b0 = row_off[p];
    const int64_t n64 = row_off[p + 1] - b0;
    const int n = n64 < 0 || n64 > MAX_ROWS ? 0 : (int)n64;
    unsigned on = 0;
    int base[MAXB];
    int64_t first[MAXB];
#pragma unroll
    for (int b = 0; b < MAXB; ++b) {
        base[b] = 0;
        first[b] = 0;
        if (b < nb && seg_cnt[p * nb + b] > 0) {
            on |= 1u << b;
            first[b] = seg_off[p * nb + b];
        }
    }
    if (!on) return;
    const float *xq = xy + 2 * kp_off[pairs[2 * p]], *xt = xy + 2 * kp_off[pairs[2 * p + 1]];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int s = 0; s < n; s += NT) {
        const int i = s + threadIdx.x;
        unsigned m = 0;
        if (i < n) {
            bool zero;
            m = bin_mask(*reinterpret_cast<const v2i *>(d2 + 2 * (b0 + i)), C, nb, zero) & on;
        }
        int pre[MAXB];
#pragma unroll
        for (int b = 0; b < MAXB; ++b) {
            const unsigned long long bal = __ballot((m >> b) & 1);
            pre[b] = __popcll(bal & ((1ull << lane) - 1));
            if (lane == 0) wcnt[wave][b] = __popcll(bal);
        }
        __syncthreads();
        if (m) {
            const int t = idx[2 * (b0 + i)];
            const float x1 = xq[2 * i], y1 = xq[2 * i + 1], x2 = xt[2 * t], y2 = xt[2 * t + 1];
#pragma unroll
            for (int b = 0; b < MAXB; ++b) {
                if (!((m >> b) & 1)) continue;
                int pos = base[b] + pre[b];
                for (int w = 0; w < wave; ++w) pos += wcnt[w][b];
                const int64_t o = first[b] + pos;
                if (o < 0 || o >= cap) continue;          // (never: cap >= n_bins * rows)
                *reinterpret_cast<float4 *>(pts + 4 * o) = make_float4(x1, y1, x2, y2);
                *reinterpret_cast<v2i *>(rows + 2 * o) = v2i{i, t};
            }
        }
#pragma unroll
        for (int b = 0; b < MAXB; ++b) base[b] += wcnt[0][b] + wcnt[1][b] + wcnt[2][b] + wcnt[3][b];
        __syncthreads();
    }
}

struct SelArgs {
    const int32_t *pairs;              // [n_pairs][2] image slots (query, train)
    const int64_t *kp_off;             // [n_images] first keypoint of every image slot
    const int32_t *key2;               // [total kp][2] round-half-even(100 * kp.pt) ("%.2f")
    int nb;
    double min_pairs;
    int min_unique;                    // best_fitted_matches of matcher.py:603
    const int32_t *bin_cnt, *seg_cnt;  // [n_pairs][nb]
    const int64_t *seg_off;            // [n_pairs * nb + 1]
    const int32_t *rows;               // [cap][2] (query row, train row) of every bin entry
    const uint8_t *mask;               // [cap] iamx_verify_pairs
    const int32_t *vstatus;            // [n_pairs * nb]
    int64_t cap;
    int stride, tab_size;
    int32_t *work;                     // [n_pairs][6 * stride + 2 * tab_size]
    int32_t *out_slots;                // [n_pairs][stride][2]
    int32_t *out_cnt, *chosen, *stats; // [n_pairs], [n_pairs], [n_pairs][nb][3]
    int32_t *flag;
};

__global__ __launch_bounds__(NT) void ratio_select_kernel(SelArgs A)
{
    __shared__ int red[NT / 64];
    const int p = blockIdx.x, nb = A.nb;
    int32_t *w = A.work + (int64_t)p * (6 * (int64_t)A.stride + 2 * (int64_t)A.tab_size);
    int32_t *cand = w, *slotq = w + 2 * (int64_t)A.stride, *slott = slotq + A.stride,
            *cont = slott + A.stride, *keep = cont + A.stride, *tabq = keep + A.stride,
            *tabt = tabq + A.tab_size;
    int32_t *out = A.out_slots + (int64_t)p * A.stride * 2;
    int32_t *stat = A.stats + (int64_t)p * nb * 3;
    const int32_t *kq = A.key2 + 2 * A.kp_off[A.pairs[2 * p]], *kt = A.key2 + 2 * A.kp_off[A.pairs[2 * p + 1]];
    int best = A.min_unique, best_fit = 0, chosen = -1, prev_fit = -1, prev_uniq = -1;
    bool refused = false;
    for (int b = 0; b < nb; ++b) {
        const int seg = p * nb + b, len = A.bin_cnt[seg];
        int fit = -1, uniq = -1;
        if (gate(len, A.min_pairs)) {
            const int n = A.seg_cnt[seg];
            const int64_t o = A.seg_off[seg];
            if (n == 0) {                               // the same set as the bin before it
                fit = prev_fit;
                uniq = prev_uniq;
            } else if (n > A.stride || o < 0 || o + n > A.cap) {
                refused = true;                         // (never: the caller sizes stride and cap)
            } else {
                const uint8_t *mk = A.mask + o;
                const int32_t *rw = A.rows + 2 * o;
                // a bin without a model (IAMX_VERIFY_NO_MODEL) has no inliers
                fit = A.vstatus[seg] != IAMX_VERIFY_OK ? 0 :
                    compact(red, n, [&](int i) { return mk[i] != 0; },
                            [&](int pos, int i) { cand[2 * pos] = rw[2 * i]; cand[2 * pos + 1] = rw[2 * i + 1]; });
                uniq = dedupe(red, kq, kt, cand, fit, tabq, tabt, slotq, slott, cont, keep, A.tab_size);
                if (uniq > best) {                      // strictly more (matcher.py:647)
                    best = uniq;
                    best_fit = fit;
                    chosen = b;
                    compact(red, fit, [&](int i) { return keep[i] != 0; },
                            [&](int pos, int i) { out[2 * pos] = cand[2 * i]; out[2 * pos + 1] = cand[2 * i + 1]; });
                }
                prev_fit = fit;
                prev_uniq = uniq;
            }
        }
        if (threadIdx.x == 0) { stat[3 * b] = len; stat[3 * b + 1] = fit; stat[3 * b + 2] = uniq; }
    }
    if (threadIdx.x == 0) {
        // matcher.py:683-694: the fitted list, then the de-duplicated one, against min_pairs
        const bool ok = !refused && chosen >= 0 && (double)best_fit >= A.min_pairs && (double)best >= A.min_pairs;
        A.out_cnt[p] = ok ? best : 0;
        A.chosen[p] = refused ? -1 : chosen;
        if (refused) atomicAdd(A.flag + 1, 1);
    }
}

__global__ __launch_bounds__(NT) void ratio_pack_kernel(const int32_t *__restrict__ cnt,
                                                        const int64_t *__restrict__ off,
                                                        const int32_t *__restrict__ slots, int stride,
                                                        int64_t cap, int32_t *__restrict__ out_rows)
{
    const int p = blockIdx.x;
    const int c = cnt[p];
    const int64_t o = off[p];
    if (c <= 0 || c > stride || o < 0 || o + c > cap) return;
    const v2i *src = reinterpret_cast<const v2i *>(slots) + (int64_t)p * stride;
    v2i *dst = reinterpret_cast<v2i *>(out_rows) + o;
    for (int i = threadIdx.x; i < c; i += NT) dst[i] = src[i];
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
    hipLaunchKernelGGL(ratio_count_kernel, dim3((unsigned)n_pairs), dim3(NT), 0, st, d2, row_off,
                       n_bins, C, min_pairs, bin_cnt, seg_cnt, flag);
    int rc = iamx::check_launch("iamx_ratio_bins");
    if (rc != IAMX_OK) return rc;
    rc = iamx_exclusive_scan_i32(seg_cnt, (int64_t)n_pairs * n_bins, seg_off, stream);
    if (rc != IAMX_OK) return rc;
    hipLaunchKernelGGL(ratio_fill_kernel, dim3((unsigned)n_pairs), dim3(NT), 0, st, idx, d2, row_off,
                       pairs, kp_off, xy, n_bins, C, (const int32_t *)seg_cnt,
                       (const int64_t *)seg_off, cap, pts, rows);
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
    IAMX_REQUIRE(stride >= 1 && stride <= MAX_ROWS, "stride outside 1..2^24");
    IAMX_REQUIRE(tab_size >= 64 && (tab_size & (tab_size - 1)) == 0 && (int64_t)tab_size >= 2 * (int64_t)stride,
                 "tab_size must be a power of two >= max(64, 2 * stride)");
    hipStream_t st = iamx::as_stream(stream);
    if (n_pairs) {
        SelArgs A{pairs, kp_off, key2, n_bins, min_pairs, min_unique, bin_cnt, seg_cnt, seg_off, rows,
                  mask, vstatus, cap, stride, tab_size, work, out_slots, out_cnt, chosen, stats, flag};
        hipLaunchKernelGGL(ratio_select_kernel, dim3((unsigned)n_pairs), dim3(NT), 0, st, A);
        const int rc = iamx::check_launch("iamx_ratio_select");
        if (rc != IAMX_OK) return rc;
    }
    const int rc = iamx_exclusive_scan_i32(out_cnt, n_pairs, out_off, stream);
    if (rc != IAMX_OK) return rc;
    if (n_pairs)
        hipLaunchKernelGGL(ratio_pack_kernel, dim3((unsigned)n_pairs), dim3(NT), 0, st,
                           (const int32_t *)out_cnt, (const int64_t *)out_off,
                           (const int32_t *)out_slots, stride, out_cap, out_rows);
    return iamx::check_launch("iamx_ratio_select");
}
