// What the 'bestratio', 'smart' and 'bruteforce' strategies share around their row rules
// (match_ratio.hip, match_smart.hip, match_brute.hip): the gate of a bin, a pair's slice of the
// select stage's scratch and the check of its sizes, the count and fill kernels of nested bins as
// templates over a row rule, the walk over nested bins, a segment's inliers taken as a
// de-duplicated list, and the scan and packing of the results.  One workgroup of NT threads per pair.
//
// Like key_dedupe.h this header holds no floating-point arithmetic beyond gate()'s comparison, so it
// compiles the same under -ffp-contract=off and under the `#pragma clang fp contract(off)` that
// follows the includes of a source; arithmetic that is ever added here needs a pragma of its own.
#pragma once
#include "iamx_common.h"
#include "key_dedupe.h"

namespace iamx_bs {
namespace {

using namespace iamx_kd;          // NT = 256, compact(), dedupe()
constexpr int MAX_ROWS = 1 << 24;          // rows of a query image, and so entries of a list

typedef int v2i __attribute__((ext_vector_type(2)));

// is a bin of `len` members looked at?  (the strategy's min_pairs, and the four points a homography needs)
__device__ __forceinline__ bool gate(int len, double min_pairs)
{
    return (double)len >= min_pairs && len >= 4;
}

// a pair's slice of `work` [n_pairs][6 * stride + 2 * tab_size]: the candidate list, dedupe()'s lists
// and its two key tables
struct WorkSlice {
    int32_t *cand, *slotq, *slott, *cont, *keep, *tabq, *tabt;
    int tab_size;
    __device__ __forceinline__ WorkSlice(int32_t *work, int p, int stride, int tab_size_)
    {
        cand = work + (int64_t)p * (6 * (int64_t)stride + 2 * (int64_t)tab_size_);
        slotq = cand + 2 * (int64_t)stride;
        slott = slotq + stride;
        cont = slott + stride;
        keep = cont + stride;
        tabq = keep + stride;
        tabt = tabq + tab_size_;
        tab_size = tab_size_;
    }
};

// the sizes WorkSlice is carved with, checked in the entry that takes them
#define IAMX_REQUIRE_WORK_SLICE(stride, tab_size)                                                      \
    do {                                                                                               \
        IAMX_REQUIRE((stride) >= 1 && (stride) <= iamx_bs::MAX_ROWS, "stride outside 1..2^24");        \
        IAMX_REQUIRE((tab_size) >= 64 && ((tab_size) & ((tab_size) - 1)) == 0 &&                       \
                         (int64_t)(tab_size) >= 2 * (int64_t)(stride),                                 \
                     "tab_size must be a power of two >= max(64, 2 * stride)");                        \
    } while (0)

// the "%.2f" keys of a pair's two images
struct PairKeys {
    const int32_t *q, *t;
    __device__ __forceinline__ PairKeys(const int32_t *key2, const int64_t *kp_off, const int32_t *pairs, int p)
        : q(key2 + 2 * kp_off[pairs[2 * p]]), t(key2 + 2 * kp_off[pairs[2 * p + 1]]) {}
};

// ---------------------------------------------------------------------------------
// nested bins: members per bin, then every looked-at bin as one segment of points
// ---------------------------------------------------------------------------------
// A row rule R is built per pair from the entry's argument struct R::Args (which holds min_pairs, cap,
// bin_cnt, seg_cnt, seg_off, pts, rows, flag beside the rule's own) and gives
//   R::n_bins(A)           the bins of the launch, at most MAXB
//   R(A, p)                the pair: n rows (0 for a pair that is not live), oversize
//   bins(i, zero, t)       the bins query row i is in (bit b), whether its distance is zero, and
//                          whatever of its train row the rule learns on the way
//   point(i, t)            for a row in a looked-at bin: x1 y1 x2 y2, t made the train row
template <int MAXB, typename R>
__global__ __launch_bounds__(NT) void bin_count_kernel(typename R::Args A)
{
    __shared__ int wsum[NT / 64][MAXB];
    const int p = blockIdx.x, nb = R::n_bins(A);
    const R rule(A, p);
    int cnt[MAXB], zd = 0;
#pragma unroll
    for (int b = 0; b < MAXB; ++b) cnt[b] = 0;
    for (int i = threadIdx.x; i < rule.n; i += NT) {
        bool zero;
        int t;
        const unsigned m = rule.bins(i, zero, t);
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
        if (zd) atomicAdd(A.flag, zd);
    }
    if (threadIdx.x == 0 && rule.oversize) atomicAdd(A.flag + 1, 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        // a bin with as many members as the last bin that was looked at IS that bin (the bins are
        // nested): its consensus would be the same and cannot win under `>`, so it gets no segment
        int prev = -1;
        for (int b = 0; b < nb; ++b) {
            const int c = wsum[0][b] + wsum[1][b] + wsum[2][b] + wsum[3][b];
            A.bin_cnt[p * nb + b] = c;
            const bool g = gate(c, A.min_pairs);
            A.seg_cnt[p * nb + b] = g && c != prev ? c : 0;
            if (g) prev = c;
        }
    }
}

template <int MAXB, typename R>
__global__ __launch_bounds__(NT) void bin_fill_kernel(typename R::Args A)
{
    __shared__ int wcnt[NT / 64][MAXB];
    const int p = blockIdx.x, nb = R::n_bins(A);
    unsigned on = 0;
    int base[MAXB];
    int64_t first[MAXB];
#pragma unroll
    for (int b = 0; b < MAXB; ++b) {
        base[b] = 0;
        first[b] = 0;
        if (b < nb && A.seg_cnt[p * nb + b] > 0) {
            on |= 1u << b;
            first[b] = A.seg_off[p * nb + b];
        }
    }
    if (!on) return;
    const R rule(A, p);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int s = 0; s < rule.n; s += NT) {
        const int i = s + threadIdx.x;
        unsigned m = 0;
        int t = -1;
        if (i < rule.n) {
            bool zero;
            m = rule.bins(i, zero, t) & on;
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
            const float4 pt = rule.point(i, t);
#pragma unroll
            for (int b = 0; b < MAXB; ++b) {
                if (!((m >> b) & 1)) continue;
                int pos = base[b] + pre[b];
                for (int w = 0; w < wave; ++w) pos += wcnt[w][b];
                const int64_t o = first[b] + pos;
                if (o < 0 || o >= A.cap) continue;          // (never: cap >= n_bins * rows)
                *reinterpret_cast<float4 *>(A.pts + 4 * o) = pt;
                *reinterpret_cast<v2i *>(A.rows + 2 * o) = v2i{i, t};
            }
        }
#pragma unroll
        for (int b = 0; b < MAXB; ++b) base[b] += wcnt[0][b] + wcnt[1][b] + wcnt[2][b] + wcnt[3][b];
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------
// the select stage
// ---------------------------------------------------------------------------------
// A segment's inliers as a list: mk[i] != 0 of its n entries rw -> W.cand (none where mk is null),
// filter_duplicates over them, and where take(unique) the kept ones -> out.  -> (inliers, unique),
// the same in every thread; take() must be too.
template <typename T>
__device__ __forceinline__ v2i take_list(int *red, const uint8_t *mk, const int32_t *rw, int n,
                                         const PairKeys &K, const WorkSlice &W, int32_t *out, T take)
{
    int32_t *cand = W.cand, *keep = W.keep;
    const int fit = !mk ? 0 :
        compact(red, n, [&](int i) { return mk[i] != 0; },
                [&](int pos, int i) { cand[2 * pos] = rw[2 * i]; cand[2 * pos + 1] = rw[2 * i + 1]; });
    const int uniq = dedupe(red, K.q, K.t, cand, fit, W.tabq, W.tabt, W.slotq, W.slott, W.cont, keep, W.tab_size);
    if (take(uniq))
        compact(red, fit, [&](int i) { return keep[i] != 0; },
                [&](int pos, int i) { out[2 * pos] = cand[2 * i]; out[2 * pos + 1] = cand[2 * i + 1]; });
    return v2i{fit, uniq};
}

// the segments of a launch and their consensus (iamx_verify_pairs), as the select entries take them
struct Segments {
    const int32_t *bin_cnt, *seg_cnt;  // [n_pairs][nb] (bin_cnt: the nested-bin walk only)
    const int64_t *seg_off;            // [n_pairs * nb + 1]
    const int32_t *rows;               // [cap][2] (query row, train row) of every segment entry
    const uint8_t *mask;               // [cap]
    const int32_t *vstatus;            // [n_pairs * nb]
    int64_t cap;
    int stride;
};

struct Walked {
    int best, best_fit;                // unique and fitted of the pair's list
    int taken;                         // 1 + the last bin that raised best; 0: none
    bool refused;                      // a segment the buffers cannot hold (never: the caller sizes them)
};

// The walk over pair p's nb nested bins, narrowest first: a bin with strictly more unique inliers than
// best becomes the pair's list in `out`; stat[b] = members, fit, unique (-1, -1: not looked at).
__device__ __forceinline__ Walked walk_bins(int *red, const Segments &S, int p, int nb, double min_pairs,
                                            const PairKeys &K, const WorkSlice &W, int32_t *out,
                                            int32_t *stat, int best, int best_fit)
{
    Walked r{best, best_fit, 0, false};
    int prev_fit = -1, prev_uniq = -1;
    for (int b = 0; b < nb; ++b) {
        const int seg = p * nb + b, len = S.bin_cnt[seg];
        int fit = -1, uniq = -1;
        if (gate(len, min_pairs)) {
            const int n = S.seg_cnt[seg];
            const int64_t o = S.seg_off[seg];
            if (n == 0) {                               // the same set as the bin before it
                fit = prev_fit;
                uniq = prev_uniq;
            } else if (n > S.stride || o < 0 || o + n > S.cap) {
                r.refused = true;
            } else {
                // a bin without a model (IAMX_VERIFY_NO_MODEL) has no inliers
                const v2i fu = take_list(red, S.vstatus[seg] != IAMX_VERIFY_OK ? nullptr : S.mask + o,
                                         S.rows + 2 * o, n, K, W, out, [&](int u) { return u > r.best; });
                fit = fu.x;
                uniq = fu.y;
                if (uniq > r.best) {                    // strictly more
                    r.best = uniq;
                    r.best_fit = fit;
                    r.taken = b + 1;
                }
                prev_fit = fit;
                prev_uniq = uniq;
            }
        }
        if (threadIdx.x == 0) { stat[3 * b] = len; stat[3 * b + 1] = fit; stat[3 * b + 2] = uniq; }
    }
    return r;
}

// the lists of the pairs' fixed slots back to back
__global__ __launch_bounds__(NT) void pack_kernel(const int32_t *__restrict__ cnt,
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

// the tail of every select entry: out_off = exclusive scan of out_cnt (written at n_pairs == 0 too),
// then the packing
inline int scan_and_pack(const char *entry, int n_pairs, int32_t *out_cnt, int64_t *out_off,
                         const int32_t *out_slots, int stride, int32_t *out_rows, int64_t out_cap,
                         void *stream)
{
    const int rc = iamx_exclusive_scan_i32(out_cnt, n_pairs, out_off, stream);
    if (rc != IAMX_OK) return rc;
    if (n_pairs)
        hipLaunchKernelGGL(pack_kernel, dim3((unsigned)n_pairs), dim3(NT), 0, iamx::as_stream(stream),
                           (const int32_t *)out_cnt, (const int64_t *)out_off, out_slots, stride, out_cap,
                           out_rows);
    return iamx::check_launch(entry);
}

}  // namespace
}  // namespace iamx_bs
