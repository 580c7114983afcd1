// K3 -- exact 3-NN descriptor matching for gfx950 (MI355X).
//
// The search of the reference's 'smart' strategy: the_matcher.knnMatch(des1, des2, k=3)
// (scripts/lib/matcher.py:456-470), whose per-row walk looks at up to three neighbours.
//
// Arithmetic, mapping, staging and the packed key are those of the top-2 kernel (match_knn2.hip):
// i8 MFMA 32x32x32 with the queries on the columns, so that one lane sees ONE query against 16
// train rows per tile, and
//     key = (acc << 9) + ((norm_t << 8) | (row & 255))
// orders by (distance, train row) inside an epoch of 256 train rows.  The running top-3 of a lane is
// three sorted keys and costs 4 VALU ops per distance (one more than the top-2):
//     m3 = med3(m2, m3, key) ; m2 = med3(m1, m2, key) ; m1 = min(m1, key)
// Every 256 train rows the keys are folded into full (distance, index) triples: a later epoch holds
// higher rows only, so an equal distance never displaces an entry that is already there.  The two
// lane halves (rows +4) hold disjoint rows of the same epochs and are merged at the end by
// (distance, row).  A train image of fewer than 3 rows leaves idx = -1, d2 = 0x7FFFFFFF.
#include "iamx_common.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int D = IAMX_DESC_DIM;        // 128 bytes per row
constexpr int QW = 2;                   // 32-query blocks per wave
constexpr int WAVES = 4;
constexpr int NT = WAVES * 64;          // threads
constexpr int QB = WAVES * QW * 32;     // 256 query rows per workgroup (iamx_knn2_wg_per_pair)
constexpr int CHUNK = 128;              // train rows staged per step (= IAMX_ROW_PAD)
constexpr int PIECES = CHUNK * D / 16 / NT;
constexpr int KEY_INVALID = 0x7FFFFFFF;
constexpr int D_NONE = KEY_INVALID >> 8;   // above every partial distance (<= 128 * 255^2)
static_assert(CHUNK == IAMX_ROW_PAD, "a chunk never reads past an image's padded rows");

struct Knn3Args {
    const int8_t *desc;
    const int32_t *norm_q;
    const int32_t *norm_t;
    const int32_t *img_off;
    const int32_t *img_n;
    const int32_t *pairs;
    const int32_t *wg_off;
    const int64_t *out_off;
    int32_t *out_idx;
    int32_t *out_d2;
    int n_pairs;
    int total_wg;
};

__device__ __forceinline__ int med3_i32(int a, int b, int c)
{
    // inline asm as in match_knn2.hip: its `c` operand is always the compiler-generated key (a VALU
    // result), never a raw MFMA accumulator
    int r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

struct Top3 {
    int d[3], i[3];
};

// (d, i) into the sorted triple.  LEX: equal distances go to the lower row; otherwise an equal
// distance stays behind what is there (the caller knows its row is the higher one).
template <bool LEX>
__device__ __forceinline__ void insert3(Top3 &b, int d, int i)
{
    auto less = [](int da, int ia, int db, int ib) {
        return da < db || (LEX && da == db && ia < ib);
    };
    const bool l0 = less(d, i, b.d[0], b.i[0]);
    const bool l1 = less(d, i, b.d[1], b.i[1]);
    const bool l2 = less(d, i, b.d[2], b.i[2]);
    b.d[2] = l1 ? b.d[1] : (l2 ? d : b.d[2]);
    b.i[2] = l1 ? b.i[1] : (l2 ? i : b.i[2]);
    b.d[1] = l0 ? b.d[0] : (l1 ? d : b.d[1]);
    b.i[1] = l0 ? b.i[0] : (l1 ? i : b.i[1]);
    b.d[0] = l0 ? d : b.d[0];
    b.i[0] = l0 ? i : b.i[0];
}

__global__ __launch_bounds__(NT, 2) void knn3_pairs_kernel(Knn3Args A)
{
    __shared__ __attribute__((aligned(16))) int8_t lds[2 * CHUNK * D + 2 * CHUNK * 4];
    int8_t *lds_tile = lds;                                      // [2][CHUNK][128]
    int *lds_tb = reinterpret_cast<int *>(lds + 2 * CHUNK * D);  // [2][CHUNK]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int c = lane & 31;     // query column inside a 32-block / train row inside a tile
    const int g = lane >> 5;     // k-half for operands, +4 row offset for results

    // XCD-aware block -> work id: each XCD gets a contiguous run (the workgroups of a pair share an L2)
    int vid;
    {
        const int total = A.total_wg;
        const int bid = blockIdx.x;
        const int xcd = bid & 7, k = bid >> 3;
        const int q = total >> 3, r = total & 7;
        vid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
    }
    // pair = largest p with wg_off[p] <= vid
    int lo = 0, hi = A.n_pairs;
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (A.wg_off[mid] <= vid) lo = mid; else hi = mid;
    }
    const int qimg = A.pairs[2 * lo], timg = A.pairs[2 * lo + 1];
    const int qoff = A.img_off[qimg], nq = A.img_n[qimg];
    const int toff = A.img_off[timg], nt = A.img_n[timg];
    const int64_t obase = A.out_off[lo];
    const int q0 = (vid - A.wg_off[lo]) * QB + wave * (QW * 32);

    if (nt <= 0) {               // no train row to stage: every neighbour is missing
        for (int r = tid; r < QB; r += NT) {
            const int row = (vid - A.wg_off[lo]) * QB + r;
            if (row < nq)
                for (int k = 0; k < 3; ++k) {
                    A.out_idx[3 * (obase + row) + k] = -1;
                    A.out_d2[3 * (obase + row) + k] = KEY_INVALID;
                }
        }
        return;
    }

    // query fragments: B operand, lane (c,g) holds bytes [32s+16g, +16) of row c
    v4i bq[QW][4];
#pragma unroll
    for (int qb = 0; qb < QW; ++qb) {
        int row = q0 + qb * 32 + c;
        row = row < nq ? row : nq - 1;
        const v4i *src = reinterpret_cast<const v4i *>(A.desc + (int64_t)(qoff + row) * D);
#pragma unroll
        for (int s = 0; s < 4; ++s) bq[qb][s] = ~src[2 * s + g];
    }

    int m1[QW], m2[QW], m3[QW];
    Top3 best[QW];
#pragma unroll
    for (int qb = 0; qb < QW; ++qb) {
        m1[qb] = m2[qb] = m3[qb] = KEY_INVALID;
#pragma unroll
        for (int k = 0; k < 3; ++k) { best[qb].d[k] = D_NONE; best[qb].i[k] = -1; }
    }

    // staging: thread loads PIECES x 16 B of the 16 KiB chunk + (tid < 128) one key term
    const int8_t *tbase = A.desc + (int64_t)toff * D;
    const int32_t *tnorm = A.norm_t + toff;
    v4i st[PIECES];
    int st_tb = KEY_INVALID;
    auto load_chunk = [&](int ch) {
#pragma unroll
        for (int j = 0; j < PIECES; ++j) {
            int e = j * NT + tid;
            st[j] = *reinterpret_cast<const v4i *>(tbase + (int64_t)(ch * CHUNK) * D + e * 16);
        }
        if (tid < CHUNK) {
            int rr = ch * CHUNK + tid;
            st_tb = rr < nt ? tnorm[rr] * 256 + (rr & 255) : KEY_INVALID;
        }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int j = 0; j < PIECES; ++j) {
            int e = j * NT + tid;
            int row = e >> 3, slot = e & 7;
            int phys = slot ^ ((row >> 1) & 7);
            *reinterpret_cast<v4i *>(lds_tile + buf * (CHUNK * D) + row * D + phys * 16) = st[j];
        }
        if (tid < CHUNK) lds_tb[buf * CHUNK + tid] = st_tb;
    };

    const int nchunks = (nt + CHUNK - 1) / CHUNK;
    load_chunk(0);
    store_chunk(0);
    __syncthreads();

    for (int ch = 0; ch < nchunks; ++ch) {
        const int buf = ch & 1;
        if (ch + 1 < nchunks) load_chunk(ch + 1);

        const int8_t *tile_base = lds_tile + buf * (CHUNK * D);
        const int *tb_base = lds_tb + buf * CHUNK;
#pragma unroll
        for (int tile = 0; tile < CHUNK / 32; ++tile) {
            const int r = tile * 32 + c;
            const int swz = (r >> 1) & 7;
            v4i a[4];
#pragma unroll
            for (int s = 0; s < 4; ++s)
                a[s] = *reinterpret_cast<const v4i *>(tile_base + r * D + (((2 * s + g) ^ swz) * 16));
            v4i tbv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                tbv[k] = *reinterpret_cast<const v4i *>(tb_base + tile * 32 + 8 * k + 4 * g);
#pragma unroll
            for (int qb = 0; qb < QW; ++qb) {
                v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], bq[qb][s], acc, 0, 0, 0);
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    // (a padded row holds zeros: acc == 0 there and the key stays KEY_INVALID)
                    int key = tbv[reg >> 2][reg & 3] + (acc[reg] << 9);
                    m3[qb] = med3_i32(m2[qb], m3[qb], key);
                    m2[qb] = med3_i32(m1[qb], m2[qb], key);
                    m1[qb] = min(m1[qb], key);
                }
            }
        }

        // fold the packed keys of this 256-row epoch into (distance, index) triples
        if ((ch & 1) || ch == nchunks - 1) {
            const int sbase = (ch >> 1) * 256;
#pragma unroll
            for (int qb = 0; qb < QW; ++qb) {
                Top3 &b = best[qb];
                const int k1 = m1[qb], k2 = m2[qb], k3 = m3[qb];
                // ascending keys: once one does not enter, none behind it does (D_NONE never enters)
                if ((k1 >> 8) < b.d[2]) {
                    insert3<false>(b, k1 >> 8, sbase + (k1 & 255));
                    if ((k2 >> 8) < b.d[2]) {
                        insert3<false>(b, k2 >> 8, sbase + (k2 & 255));
                        if ((k3 >> 8) < b.d[2]) insert3<false>(b, k3 >> 8, sbase + (k3 & 255));
                    }
                }
                m1[qb] = m2[qb] = m3[qb] = KEY_INVALID;
            }
        }

        if (ch + 1 < nchunks) store_chunk(buf ^ 1);
        __syncthreads();
    }

    // merge the two lane halves, add the query norm, store
#pragma unroll
    for (int qb = 0; qb < QW; ++qb) {
        Top3 a = best[qb];
        int od[3], oi[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            od[k] = __shfl_xor(a.d[k], 32);
            oi[k] = __shfl_xor(a.i[k], 32);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (od[k] != D_NONE) insert3<true>(a, od[k], oi[k]);
        const int row = q0 + qb * 32 + c;
        if (g == 0 && row < nq) {
            const int na = A.norm_q[qoff + row];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const bool some = a.d[k] != D_NONE;
                A.out_idx[3 * (obase + row) + k] = some ? a.i[k] : -1;
                A.out_d2[3 * (obase + row) + k] = some ? a.d[k] + na : KEY_INVALID;
            }
        }
    }
}

}  // namespace

extern "C" int iamx_knn3_l2_pairs(const int8_t *desc, const int32_t *norm_q,
                                  const int32_t *norm_t, const int32_t *img_off,
                                  const int32_t *img_n, const int32_t *pairs,
                                  const int32_t *wg_off, const int64_t *out_off, int n_pairs,
                                  int total_wg, int32_t *out_idx, int32_t *out_d2, void *stream)
{
    IAMX_REQUIRE(desc && norm_q && norm_t && img_off && img_n && pairs && wg_off && out_off &&
                     out_idx && out_d2,
                 "null pointer");
    IAMX_REQUIRE(n_pairs >= 0 && total_wg >= 0, "negative count");
    if (n_pairs == 0 || total_wg == 0) return IAMX_OK;
    Knn3Args a{desc, norm_q, norm_t, img_off, img_n, pairs, wg_off, out_off,
               out_idx, out_d2, n_pairs, total_wg};
    hipLaunchKernelGGL(knn3_pairs_kernel, dim3((unsigned)total_wg), dim3(NT), 0,
                       iamx::as_stream(stream), a);
    return iamx::check_launch("iamx_knn3_l2_pairs");
}
