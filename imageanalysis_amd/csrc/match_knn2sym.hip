// K2 (symmetric form) -- ONE i8-MFMA sweep of a distance matrix serves BOTH directions of an
// image pair (gfx950).  Replaces the two knnMatch calls of bidirectional_pair_matches
// (scripts/lib/matcher.py:304-347 -> :203-216) and the metric loop (:253-263).
//
// Why: the one-direction fast form (match_knn2v2.hip) runs the MFMA pipe at ~80 % of its
// power-limited rate, but every distance matrix is executed twice (queries = image i against
// train = image j, then j against i).  The only factor left is that 2x.
//
// How: the sweep does not try to be exact.  For every row of BOTH images it only produces
//     L  <= exact best squared distance,      U  >= exact second squared distance
// cheaply enough to stay MFMA bound; the reference's test  d0*(d0/d1) < 270*ratio  is monotone
// (increasing in d0, decreasing in d1), so thresholding (L, U) keeps a SUPERSET of the rows the
// reference keeps (a few rows per image pair), and symexact_kernel recomputes those rows
// exactly (all train rows, v_dot4, lowest train row wins ties = cv2.BFMatcher order).  What
// leaves the path is bit-identical to the exact forms (tests/test_match_sym_gpu.py).
//
// Arithmetic.  s = value-128 (int8), n2 = |s|^2, nb = n2 + 2*sum(s), Ct = nb>>1, Cq = n2>>1,
// p = n2&1 (= nb&1).  With the B operand holding ~s_a = -s_a-1 and the C operand Ct[t]:
//     acc_out(a,t) = Ct[t] + sum(~s_a * s_t)         d2(a,t) = 2*(acc_out + Cq[a]) + p[a] + p[t]
// Column direction (queries = B rows, lane local): v = min_t acc_out, kept as 4 interleaved
//   running minima per lane (tile & 3) x 2 lane halves = 8 groups of train rows:
//   best >= 2*(v1+Cq[a]) + p[a],  second <= 2*(v2+Cq[a]) + p[a] + 1   (v2 = 2nd smallest group
//   minimum; 8 v_min3 per 16 distances = 0.5 VALU / distance).
// Row direction (queries = A rows, across lanes): R_w(t) = min over the 128 B rows of a wave of
//   acc_out: v_min3 across the wave's four 32-row blocks (0.5 VALU / distance), then a
//   TRANSPOSING butterfly over the 32 lanes (DPP quad_perm with bank masks, row_ror,
//   v_permlane16_swap: 36 instructions for 16 registers instead of 80).  The B rows of an image
//   are stored SORTED by n2, so Cq of a wave's rows lies in a narrow [lo_w, hi_w]:
//   group minimum in [R_w + lo_w, R_w + hi_w]; per train row the 8 waves of a workgroup are
//   merged through LDS into (L, U1, U2) = (min lower bound, two smallest upper bounds).
// One sorted store serves both roles (any order is legal for the A side).
//
// Workgroup shapes (iamx_knn2sym_sweep `form`).  Form 2, images of >= 4096 rows: 1024 B rows per
// workgroup as 4 waves x 8 query blocks, ONE wave per SIMD (WPE = 1, 512 registers: the B operand
// in the AGPR half, accumulators in VGPRs -- the file is compiled with -mllvm
// -amdgpu-mfma-vgpr-form) -- the butterfly and the LDS operand reads of a tile serve 32 MFMAs,
// 5.2 VALU per MFMA (round 3; before: 8 waves x 4 blocks at two waves per SIMD, 6.4 per MFMA).
// Forms 1 / 0 (512 / 256 rows per workgroup): 4 waves x 4 / 2 blocks, two waves per SIMD.
#include "iamx_common.h"
#include "sym_cand_rule.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));

#ifndef IAMX_DESC_OFFSET
#define IAMX_DESC_OFFSET 128
#endif
constexpr int D = IAMX_DESC_DIM;
constexpr int CHUNK = 128;
constexpr int BIG = 0x3F000000;          // Ct of padding rows: loses every comparison

// ---------------------------------------------------------------------------------
// pack ("desc3"): rows of an image sorted by n2 (stable), padded to 128 rows
//   A  per row (8 threads): n2, nb                       -> scratch
//   B  per row: rank = #{r' : (n2', r') < (n2, r)}        -> scratch (O(n^2), LDS tiled)
//   C  per row (8 threads): convert + scatter, sn2 / sct / sperm / sinv
//   D  padding rows
// ---------------------------------------------------------------------------------
struct Pack3Args {
    const void *src;             // [rows][128] u8 or f32, images back to back
    const int64_t *src_off;      // DEV [n_img+1] first source row of each image, or NULL:
    int64_t single_n;            //   one image of single_n rows
    const int32_t *dst_off;      // DEV [n_img] first packed row of each image (NULL: 0)
    int8_t *dst;
    int32_t *sn2, *sct, *sperm, *sinv;
    int32_t *n2, *nb, *pos;      // scratch, one int per source row each
    int n_img;
};

template <typename SRC>
__device__ __forceinline__ int load_value(const SRC *p, int i)
{
    if constexpr (sizeof(SRC) == 1) {
        return (int)p[i];
    } else {
        int v = (int)rintf((float)p[i]);
        return v < 0 ? 0 : (v > 255 ? 255 : v);
    }
}

template <typename SRC>
__global__ __launch_bounds__(256) void pack3_rows_kernel(Pack3Args P, int64_t total_rows)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = t >> 3;
    const int part = (int)(t & 7);
    int s2 = 0, s1 = 0;
    if (row < total_rows) {
        const SRC *p = static_cast<const SRC *>(P.src) + row * D + part * 16;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int s = load_value(p, i) - IAMX_DESC_OFFSET;
            s2 += s * s;
            s1 += s;
        }
    }
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) {
        s2 += __shfl_xor(s2, m, 8);
        s1 += __shfl_xor(s1, m, 8);
    }
    if (row < total_rows && part == 0) {
        P.n2[row] = s2;
        P.nb[row] = s2 + 2 * s1;
    }
}

// rank of every row inside its image = rows with a smaller key (ties: the earlier row).
// FIRST by binning (round 6; one workgroup per image): the keys of an image spread over a few
// hundred thousand values, so 4096 equal-width bins between its smallest and its largest key hold a
// few dozen rows each -- histogram in LDS, exclusive scan, the rows of a bin listed (row, key) in the
// image's still unused sperm / sinv slices, and a row's rank = start of its bin + the rows of its bin
// that come before it: n x (rows per bin) comparisons instead of n x n (51 ms per 256 frames of
// 37 k rows -> well under one).  An image whose fullest bin exceeds RANK_BIN_LIMIT rows (constant
// images, synthetic ties) is left to the counting kernel below: RANK_TODO at the head of its sct slice.
constexpr int RANK_BINS = 4096;
constexpr int RANK_BIN_LIMIT = 1024;
constexpr int RANK_TODO = 0x52414E4B;

__global__ __launch_bounds__(1024) void pack3_rank_bins_kernel(Pack3Args P)
{
    __shared__ int start[RANK_BINS + 1];
    __shared__ int cursor[RANK_BINS];
    __shared__ int wsum[16];
    __shared__ int s_lo, s_hi, s_max;
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = P.src_off ? P.src_off[img] : 0;
    const int n = (int)(P.src_off ? P.src_off[img + 1] - r0 : P.single_n);
    const int d0 = P.dst_off ? P.dst_off[img] : 0;
    if (n <= 0) return;
    const int32_t *key = P.n2 + r0;
    int32_t *list_row = P.sperm + d0, *list_key = P.sinv + d0;
    if (tid == 0) { s_lo = 0x7FFFFFFF; s_hi = -0x7FFFFFFF; s_max = 0; }
    for (int b = tid; b < RANK_BINS; b += 1024) cursor[b] = 0;
    __syncthreads();
    int lo = 0x7FFFFFFF, hi = -0x7FFFFFFF;
    for (int r = tid; r < n; r += 1024) {
        const int k = key[r];
        lo = min(lo, k);
        hi = max(hi, k);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        lo = min(lo, __shfl_xor(lo, m));
        hi = max(hi, __shfl_xor(hi, m));
    }
    if (lane == 0) { atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
    __syncthreads();
    lo = s_lo;
    int shift = 0;
    while (((int64_t)s_hi - lo) >> shift >= RANK_BINS) ++shift;
    for (int r = tid; r < n; r += 1024) atomicAdd(&cursor[(key[r] - lo) >> shift], 1);
    __syncthreads();
    // exclusive scan of the 4096 counts: 4 per thread, waves through shuffles, 16 wave sums through LDS
    int c[4], t = 0, mx = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        c[k] = cursor[4 * tid + k];
        t += c[k];
        mx = max(mx, c[k]);
    }
    int x = t;
#pragma unroll
    for (int sft = 1; sft < 64; sft <<= 1) {
        const int y = __shfl_up(x, sft);
        if (lane >= sft) x += y;
    }
    if (lane == 63) wsum[wave] = x;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mx = max(mx, __shfl_xor(mx, m));
    if (lane == 0) atomicMax(&s_max, mx);
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wave; ++w) woff += wsum[w];
    int run = woff + x - t;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        start[4 * tid + k] = run;
        run += c[k];
    }
    if (tid == 1023) start[RANK_BINS] = run;
    __syncthreads();
    if (s_max > RANK_BIN_LIMIT) {                        // (uniform: the counting kernel takes the image)
        if (tid == 0) P.sct[d0] = RANK_TODO;
        return;
    }
    if (tid == 0) P.sct[d0] = 0;
    for (int b = tid; b < RANK_BINS; b += 1024) cursor[b] = start[b];
    __syncthreads();
    for (int r = tid; r < n; r += 1024) {
        const int k = key[r];
        const int at = atomicAdd(&cursor[(k - lo) >> shift], 1);
        list_row[at] = r;
        list_key[at] = k;
    }
    __threadfence_block();
    __syncthreads();
    for (int r = tid; r < n; r += 1024) {
        const int k = key[r], b = (k - lo) >> shift;
        const int e = start[b + 1];
        int cnt = start[b];
        for (int i = start[b]; i < e; ++i) {
            const int kj = list_key[i], j = list_row[i];
            cnt += (kj < k) || (kj == k && j < r);
        }
        P.pos[r0 + r] = cnt;
    }
}

// The counting form (every image until round 6; now the images the binning kernel leaves).  blockIdx.z splits the comparisons of a 256-row group over `gridDim.z` workgroups
// (each adds its part to pos[], zeroed by the caller): one 38 k-row frame is 150 groups x 38 k
// compares -- 150 workgroups leave most of the chip idle (1.55 ms per frame, a fifth of the
// match stage of a 128-frame survey); split 16 ways it is 0.15 ms.
__global__ __launch_bounds__(256) void pack3_rank_kernel(Pack3Args P)
{
    __shared__ __attribute__((aligned(16))) int keys[1024];
    const int img = blockIdx.y;
    const int64_t r0 = P.src_off ? P.src_off[img] : 0;
    const int n = (int)(P.src_off ? P.src_off[img + 1] - r0 : P.single_n);
    if ((int)blockIdx.x * 256 >= n) return;
    // (only the images pack3_rank_bins_kernel left: it drops RANK_TODO at the head of the image's sct slice)
    if (P.sct[P.dst_off ? P.dst_off[img] : 0] != RANK_TODO) return;
    const int r = blockIdx.x * 256 + threadIdx.x;
    const int mine = r < n ? P.n2[r0 + r] : 0;
    const int tiles = (n + 1023) / 1024, per = (tiles + (int)gridDim.z - 1) / (int)gridDim.z;
    const int b_lo = (int)blockIdx.z * per * 1024, b_hi = min(n, b_lo + per * 1024);
    int cnt = 0;
    for (int base = b_lo; base < b_hi; base += 1024) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = base + k * 256 + threadIdx.x;
            keys[k * 256 + threadIdx.x] = j < n ? P.n2[r0 + j] : 0x7FFFFFFF;
        }
        __syncthreads();
        // rows before r with key <= mine, rows after r with key < mine (the fill value of the
        // last tile never counts)
        for (int j = 0; j < 1024; j += 4) {
            const v4i k = *reinterpret_cast<const v4i *>(&keys[j]);
            cnt += (k.x < mine) || (k.x == mine && base + j < r);
            cnt += (k.y < mine) || (k.y == mine && base + j + 1 < r);
            cnt += (k.z < mine) || (k.z == mine && base + j + 2 < r);
            cnt += (k.w < mine) || (k.w == mine && base + j + 3 < r);
        }
    }
    if (r < n) {
        if (gridDim.z == 1) P.pos[r0 + r] = cnt;
        else if (cnt) atomicAdd(&P.pos[r0 + r], cnt);
    }
}

template <typename SRC>
__global__ __launch_bounds__(256) void pack3_scatter_kernel(Pack3Args P)
{
    const int img = blockIdx.y;
    const int64_t r0 = P.src_off ? P.src_off[img] : 0;
    const int n = (int)(P.src_off ? P.src_off[img + 1] - r0 : P.single_n);
    const int d0 = P.dst_off ? P.dst_off[img] : 0;
    const int cap = (n + CHUNK - 1) / CHUNK * CHUNK;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int r = t >> 3, part = t & 7;
    if (r >= cap) return;
    if (r >= n) {                              // padding rows n .. cap-1
        *reinterpret_cast<uint4 *>(P.dst + (int64_t)(d0 + r) * D + part * 16) = make_uint4(0, 0, 0, 0);
        if (part == 0) {
            P.sn2[d0 + r] = 0;
            P.sct[d0 + r] = BIG;
            P.sperm[d0 + r] = -1;
            P.sinv[d0 + r] = -1;
        }
        return;
    }
    const SRC *p = static_cast<const SRC *>(P.src) + (r0 + r) * D + part * 16;
    unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i)
        w[i >> 2] |= (unsigned)((load_value(p, i) - IAMX_DESC_OFFSET) & 0xFF) << (8 * (i & 3));
    const int pos = d0 + P.pos[r0 + r];
    *reinterpret_cast<uint4 *>(P.dst + (int64_t)pos * D + part * 16) = make_uint4(w[0], w[1], w[2], w[3]);
    if (part == 0) {
        P.sn2[pos] = P.n2[r0 + r];
        P.sct[pos] = P.nb[r0 + r] >> 1;
        P.sperm[pos] = r;
        P.sinv[d0 + r] = pos - d0;
    }
}

// ---------------------------------------------------------------------------------
// sweep
// ---------------------------------------------------------------------------------
// a row partial in 8 bytes (16 until round 6: the partials are a quarter of the sweep's HBM traffic,
// all of the candidate pass's, and what bounds the pairs of a round): the lower bound L and the
// two upper bounds as 16-bit offsets from it -- an offset that does not fit (the waves' minima of a
// row lie a few thousand apart) saturates and reads back as "no bound": still an upper bound.
constexpr int ROW_NO_BOUND = 0x7F000000;
__device__ __forceinline__ int pack_row_bounds(int L, int U1, int U2)
{
#if defined(IAMX_T_NOPACK)
    return U1;                           // (timing only)
#else
    // v_cvt_pk_u16_u32: both offsets (never negative) saturated to 16 bits and packed in ONE
    // instruction -- the merge sits on the critical path of its waves (one wave per SIMD: nothing
    // hides a dependent VALU chain), every instruction in it shows in the sweep's time
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    const us2 d = __builtin_amdgcn_cvt_pk_u16((unsigned)(U1 - L), (unsigned)(U2 - L));
    return (int)__builtin_bit_cast(unsigned, d);
#endif
}
__device__ __forceinline__ void unpack_row_bounds(v2i e, int &L, int &U1, int &U2)
{
    const int d1 = e.y & 0xFFFF, d2 = (int)((unsigned)e.y >> 16);
    L = e.x;
    U1 = d1 == 0xFFFF ? ROW_NO_BOUND : e.x + d1;
    U2 = d2 == 0xFFFF ? ROW_NO_BOUND : e.x + d2;
}

struct SymArgs {
    const int8_t *sdesc;
    const int32_t *sn2, *sct;
    const int32_t *img_off, *img_n;
    const int32_t *upairs;       // [n_u][2]: (B image = register resident, A image = streamed)
    const int32_t *wg_off;       // [n_u+1] scan of ceil(n_B / rows per workgroup)
    const int64_t *col_off;      // [n_u] first column-result row (sum of B caps)
    const int64_t *rowp_off;     // [n_u] first row partial (sum of workgroups x A caps)
    int32_t *col;                // [..][2]  (v1, v2)
    int32_t *rowp;               // [..][2]  (L, (U1 - L) | (U2 - L) << 16, each saturated at 0xFFFF = "no bound")
    int n_u, total_wg;
    uint8_t *colmask;            // [..] per column-result row: the groups (bit (tile & 3) + 4 * lane half)
                                 //      whose minimum is <= v2 (NULL: not wanted) -- the only train rows
                                 //      that can be the query's best or second (narrow exact stage)
#if defined(IAMX_T_STAMPS)
    unsigned long long *stamps;  // [workgroups][waves][4]: segment sum (knn2sym16_kernel: pair tails), chunks, loop cycles, loop 100 MHz ticks --
                                 //      a buffer of its own: nothing in the library reads it; knn2sym16_kernel also writes
                                 //      [workgroups][waves] item-start cycles behind that block (5 words a wave in all)
#endif
};

__device__ __forceinline__ int uniform32(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ int64_t uniform64(int64_t x)
{
    return (int64_t)(((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(x >> 32)) << 32) |
                     (unsigned)__builtin_amdgcn_readfirstlane((int)x));
}

// min over the 32 lanes of a half wave (lanes 0-31: g = 0, lanes 32-63: g = 1) of 16 registers
// in 40 VALU instructions (32 half-rate slots) instead of 80: a DPP bank mask selects QUADS
// (lane bits 3:2) and a row mask 16-lane rows, so the levels "xor 8", "xor 4" and "xor 16" can
// keep a DIFFERENT register in the two halves they combine (a transposing butterfly: 16 -> 8
// -> 4 -> 2 registers); only the two levels inside a quad run on every remaining register.
// On return every lane of quad (b4 = lane bit 4, b3, b2) holds
//     m0 = min over the half wave of r[4*b4 + 2*b2 + b3],   m1 = ... of r[8 + 4*b4 + 2*b2 + b3].
// FUSED: the two masked levels as v_min_i32_dpp (DPP source and minimum in ONE instruction, the
// bank mask leaves the other quads' value in place: 2 instead of 3 instructions per register
// pair and no copies), written as inline assembly -- the compiler only forms v_min_dpp where
// the mask is full.  A DPP read needs two wait states after a VALU write of the register; the
// hazard recogniser does not look into inline assembly, hence the s_nop in front of each level
// (inside a level no instruction reads through DPP what an earlier one of the level wrote).
// `lo`: added to the four registers that are left after the two levels inside a 16-lane row
// (lanes l, l^4, l^8, l^12 hold the same `lo`, see GROUPLO in the sweep): 4 adds instead of 16.
template <bool FUSED>
__device__ __forceinline__ void half_wave_min16(int (&r)[16], int lo, int &m0, int &m1)
{
    int u[4], w[2];
    if constexpr (FUSED) {
        asm("s_nop 1\n\t"
            "v_min_i32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
            "v_min_i32_dpp %0, %8, %8 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
            "v_min_i32_dpp %1, %1, %1 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
            "v_min_i32_dpp %1, %9, %9 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
            "v_min_i32_dpp %2, %2, %2 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
            "v_min_i32_dpp %2, %10, %10 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
            "v_min_i32_dpp %3, %3, %3 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
            "v_min_i32_dpp %3, %11, %11 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
            "v_min_i32_dpp %4, %4, %4 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
            "v_min_i32_dpp %4, %12, %12 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
            "v_min_i32_dpp %5, %5, %5 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
            "v_min_i32_dpp %5, %13, %13 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
            "v_min_i32_dpp %6, %6, %6 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
            "v_min_i32_dpp %6, %14, %14 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
            "v_min_i32_dpp %7, %7, %7 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
            "v_min_i32_dpp %7, %15, %15 row_ror:8 row_mask:0xf bank_mask:0xc"
            : "+v"(r[0]), "+v"(r[2]), "+v"(r[4]), "+v"(r[6]), "+v"(r[8]), "+v"(r[10]), "+v"(r[12]), "+v"(r[14])
            : "v"(r[1]), "v"(r[3]), "v"(r[5]), "v"(r[7]), "v"(r[9]), "v"(r[11]), "v"(r[13]), "v"(r[15]));
        // (quads 0,1 now hold min r[2k], quads 2,3 min r[2k+1], in the register of r[2k])
        asm("s_nop 1\n\t"
            "v_min_i32_dpp %0, %0, %0 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
            "v_min_i32_dpp %0, %4, %4 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
            "v_min_i32_dpp %1, %1, %1 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
            "v_min_i32_dpp %1, %5, %5 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
            "v_min_i32_dpp %2, %2, %2 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
            "v_min_i32_dpp %2, %6, %6 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
            "v_min_i32_dpp %3, %3, %3 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
            "v_min_i32_dpp %3, %7, %7 row_ror:4 row_mask:0xf bank_mask:0xa"
            : "+v"(r[0]), "+v"(r[4]), "+v"(r[8]), "+v"(r[12])
            : "v"(r[2]), "v"(r[6]), "v"(r[10]), "v"(r[14]));
#pragma unroll
        for (int k = 0; k < 4; ++k) u[k] = r[4 * k] + lo;
    } else {
        int s[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {          // lanes xor 8: quads 0,1 keep r[2k], quads 2,3 r[2k+1]
            const int a = r[2 * k], b = r[2 * k + 1];
            const int t1 = __builtin_amdgcn_update_dpp(b, a, 0x128, 0xF, 0x3, false);   // row_ror:8
            const int t2 = __builtin_amdgcn_update_dpp(a, b, 0x128, 0xF, 0xC, false);
            s[k] = min(t1, t2);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {          // lanes xor 4: quads 0,2 keep s[2k], quads 1,3 s[2k+1]
            const int a = s[2 * k], b = s[2 * k + 1];
            const int t1 = __builtin_amdgcn_update_dpp(b, a, 0x12C, 0xF, 0x5, false);   // row_ror:12 = lane+4
            const int t2 = __builtin_amdgcn_update_dpp(a, b, 0x124, 0xF, 0xA, false);   // row_ror:4  = lane-4
            u[k] = min(t1, t2) + lo;
        }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {          // lanes xor 16: v_permlane16_swap exchanges the odd rows
        // of its first operand with the even rows of its second: even rows keep u[2k], odd u[2k+1]
        const v2u x = __builtin_amdgcn_permlane16_swap((unsigned)u[2 * k], (unsigned)u[2 * k + 1], false, false);
        w[k] = min((int)x[0], (int)x[1]);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {          // inside the quads
        w[k] = min(w[k], __builtin_amdgcn_update_dpp(0, w[k], 0xB1, 0xF, 0xF, true));    // quad_perm:[1,0,3,2]
        w[k] = min(w[k], __builtin_amdgcn_update_dpp(0, w[k], 0x4E, 0xF, 0xF, true));    // quad_perm:[2,3,0,1]
    }
    m0 = w[0];
    m1 = w[1];
}

// half_wave_min16<true> cut into four pieces that can ride in four different MFMA gaps (the sweep
// runs them in the steps of the next tile): 0 and 1 the level "xor 8" on register pairs 0-3 and
// 4-7, 2 the level "xor 4" and the floor `lo`, 3 the levels "xor 16" and inside the quads and the
// two stores dst[0] = m0, dst[16] = m1.  Each asm block opens with its own s_nop 1 (DPP reads).
template <int P>
__device__ __forceinline__ void row_min16_piece(int (&r)[16], int (&u)[4], int lo, int *dst)
{
    if constexpr (P == 0) {
        asm("s_nop 1\n\t"
            "v_min_i32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
            "v_min_i32_dpp %0, %4, %4 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
            "v_min_i32_dpp %1, %1, %1 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
            "v_min_i32_dpp %1, %5, %5 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
            "v_min_i32_dpp %2, %2, %2 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
            "v_min_i32_dpp %2, %6, %6 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
            "v_min_i32_dpp %3, %3, %3 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
            "v_min_i32_dpp %3, %7, %7 row_ror:8 row_mask:0xf bank_mask:0xc"
            : "+v"(r[0]), "+v"(r[2]), "+v"(r[4]), "+v"(r[6])
            : "v"(r[1]), "v"(r[3]), "v"(r[5]), "v"(r[7]));
    } else if constexpr (P == 1) {
        asm("s_nop 1\n\t"
            "v_min_i32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
            "v_min_i32_dpp %0, %4, %4 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
            "v_min_i32_dpp %1, %1, %1 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
            "v_min_i32_dpp %1, %5, %5 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
            "v_min_i32_dpp %2, %2, %2 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
            "v_min_i32_dpp %2, %6, %6 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
            "v_min_i32_dpp %3, %3, %3 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
            "v_min_i32_dpp %3, %7, %7 row_ror:8 row_mask:0xf bank_mask:0xc"
            : "+v"(r[8]), "+v"(r[10]), "+v"(r[12]), "+v"(r[14])
            : "v"(r[9]), "v"(r[11]), "v"(r[13]), "v"(r[15]));
    } else if constexpr (P == 2) {
        asm("s_nop 1\n\t"
            "v_min_i32_dpp %0, %0, %0 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
            "v_min_i32_dpp %0, %4, %4 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
            "v_min_i32_dpp %1, %1, %1 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
            "v_min_i32_dpp %1, %5, %5 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
            "v_min_i32_dpp %2, %2, %2 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
            "v_min_i32_dpp %2, %6, %6 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
            "v_min_i32_dpp %3, %3, %3 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
            "v_min_i32_dpp %3, %7, %7 row_ror:4 row_mask:0xf bank_mask:0xa"
            : "+v"(r[0]), "+v"(r[4]), "+v"(r[8]), "+v"(r[12])
            : "v"(r[2]), "v"(r[6]), "v"(r[10]), "v"(r[14]));
#pragma unroll
        for (int k = 0; k < 4; ++k) u[k] = r[4 * k] + lo;
    } else {
        int w[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const v2u x = __builtin_amdgcn_permlane16_swap((unsigned)u[2 * k], (unsigned)u[2 * k + 1], false, false);
            w[k] = min((int)x[0], (int)x[1]);
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            w[k] = min(w[k], __builtin_amdgcn_update_dpp(0, w[k], 0xB1, 0xF, 0xF, true));    // quad_perm:[1,0,3,2]
            w[k] = min(w[k], __builtin_amdgcn_update_dpp(0, w[k], 0x4E, 0xF, 0xF, true));    // quad_perm:[2,3,0,1]
        }
        dst[0] = w[0];
        dst[16] = w[1];
    }
}

// The two asm levels of half_wave_min16<true> in SIX blocks of four DPP instructions (round 13: a
// block of eight filled its MFMA gap twice over).  P = 0..3: the level "xor 8" on register pairs
// 2P and 2P + 1; P = 4, 5: the level "xor 4" on the register quadruples 2(P-4) and 2(P-4) + 1 and
// (the sweep adds their floor `lo` itself, as it runs the levels "xor 16" and inside the quads: one
// or two instructions a gap).  Each block opens with its own s_nop 1 (DPP reads).
template <int P, bool PASS>
__device__ __forceinline__ void row_min16_block(int (&r)[16], int &after)
{
    static_assert(P >= 0 && P < 6, "six blocks");
    // (`after`: a value the block follows; with PASS it leaves the block again, so that what reads it next
    //  follows the block.  The block's text does not touch it.)
    int keep = after;
    if constexpr (P < 4) {
        asm("s_nop 1\n\t"
            "v_min_i32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
            "v_min_i32_dpp %0, %3, %3 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
            "v_min_i32_dpp %1, %1, %1 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
            "v_min_i32_dpp %1, %4, %4 row_ror:8 row_mask:0xf bank_mask:0xc"
            : "+v"(r[4 * P]), "+v"(r[4 * P + 2]), "+v"(keep)
            : "v"(r[4 * P + 1]), "v"(r[4 * P + 3]));
    } else {
        constexpr int Q = 8 * (P - 4);
        asm("s_nop 1\n\t"
            "v_min_i32_dpp %0, %0, %0 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
            "v_min_i32_dpp %0, %3, %3 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
            "v_min_i32_dpp %1, %1, %1 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
            "v_min_i32_dpp %1, %4, %4 row_ror:4 row_mask:0xf bank_mask:0xa"
            : "+v"(r[Q]), "+v"(r[Q + 4]), "+v"(keep)
            : "v"(r[Q + 2]), "v"(r[Q + 6]));
    }
    if constexpr (PASS) after = keep;
}

// One piece of form 2's stage in the chunk loop (round 16): the LDS-DMA load as an asm statement, so that it
// can be HELD in a gap of the step that carries valu instructions only -- it follows and feeds the running
// minimum `after`, the way row_min16_block is held -- instead of landing in the step's last gap beside the
// operand reads, where an LDS-DMA instruction costs several times its issue slot.  `lds_dst`: the wave's LDS
// byte address (wave-uniform, M0's value); `gsrc`: the lane's source.  M0 belongs to the compiler and is not
// preserved around a statement: it is saved, written and read in this ONE statement and put back.  The
// compiler does not count an asm load: what waits for these pieces is the chunk loop's own explicit
// s_waitcnt vmcnt(0) at its barrier step (and the one behind the loop) -- every piece is issued in program
// order before it, vmcnt(0) waits for ALL of the wave's outstanding vector memory loads, counted by the
// hardware and not by the compiler, and the barrier behind it covers the other waves' pieces.
template <int BYTES>
__device__ __forceinline__ void stage_piece_held(const void *gsrc, unsigned lds_dst, int &after)
{
    static_assert(BYTES == 16 || BYTES == 4, "one dwordx4 or one dword a lane");
    unsigned m0_was;
    int keep = after;
    if constexpr (BYTES == 16)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(m0_was), "+v"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
    else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %2, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(m0_was), "+v"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
    after = keep;
}

// The same piece where nothing has to hold it: a pair's first two stages of the 16x16x64 item kernel, issued in
// front of the B slice's loads.  An asm load as above, so the compiler neither counts it -- the waits it puts
// behind the loads that follow count those alone, and loads return in order -- nor puts a wait of its own in
// front of a later LDS access; the kernel's explicit s_waitcnt vmcnt(0) in front of the pair's first barrier
// waits for it.
template <int BYTES>
__device__ __forceinline__ void stage_piece(const void *gsrc, unsigned lds_dst)
{
    static_assert(BYTES == 16 || BYTES == 4, "one dwordx4 or one dword a lane");
    unsigned m0_was;
    if constexpr (BYTES == 16)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(m0_was) : "v"(gsrc), "s"(lds_dst) : "memory");
    else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(m0_was) : "v"(gsrc), "s"(lds_dst) : "memory");
}

// IAMX_T_STAMPS=<segment>: a DIAGNOSTIC build of form 2 (tools/sweep_stamps.py; never the shipped library)
// that brackets ONE segment of the chunk loop with s_memtime and adds the differences into a 64-bit scalar
// sum.  Segment 1..16: step segment - 1; 17: the barrier step's s_waitcnt; 18: its s_barrier; 19: two stamps
// back to back (the stamp's own cost).  Every such build also brackets the whole loop with s_memtime and
// s_memrealtime (the in-kernel clock).  A stamp is one asm statement between two scheduling fences; its
// lgkmcnt(0) is part of it (s_memtime returns out of order with LDS reads).  Read SHARES from such a build,
// never its run time: the fences forbid overlaps the shipped loop has.
#if defined(IAMX_T_STAMPS)
#define SWEEP_STAMP(t)                                                                     \
    do {                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                 \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");       \
        __builtin_amdgcn_sched_barrier(0);                                                 \
    } while (0)
#endif

// Form 2's chunk loop: the valu instructions that go behind MFMA `g` (0..7) of a step with `nv` of them
// and `tail` other vector instructions (they end up in the last gap).  With `blocks`, gaps 3 and 4 hold
// one minimum and an asm block of the row butterfly each.  Six issue slots a gap.
constexpr int sweep_gap_valu(int nv, int tail, bool blocks, int g)
{
    const int last = tail < 6 ? 6 - tail : 0;
    const int rest = nv - last - (blocks ? 2 : 0), n = blocks ? 5 : 7;
    if (g == 7) return last;
    if (blocks && (g == 3 || g == 4)) return 1;
    const int i = blocks && g > 4 ? g - 2 : g;
    return rest / n + (i < rest % n ? 1 : 0);
}

// Form 2's chunk loop: which of a step's 32 minima is written `i`-th (0..15 the row minimum of accumulator
// register i, 16 + w the column minimum w: chain 0, w < 8, reads acc0 only, chain 1 acc1 only).  A step opens
// with chain 0 (round 16): acc0 was written two MFMAs before the step's first valu instruction, acc1 by the
// MFMA right in front of it, and a row minimum reads both -- the compiler padded 13 of the 16 step heads
// with an s_nop of 1 to 5 wait states (54 a chunk) in gaps that are full without it.  Chain 1 follows, then
// the rows.  With `blocks`, minima 6 and 7 of chain 0 are held back to positions `p3` and `p3 + 1`, the single
// minima of gaps 3 and 4, which the asm blocks of the row butterfly follow.  `min` is exact in any order, and
// every chain keeps its own order.
constexpr int sweep_min_order(bool blocks, int p3, int i)
{
    const int head = blocks ? 6 : 8;
    if (i < head) return 16 + i;
    if (blocks && (i == p3 || i == p3 + 1)) return 16 + 6 + (i - p3);
    const int f = i - (blocks && i < p3 ? 6 : 8);       // chain 1, then the rows
    return f < 8 ? 24 + f : f - 8;
}

// a loop whose index is a compile-time constant in its body: f(int_c<I>) for I = FROM .. TO - 1
template <int V> struct int_c { static constexpr int value = V; };
template <int FROM, int TO, typename F>
__device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (FROM < TO) {
        f(int_c<FROM>{});
        static_for<FROM + 1, TO>(f);
    }
}

// PIPE: the MFMAs of a pair of query blocks are issued while the minima of the previous pair are
// taken (software pipeline across the 8 steps of a chunk, sched_group_barrier interleave); PIPE
// epilogue VALU instructions go beside every MFMA.
// MERGEW: waves that share the per-chunk row merge (CHUNK / MERGEW rows each).
// GROUPLO: the Cq floor is shared by the four lanes l, l^4, l^8, l^12 (they hold 4 QW consecutive
// sorted rows) and added after the two butterfly levels inside a 16-lane row instead of riding in
// the C operand; with it the fused butterfly (half_wave_min16<true>).
// The timing ablations (VARIANT), the de-phasing sleep (SLEEP), the Cq floor in the C operand
// (GROUPLO = false), 256-row chunks (CH), other merge splits and the unpipelined tile loop were
// measured and removed (profiles/r2_knn2sym_ablate*.txt); the parameters stay in the kernel's name.
// VARIANT = 1 (ITEMS, form 2: iamx_knn2sym_sweep_items): a workgroup walks an ITEM instead of one
// (pair, slice) found by a binary search.  A.wg_off is then the item table ([total_wg][3]: first
// unordered pair, pair count, B slice -- kernels.sym_items), one read per workgroup.  The pairs of
// an item share their B image (the pairs are sorted by B), so the B slice stays in registers from
// one pair to the next and is reloaded only where the image changes; per pair the workgroup
// switches the A stream, the row partials' buffer resource and the column results, and the
// pipeline drains and refills (a barrier, the pair's first two stages).  One wave launch, one
// table read and one B load per item instead of per pair.  VARIANT = 0 compiles to the same
// instructions as before the item walk existed (the pair loop folds away).
template <int QW, int NW, int VARIANT, int PIPE, int MERGEW, int SLEEP, bool GROUPLO, int CH, int WPE>
__global__ __launch_bounds__(NW * 64, WPE) void knn2sym_kernel(SymArgs A)
{
    static_assert((VARIANT == 0 || VARIANT == 1) && PIPE > 0 && MERGEW == 2 && SLEEP == 0 && GROUPLO && CH == 128,
                  "only the shipped sweep is implemented");
    constexpr bool ITEMS = VARIANT == 1;
    constexpr int CHUNK = CH;        // train rows per LDS stage
    constexpr int WGROWS = NW * QW * 32;
    constexpr int NT = NW * 64;
    constexpr int PIECES = CHUNK * D / 16 / NT;
    // (R_w: three buffers -- a chunk's last row minima are stored while the next chunk runs, and its
    //  merge follows the next chunk's barrier; the dump area takes a lane's stores at the same buffer
    //  offsets as the row area)
    __shared__ __attribute__((aligned(16))) int8_t lds[2 * CHUNK * D + 2 * CHUNK * 4 + 3 * NW * CHUNK * 4 + 2 * NW * 4 + (2 * NW * CHUNK + NW * 256) * 4];   // (lds_cq: NW used)
    int8_t *lds_tile = lds;
    int *lds_tb = reinterpret_cast<int *>(lds + 2 * CHUNK * D);      // [2][CHUNK]     Ct
    int *lds_row = lds_tb + 2 * CHUNK;                               // [3][NW][CHUNK] R_w
    int *lds_cq = lds_row + 3 * NW * CHUNK;                          // [NW] (2 NW reserved) S_w
    int *lds_dump = lds_cq + 2 * NW;                                 // [NW][256] (+ 2 buffer strides) unused stores
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 31, g = lane >> 5;

    int vid;
    {
        const int total = A.total_wg, bid = blockIdx.x;
        const int xcd = bid & 7, k = bid >> 3, q = total >> 3, r = total & 7;
        vid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
    }
    int lo = 0, hi = A.n_u;
    if constexpr (!ITEMS)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (A.wg_off[mid] <= vid) lo = mid; else hi = mid;
        }
    int u = lo, u_end = 0, item_wgi = 0;
    if constexpr (ITEMS) {
        u = A.wg_off[3 * vid];
        u_end = u + A.wg_off[3 * vid + 1];
        item_wgi = A.wg_off[3 * vid + 2];
    }
    v4i bq[QW][4];
    int lo_lane;
    int bimg_held = -1;              // (ITEMS: the B image whose slice bq holds)
    // (ITEMS: the item's loop state lives in vector registers and is read back through readfirstlane
    //  where it is used: the chunk loop already holds 96 scalar registers, and with this state in
    //  scalar registers too its barrier step spread over three MFMA gaps of 22-27 instructions)
    if constexpr (ITEMS) asm volatile("" : "+v"(u_end), "+v"(item_wgi), "+v"(bimg_held));
    // ITEMS: the table entries of the pair the loop runs next, read one pair ahead -- its images and
    // offsets in front of the current pair's first stages (they land with them), the images' store
    // offsets and rows behind that pair's first barrier (they land during its chunk loop) -- and
    // taken through readfirstlane: behind the pair's stores they are vector loads, and the row
    // partials' buffer resource must stay in scalar registers (no waterfall loop around the merge)
#if defined(IAMX_T_STAMPS)
    unsigned long long stamp_sum = 0, stamp_chunks = 0, stamp_cycles = 0, stamp_ticks = 0;
#endif
    int nx_b = 0, nx_a = 0, nx_boff = 0, nx_nb = 0, nx_aoff = 0, nx_na = 0;
    int64_t nx_rowp = 0;
    if constexpr (ITEMS) {
        nx_b = A.upairs[2 * u];
        nx_a = A.upairs[2 * u + 1];
        nx_boff = A.img_off[nx_b];
        nx_nb = A.img_n[nx_b];
        nx_aoff = A.img_off[nx_a];
        nx_na = A.img_n[nx_a];
        nx_rowp = A.rowp_off[u];
    }
    for (;;) {
        const int bimg = ITEMS ? uniform32(nx_b) : A.upairs[2 * u], aimg = ITEMS ? uniform32(nx_a) : A.upairs[2 * u + 1];
        const int boff = ITEMS ? uniform32(nx_boff) : A.img_off[bimg], nb = ITEMS ? uniform32(nx_nb) : A.img_n[bimg];
        const int aoff = ITEMS ? uniform32(nx_aoff) : A.img_off[aimg], na = ITEMS ? uniform32(nx_na) : A.img_n[aimg];
        const int capA = (na + CHUNK - 1) / CHUNK * CHUNK;
        const int nchunks = capA / CHUNK;
        const int wgi = ITEMS ? uniform32(item_wgi) : vid - A.wg_off[u];
        const int q0 = wgi * WGROWS + wave * (QW * 32);
        const bool wave_valid = q0 < nb;
        const int64_t rbase = (ITEMS ? uniform64(nx_rowp) : A.rowp_off[u]) + (int64_t)wgi * capA;
        // (ITEMS, from the item's second pair on: every wave is past the previous pair's last merge
        //  -- its lds_row reads -- before an invalid wave refills its rows with BIG below)
        if constexpr (ITEMS)
            if (uniform32(bimg_held) >= 0) __syncthreads();

        // B operand: lane (c, g) holds bytes [32s+16g, +16) of the QW consecutive (sorted) B rows
        // q0 + QW*c + qb; rows past the end repeat the last row (it belongs to this wave, so the
        // group minimum is unchanged).  Cq of a lane's rows lies in [lo_lane, lo_lane + spread]:
        // lo_lane rides into the sweep with the C operand, the wave's largest spread S_w (a few
        // hundred for SIFT-like rows, the rows are sorted) widens the upper bound afterwards.
        // (GROUPLO: lane c holds the row quadruple rc, c's bits 3:2 moved to the bottom, so that
        //  the lanes that differ in bits 3:2 hold 4 QW CONSECUTIVE rows)
        const int rc = (c & 16) | ((c & 3) << 2) | ((c >> 2) & 3);
        if (!ITEMS || bimg != uniform32(bimg_held)) {
            bimg_held = bimg;
#pragma unroll
            for (int qb = 0; qb < QW; ++qb) {
                int row = q0 + QW * rc + qb;
                row = row < nb ? row : nb - 1;
                const v4i *src = reinterpret_cast<const v4i *>(A.sdesc + (int64_t)(boff + row) * D);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    bq[qb][s] = ~src[2 * s + g];
                    // one wave per SIMD (512 registers): the B operand -- only ever an MFMA source -- belongs
                    // in the AGPR half, the accumulators the VALU reads in the VGPR half; left alone the
                    // allocator does the opposite and pays a v_accvgpr_read per accumulator element
                    if constexpr (WPE == 1) asm volatile("" : "+a"(bq[qb][s]));
                }
            }
            lo_lane = 0;
            {
                int spread = 0;
                if (wave_valid) {
                    const int g_lo = rc & ~3, g_hi = rc | 3;
                    const int r_lo = q0 + QW * g_lo < nb ? q0 + QW * g_lo : nb - 1;
                    const int r_hi = q0 + QW * g_hi + QW - 1 < nb ? q0 + QW * g_hi + QW - 1 : nb - 1;
                    lo_lane = A.sn2[boff + r_lo] >> 1;
                    spread = (A.sn2[boff + r_hi] >> 1) - lo_lane;
                }
#pragma unroll
                for (int sh = 32; sh >= 1; sh >>= 1) spread = max(spread, __shfl_xor(spread, sh));
                if (lane == 0) lds_cq[wave] = spread;
            }
        }
        if (!wave_valid) {
#pragma unroll
            for (int k = 0; k < 3 * CHUNK / 64; ++k)
                lds_row[((k / (CHUNK / 64)) * NW + wave) * CHUNK + (k % (CHUNK / 64)) * 64 + lane] = BIG;
        }
        int m[QW][4];
#pragma unroll
        for (int qb = 0; qb < QW; ++qb)
#pragma unroll
            for (int k = 0; k < 4; ++k) m[qb][k] = BIG;

        const int8_t *tbase = A.sdesc + (int64_t)aoff * D;
        const int32_t *tci = A.sct + aoff;
        // global -> LDS directly; the XOR swizzle of the 16-byte slots is applied on the source side
        typedef __attribute__((address_space(3))) void *lds_ptr;
        auto stage_direct = [&](int ch, int buf) {
#pragma unroll
            for (int j = 0; j < PIECES; ++j) {
                const int e = j * NT + tid, row = e >> 3, slot = (e & 7) ^ ((row >> 1) & 7);
                const int8_t *gsrc = tbase + (int64_t)(ch * CHUNK + row) * D + slot * 16;
                int8_t *ldst = lds_tile + buf * (CHUNK * D) + (j * NT + wave * 64) * 16;
                __builtin_amdgcn_global_load_lds(gsrc, (lds_ptr)ldst, 16, 0, 0);
            }
            // (Ct: every wave, the waves past CHUNK / 64 repeat the same words -- no branch in the step)
            __builtin_amdgcn_global_load_lds(tci + ch * CHUNK + (tid & (CHUNK - 1)),
                                             (lds_ptr)(lds_tb + buf * CHUNK + (wave & (CHUNK / 64 - 1)) * 64), 4, 0, 0);
        };
        auto wait_direct = [&]() { __builtin_amdgcn_s_waitcnt(0x0F70); };       // vmcnt(0)
        // per train row: the waves' group minima -> (L, U1, U2).  Every wave runs the merge (no branch in
        // the step it rides in); only waves < MERGEW store, through a buffer resource over this
        // workgroup's partials: an offset past num_records drops the store
        constexpr int MROWS = CHUNK / MERGEW;                // rows a merging wave takes
        static_assert(MROWS == 64 && NW % MERGEW == 0, "one merge row per lane");
        const int mrow = (wave % MERGEW) * MROWS + lane;
        const bool merger = wave < MERGEW;
        // Buffer resource over this workgroup's capA partials (8 bytes each): stride 0 (a raw buffer),
        // num_records = capA * 8 bytes.  Word 3 of a gfx9 descriptor: DATA_FORMAT = 4 (32 bits) in bits
        // 15-18, every other field 0 -- the value the gfx9 buffer stores of LLVM and composable_kernel
        // use for untyped dword access (the untyped store ignores the format, but DATA_FORMAT 0 is
        // "invalid").  A raw buffer store whose offset + size exceeds num_records is dropped by the
        // hardware's range check: RANGE_DROP is such an offset for any capA (below 2^31, so offset + 8
        // does not wrap).
        constexpr int RSRC_WORD3_DATA_FORMAT_32 = 4 << 15;
        constexpr int RANGE_DROP = 0x7FFFFFF0;
        const __amdgpu_buffer_rsrc_t rowp_rsrc =
            __builtin_amdgcn_make_buffer_rsrc(A.rowp + 2 * rbase, (short)0, capA * 8, RSRC_WORD3_DATA_FORMAT_32);
        // (the waves' spreads S_w, read once behind the first barrier into scalar registers: the merge
        //  sits on the critical path of its waves -- one wave per SIMD, nothing hides its LDS reads)
        int spread_w[NW];
        auto merge_rows = [&](int ch, int rbo, bool store) {
            int L = BIG, U1 = BIG, U2 = BIG;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const int R = lds_row[rbo + w * CHUNK + mrow];
                const int lw = R, uw = R + spread_w[w];
                L = min(L, lw);
                U2 = min(max(U1, uw), U2);
                U1 = min(U1, uw);
            }
            __builtin_amdgcn_raw_buffer_store_b64(v2i{L, pack_row_bounds(L, U1, U2)}, rowp_rsrc,
                                                  store ? (ch * CHUNK + mrow) * 8 : RANGE_DROP, 0, 0);
        };

        // The tile loop is one software pipeline across the chunks (8 MFMAs a step, PP = QW / 2 steps a
        // tile, 4 tiles a chunk): step s issues the MFMAs of step s + 1 while it takes the minima of
        // step s; the row butterfly of a tile is cut into four pieces that ride in the steps of the NEXT
        // tile (a second r set); the operands of tile t + 2 are read two per step from the last step of
        // tile t on.  The chunk's barrier sits in front of the last step of tile NT4 - 2: every read of
        // the chunk's LDS stage has been issued by then, so the stage of chunk + 2 goes behind it and the
        // reads of the next chunk's first two tiles, the first MFMAs of the next chunk, the last tile's
        // butterfly and the merge of the previous chunk all ride in MFMA gaps.  The last chunk issues
        // (and drops) one step of MFMAs on a repeated stage: no branch in the loop body.
        constexpr int PP = QW / 2, NT4 = CHUNK / 32, NS = NT4 * PP;
        static_assert(NT4 % 2 == 0 && NT4 >= 2, "tile parity must carry across chunks");
        // accumulator register reg of lane half g is tile row 8*(reg>>2) + 4*g + (reg&3); after the
        // butterfly a quad holds reg = 4*b4 + 2*b2 + b3 (m0) and 8 + that (m1).  One lane per quad
        // stores them; the others store into a dump area (no branch in the tile loop: a branch
        // there makes the compiler sink the column minima below it and keep the accumulators alive).
        // A wave past the end of the B image (only in the last workgroup of a pair whose B image is not
        // a multiple of the workgroup's rows) runs the loop too -- it shares the barriers and the merge
        // -- on repeats of the last B row, with every row store in the dump area and no column result:
        // MFMA work on a SIMD that would otherwise idle, the price of a branch-free step.
        int *const row_dst = (lane & 3) == 0 && wave_valid
            ? lds_row + wave * CHUNK + 8 * ((lane >> 4) & 1) + 4 * g + 2 * ((lane >> 2) & 1) + ((lane >> 3) & 1)
            : lds_dump + wave * 256 + lane;                 // (+ row buffer offset + tile*32 + 16: inside the dump area)
        v4i aop[2][4], tbop[2][4];
        v16i accs[2][2];
        int r[2][16], bu[4];
#pragma unroll
        for (int k = 0; k < 16; ++k) r[1][k] = BIG;
        // read k (0..7) of a tile's operands: the C operand Ct first (the first MFMA needs all of it)
        auto load_op = [&](int buf, int tile, int k, v4i (&a)[4], v4i (&tbv)[4]) {
            if (k < 4) {
                tbv[k] = *reinterpret_cast<const v4i *>(lds_tb + buf * CHUNK + tile * 32 + 8 * k + 4 * g);
            } else {
                const int s = k - 4, rr = tile * 32 + c, swz = (rr >> 1) & 7;
                a[s] = *reinterpret_cast<const v4i *>(lds_tile + buf * (CHUNK * D) + rr * D + (((2 * s + g) ^ swz) * 16));
            }
        };
        // (the statement that pins the accumulators to the VGPR half has side effects: it keeps its order
        //  against a held stage piece, so form 2's chunk loop writes it behind its minima -- in front of them
        //  it would push the piece behind the step's last MFMA)
        auto pin_accs = [&](v16i &acc0, v16i &acc1) {
            if constexpr (WPE == 1) asm volatile("" : "+v"(acc0), "+v"(acc1));
        };
        auto issue = [&](int t, int qp, v16i &acc0, v16i &acc1, bool pin = true) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) acc0[reg] = acc1[reg] = tbop[t & 1][reg >> 2][reg & 3];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(aop[t & 1][s], bq[qp][s], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(aop[t & 1][s], bq[qp + 1][s], acc1, 0, 0, 0);
            }
            if (pin) pin_accs(acc0, acc1);
        };

        if constexpr (ITEMS) {           // (the last pair of the item reads its own entries again)
            const int un = u + 1 < u_end ? u + 1 : u;
            nx_b = A.upairs[2 * un];
            nx_a = A.upairs[2 * un + 1];
            nx_rowp = A.rowp_off[un];
        }
        stage_direct(0, 0);
        stage_direct(nchunks > 1 ? 1 : 0, 1);
        wait_direct();
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NW; ++w) spread_w[w] = __builtin_amdgcn_readfirstlane(lds_cq[w]);
        if constexpr (ITEMS) {
            const int b = uniform32(nx_b), a = uniform32(nx_a);
            nx_boff = A.img_off[b];
            nx_nb = A.img_n[b];
            nx_aoff = A.img_off[a];
            nx_na = A.img_n[a];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) load_op(0, 0, k, aop[0], tbop[0]);
#pragma unroll
        for (int k = 0; k < 8 / PP; ++k) load_op(0, 1, k, aop[1], tbop[1]);
        issue(0, 0, accs[0][0], accs[0][1]);
        __builtin_amdgcn_sched_barrier(0);
        // row buffers (offsets in ints) of this chunk and of the previous one; "chunk -1" stores its
        // (meaningless) last tile into the buffer chunk 2 overwrites
        int rbo = 0, rbo_prev = 2 * NW * CHUNK;
        // (the stage inside the chunk loop: ONE lane offset for every piece and chunk -- the swizzle of a
        //  row depends on the row inside its piece only -- beside a scalar base, and the wave's LDS
        //  destination from a scalar register)
        const int wave_u = uniform32(wave);
        // (the operand reads inside the chunk loop: a lane's LDS offsets in the stage buffer the reads go
        //  to, switched by one xor each where the reads move on to the next chunk's buffer -- the tile and
        //  the read ride in the instruction's offset)
        typedef __attribute__((address_space(3))) const int8_t *lds_bytes;
        int opoff[4], tboff = 2 * CHUNK * D + 16 * g;
#pragma unroll
        for (int s = 0; s < 4; ++s) opoff[s] = c * D + (((2 * s + g) ^ ((c >> 1) & 7)) * 16);
        auto load_op_at = [&](int tile, int k, v4i (&a)[4], v4i (&tbv)[4]) {
            if (k < 4) tbv[k] = *reinterpret_cast<const __attribute__((address_space(3))) v4i *>((lds_bytes)lds + tboff + tile * 128 + 32 * k);
            else a[k - 4] = *reinterpret_cast<const __attribute__((address_space(3))) v4i *>((lds_bytes)lds + opoff[k - 4] + tile * (32 * D));
        };
        const unsigned stage_voff = (unsigned)((tid >> 3) * D + (((tid & 7) ^ ((tid >> 4) & 7)) * 16));
        // (the wave's LDS byte addresses of a stage's first piece and of its Ct words, in scalar registers)
        const unsigned lds_tile_at = (unsigned)(uintptr_t)(lds_ptr)(lds_tile + wave_u * (64 * 16));
        const unsigned lds_tb_at = (unsigned)(uintptr_t)(lds_ptr)(lds_tb + (wave_u & (CHUNK / 64 - 1)) * 64);
        const unsigned ct_voff = (unsigned)((tid & (CHUNK - 1)) * 4);
#if defined(IAMX_T_STAMPS)
        const unsigned long long loop_c0 = __builtin_amdgcn_s_memtime(), loop_r0 = __builtin_amdgcn_s_memrealtime();
        __builtin_amdgcn_s_waitcnt(0xC07F);              // lgkmcnt(0) alone: the loop's first LDS waits stay counted
#endif
        for (int ch = 0; ch < nchunks; ++ch) {
            const int buf = ch & 1;
            if constexpr (PP == 4) {
            // Form 2 (round 13): the gap behind every MFMA of a step gets its own count of valu instructions
            // (sched_group_barrier, sweep_gap_valu), so that no gap carries more than the MFMA beside it hides:
            // 6 issue slots of 4 cycles behind the MFMA's own 8, of 32.  A step has 32 minima (16 row minima,
            // then 8 + 8 column minima in two chains) and its share of the previous tile's row butterfly: an
            // asm block of four DPP instructions in each of gaps 3 and 4 of the tile's first three steps, the
            // floor behind the second level, the levels "xor 16" and inside the quads in the fourth step.
            // What is no valu instruction belongs to no group (a group of LDS or memory instructions breaks
            // the pipeline of groups behind it with this compiler) and ends up behind the step's last group:
            // the step's two operand reads, and at most one instruction of the chunk's own work -- the merge of
            // the previous chunk reads, computes and stores in three steps.  The stage of chunk + 2 goes one
            // piece a step into the five steps from the barrier on, never two in one gap; since round 16 a
            // piece is an asm statement held in a gap that carries valu instructions only (stage_piece_held).
            // The chunk's barrier is the head of the last step of tile NT4 - 2; the step in front of it
            // issues no LDS read.
            constexpr int BAR = (NT4 - 1) * PP - 1;
            static_assert(NW == 4 && PIECES == 4 && BAR + 4 < NS && (NT / 8) % 16 == 0, "the gaps below are form 2's");
            const int chs = ch + 2 < nchunks ? ch + 2 : nchunks - 1;
            const int8_t *const sg_tile = tbase + (int64_t)chs * (CHUNK * D);
            const int8_t *const sg_ct = reinterpret_cast<const int8_t *>(tci + chs * CHUNK);
            int mR[NW], mL = BIG, mU1 = BIG, mU2 = BIG;
            static_for<0, NS>([&](auto st_c) {
                constexpr int st = decltype(st_c)::value;
                constexpr int t = st / PP, ph = st % PP, qp = 2 * ph, cur = st & 1;
                constexpr int nst = st + 1 < NS ? st + 1 : 0;
#if defined(IAMX_T_STAMPS)
                unsigned long long stamp_t0 = 0, stamp_t1 = 0;
                if constexpr (IAMX_T_STAMPS == st + 1 || (st == BAR && IAMX_T_STAMPS == 17)) SWEEP_STAMP(stamp_t0);
                if constexpr (st == 0 && IAMX_T_STAMPS == 19) {      // (two stamps back to back: a stamp's own cost)
                    SWEEP_STAMP(stamp_t0);
                    SWEEP_STAMP(stamp_t1);
                    stamp_sum += stamp_t1 - stamp_t0;
                }
#endif
                if constexpr (st == BAR) {
                    // every read of this chunk's stage is done (lgkmcnt), the next chunk's stage has landed
                    // (vmcnt): the stage of chunk + 2 may overwrite this one
                    __builtin_amdgcn_s_waitcnt(0x0070);              // vmcnt(0) lgkmcnt(0)
#if defined(IAMX_T_STAMPS)
                    if constexpr (IAMX_T_STAMPS == 17) {
                        SWEEP_STAMP(stamp_t1);
                        stamp_sum += stamp_t1 - stamp_t0;
                    }
                    if constexpr (IAMX_T_STAMPS == 18) SWEEP_STAMP(stamp_t0);
#endif
                    __syncthreads();
#if defined(IAMX_T_STAMPS)
                    if constexpr (IAMX_T_STAMPS == 18) {
                        SWEEP_STAMP(stamp_t1);
                        stamp_sum += stamp_t1 - stamp_t0;
                    }
#endif
                }
                issue(nst / PP, 2 * (nst % PP), accs[cur ^ 1][0], accs[cur ^ 1][1], false);
                // the operand reads of tile T (flattened across chunks), 8 / PP a step as before; from tile
                // NT4 on they read the next chunk's stage.  The step in front of the barrier has none (the
                // barrier's wait would sit right behind them): the step before that issues them
                // (they are written behind the step's minima: a held stage piece is an asm statement, which no
                //  LDS read crosses, and the reads belong in the step's last gap, behind it)
                auto operand_reads = [&]() {
                    static_for<(st == BAR - 1 ? 1 : 0), (st == BAR - 2 ? 2 : 1)>([&](auto d_c) {
                        constexpr int sr = st + decltype(d_c)::value;
                        constexpr int T = (sr + 1) / PP + 1, i = (sr + 1) % PP;
#pragma unroll
                        for (int k = i * 8 / PP; k < (i + 1) * 8 / PP; ++k) load_op_at(T % NT4, k, aop[T & 1], tbop[T & 1]);
                    });
                };
                if constexpr (st == BAR) {           // (its reads are tile NT4's first: the next chunk's stage)
#pragma unroll
                    for (int s = 0; s < 4; ++s) opoff[s] ^= CHUNK * D;
                    tboff ^= CHUNK * 4;
                }
                // the valu instructions of the step (the two swaps of the fourth step count twice) and what
                // its last gap holds beside them
                constexpr int nv = (ph == 2 ? 36 : ph == 3 ? 40 : 32) + (st == BAR + 2 ? 11 : 0) + (st == BAR + 3 ? 5 : 0) +
                                   (st >= BAR && st <= BAR + PIECES ? 1 : 0) +    // (a stage instruction's address)
                                   (st == NS - 1 ? 2 : 0);                          // (the loop's own)
                constexpr int tail = (st == BAR - 1 ? 0 : st == BAR - 2 ? 4 : 2) + (ph == 3 ? 1 + 2 : 0) +
                                     (st == BAR + 1 ? 2 : 0) + (st == BAR + 3 ? 1 : 0);
                // (a step from the barrier on holds one piece of the stage of chunk + 2 in gap STAGE_GAP, which
                //  carries valu instructions only: behind the second minimum of column chain 1, which it follows,
                //  and one valu instruction fewer in that gap)
                constexpr bool staging = st >= BAR && st <= BAR + PIECES;
                constexpr int STAGE_GAP = 1, STAGE_AT = 8 + 1;
                // (the asm blocks of the row butterfly belong to no group: the first sits between the column
                //  minimum that is the one valu instruction of gap 3 and the next one -- it passes the running
                //  minimum through -- and the second reads that next one, the one of gap 4)
                // (in a staging step the piece's address is a valu instruction in front of them, and gap 1 holds one fewer)
                constexpr int blk_at = sweep_gap_valu(nv, tail, true, 0) + sweep_gap_valu(nv, tail, true, 1) +
                                       sweep_gap_valu(nv, tail, true, 2) - (staging ? 2 : 0);
                static_assert(ph == 3 || (blk_at >= 6 && blk_at < 31), "gaps 3 and 4 hold the last two minima of column chain 0");
                // minima of this step, in the order of sweep_min_order: column chain 0 first (it reads acc0
                // alone), then column chain 1 (a held stage piece follows its second minimum, which that order
                // puts in gap 1 or 2), then the rows; with them the previous tile's row butterfly
                // (tile NT4 - 1 of the previous chunk for t = 0)
                const v16i acc0 = accs[cur][0], acc1 = accs[cur][1];
                int (&rc_)[16] = r[t & 1];
                int (&rp)[16] = r[(t + 1) & 1];
                static_for<0, 32>([&](auto i_c) {
                    constexpr int i = decltype(i_c)::value, op = sweep_min_order(ph < 3, blk_at, i);
                    if constexpr (op < 16) {
                        rc_[op] = qp == 0 ? min(acc0[op], acc1[op]) : min(min(rc_[op], acc0[op]), acc1[op]);
                    } else {
                        constexpr int w = op - 16;
                        int &mm = m[qp + (w >> 3)][t & 3];
                        const v16i &acc = w < 8 ? acc0 : acc1;
                        mm = min(min(mm, acc[2 * (w & 7)]), acc[2 * (w & 7) + 1]);
                        if constexpr (ph < 3 && i == blk_at) row_min16_block<2 * ph, true>(rp, mm);
                        if constexpr (ph < 3 && i == blk_at + 1) row_min16_block<2 * ph + 1, true>(rp, mm);
                        // the stage of chunk + 2, one piece a step: its buffer is free behind the barrier, its
                        // data is due a chunk later (the next chunk's barrier step waits for it)
                        if constexpr (staging && w == STAGE_AT) {
                            if constexpr (st < BAR + PIECES)
                                stage_piece_held<16>(sg_tile + (st - BAR) * ((NT / 8) * D) + stage_voff,
                                                     lds_tile_at + buf * (CHUNK * D) + (st - BAR) * NT * 16, mm);
                            else
                                stage_piece_held<4>(sg_ct + ct_voff, lds_tb_at + buf * (CHUNK * 4), mm);
                        }
                    }
                });
                pin_accs(accs[cur ^ 1][0], accs[cur ^ 1][1]);
                operand_reads();
                if constexpr (ph == 2) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) bu[k] = rp[4 * k] + lo_lane;
                }
                if constexpr (ph == 3) {
                    int *const dst = row_dst + (t > 0 ? rbo : rbo_prev) + (t > 0 ? t - 1 : NT4 - 1) * 32;
                    row_min16_piece<3>(rp, bu, lo_lane, dst);
                }
                // the chunk's own work behind its barrier: the merge of the previous chunk (its rows' last
                // minima were stored in this chunk's first tile) and the stage of chunk + 2
                // what is no valu instruction belongs to no group and goes behind the step's last group, into
                // its last gap: the step's two operand reads, the store of the row minima, and one piece of the
                // chunk's own work a step from the barrier on -- the merge of the previous chunk (its rows' last
                // minima were stored in this chunk's first tile); the stage of chunk + 2 is held among the minima
                if constexpr (st == BAR + 1) {
#pragma unroll
                    for (int w = 0; w < NW; ++w) mR[w] = lds_row[rbo_prev + w * CHUNK + mrow];
                }
                if constexpr (st == BAR + 2) {
#pragma unroll
                    for (int w = 0; w < NW; ++w) {
                        const int uw = mR[w] + spread_w[w];
                        mL = min(mL, mR[w]);
                        mU2 = min(max(mU1, uw), mU2);
                        mU1 = min(mU1, uw);
                    }
                }
                if constexpr (st == BAR + 3)
                    __builtin_amdgcn_raw_buffer_store_b64(v2i{mL, pack_row_bounds(mL, mU1, mU2)}, rowp_rsrc,
                                                          merger && ch > 0 ? ((ch - 1) * CHUNK + mrow) * 8 : RANGE_DROP, 0, 0);
                static_for<0, 8>([&](auto g_c) {
                    constexpr int g = decltype(g_c)::value;
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    // (the last group takes what the counts above missed)
                    __builtin_amdgcn_sched_group_barrier(0x002, sweep_gap_valu(nv, tail, ph < 3, g) + (g == 7 ? 3 : 0) -
                                                                    (staging && g == STAGE_GAP ? 1 : 0), 0);
                });
                __builtin_amdgcn_sched_barrier(0);
#if defined(IAMX_T_STAMPS)
                if constexpr (IAMX_T_STAMPS == st + 1) {
                    SWEEP_STAMP(stamp_t1);
                    stamp_sum += stamp_t1 - stamp_t0;
                }
#endif
            });
            } else {
#pragma unroll
            for (int st = 0; st < NS; ++st) {
                const int t = st / PP, qp = 2 * (st % PP), cur = st & 1;
                if (st == (NT4 - 1) * PP - 1) {
                    // every read of this chunk's stage is done (lgkmcnt), the next chunk's stage has landed
                    // (vmcnt): the stage of chunk + 2 may overwrite this one
                    __builtin_amdgcn_s_waitcnt(0x0070);              // vmcnt(0) lgkmcnt(0)
                    __syncthreads();
                    stage_direct(ch + 2 < nchunks ? ch + 2 : nchunks - 1, buf);
                    merge_rows(ch - 1, rbo_prev, merger && ch > 0);
                }
                // the MFMAs of the next step (the next chunk's first step from the last one)
                if (st + 1 < NS) issue((st + 1) / PP, 2 * ((st + 1) % PP), accs[cur ^ 1][0], accs[cur ^ 1][1]);
                else issue(0, 0, accs[cur ^ 1][0], accs[cur ^ 1][1]);
                // the operand reads of tile T (flattened across chunks) run from the last step of tile T - 2
                // to the step before T's first MFMAs, 8 / PP a step: here those of tile T = (st + 1) / PP + 1
                {
                    const int T = (st + 1) / PP + 1, i = (st + 1) % PP;
#pragma unroll
                    for (int k = i * 8 / PP; k < (i + 1) * 8 / PP; ++k)
                        load_op(T < NT4 ? buf : buf ^ 1, T % NT4, k, aop[T & 1], tbop[T & 1]);
                }
                // minima of this step
                const v16i acc0 = accs[cur][0], acc1 = accs[cur][1];
                int t0 = min(min(m[qp][t & 3], acc0[0]), acc0[1]);
                int t1m = min(min(m[qp + 1][t & 3], acc1[0]), acc1[1]);
#pragma unroll
                for (int reg = 2; reg < 16; reg += 2) {
                    t0 = min(min(t0, acc0[reg]), acc0[reg + 1]);
                    t1m = min(min(t1m, acc1[reg]), acc1[reg + 1]);
                }
                m[qp][t & 3] = t0;
                m[qp + 1][t & 3] = t1m;
                int (&rc_)[16] = r[t & 1];
                if (qp == 0) {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) rc_[reg] = min(acc0[reg], acc1[reg]);
                } else {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) rc_[reg] = min(min(rc_[reg], acc0[reg]), acc1[reg]);
                }
                // pieces of the previous tile's row butterfly (tile NT4 - 1 of the previous chunk for t = 0)
                {
                    int (&rp)[16] = r[(t + 1) & 1];
                    const int tp = t > 0 ? t - 1 : NT4 - 1;
                    int *dst = row_dst + (t > 0 ? rbo : rbo_prev) + tp * 32;
                    if constexpr (PP == 1) {                         // (one step a tile: the whole butterfly)
                        int m0, m1;
                        half_wave_min16<true>(rp, lo_lane, m0, m1);
                        dst[0] = m0;
                        dst[16] = m1;
                    } else {
                        if (0 * PP / 4 == st % PP) row_min16_piece<0>(rp, bu, lo_lane, dst);
                        if (1 * PP / 4 == st % PP) row_min16_piece<1>(rp, bu, lo_lane, dst);
                        if (2 * PP / 4 == st % PP) row_min16_piece<2>(rp, bu, lo_lane, dst);
                        if (3 * PP / 4 == st % PP) row_min16_piece<3>(rp, bu, lo_lane, dst);
                    }
                }
                // one MFMA, then the VALU work (and an operand read) that fits beside it
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, PIPE, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            }
            rbo_prev = rbo;
            rbo = rbo == 2 * NW * CHUNK ? 0 : rbo + NW * CHUNK;
        }
#if defined(IAMX_T_STAMPS)
        if constexpr (PP == 4) {
            unsigned long long loop_c1;
            SWEEP_STAMP(loop_c1);
            stamp_cycles += loop_c1 - loop_c0;
            stamp_ticks += __builtin_amdgcn_s_memrealtime() - loop_r0;
            stamp_chunks += (unsigned)nchunks;
            // (lane 0, ordinary vector stores, after every pair: the sums so far)
            if (A.stamps && lane == 0) {
                unsigned long long *o = A.stamps + ((size_t)blockIdx.x * NW + wave) * 4;
                o[0] = stamp_sum;
                o[1] = stamp_chunks;
                o[2] = stamp_cycles;
                o[3] = stamp_ticks;
            }
        }
#endif
        // (ITEMS: this pair's first column-result row, read here -- it lands with the vmcnt(0) below --
        //  rather than carried through the chunk loop in scalar registers, which the loop needs)
        int64_t col_v = 0;
        if constexpr (ITEMS) col_v = A.col_off[u];
        // the last chunk's last tile, its merge
        {
            int m0, m1;
            half_wave_min16<true>(r[(NT4 - 1) & 1], lo_lane, m0, m1);
            int *dst = row_dst + rbo_prev + (NT4 - 1) * 32;
            dst[0] = m0;
            dst[16] = m1;
        }
        wait_direct();
        __syncthreads();
        merge_rows(nchunks - 1, rbo_prev, merger);

        const int64_t col_u = ITEMS ? uniform64(col_v) : 0;
        // ---- column results: two smallest of the 4 x 2 group minima of every query, and the groups
        // whose minimum is <= the second smallest (bit k + 4 g: tiles with (tile & 3) == k, lane half g):
        // the only train rows that can be the query's best or second (narrow exact stage).  The masks of
        // a lane's QW queries travel as ONE word (4 bits each: one lane exchange, one store for QW = 8).
        if (wave_valid) {
            unsigned ownpack = 0;
            int v1s[QW], v2s[QW];
#pragma unroll
            for (int qb = 0; qb < QW; ++qb) {
                const int lo01 = min(m[qb][0], m[qb][1]), hi01 = max(m[qb][0], m[qb][1]);
                const int lo23 = min(m[qb][2], m[qb][3]), hi23 = max(m[qb][2], m[qb][3]);
                const int a1 = min(lo01, lo23), a2 = min(max(lo01, lo23), min(hi01, hi23));
                const int b1 = __shfl_xor(a1, 32), b2 = __shfl_xor(a2, 32);
                const int v1 = min(a1, b1), v2 = min(max(a1, b1), min(a2, b2));
                v1s[qb] = v1;
                v2s[qb] = v2;
#if !defined(IAMX_T_NOMASK)
                const unsigned own = (m[qb][0] <= v2 ? 1u : 0u) | (m[qb][1] <= v2 ? 2u : 0u) |
                                     (m[qb][2] <= v2 ? 4u : 0u) | (m[qb][3] <= v2 ? 8u : 0u);
                ownpack |= own << (4 * qb);
#endif
            }
            const unsigned othpack = A.colmask ? (unsigned)__shfl_xor((int)ownpack, 32) : 0u;
            const int row0 = q0 + QW * rc;
            if (g == 0) {
#pragma unroll
                for (int qb = 0; qb < QW; ++qb)
                    if (row0 + qb < nb)
                        *reinterpret_cast<v2i *>(A.col + 2 * ((ITEMS ? col_u : A.col_off[u]) + row0 + qb)) = v2i{v1s[qb], v2s[qb]};
                if (A.colmask) {
                    // byte qb = own nibble | other half's nibble << 4
                    uint8_t *dst = A.colmask + (ITEMS ? col_u : A.col_off[u]) + row0;
                    if (QW == 8 && row0 + QW <= nb) {
                        auto spread = [](unsigned nib4) {    // four nibbles -> the low nibbles of four bytes
                            const unsigned x = (nib4 | (nib4 << 8)) & 0x00FF00FFu;
                            return (x | (x << 4)) & 0x0F0F0F0Fu;
                        };
                        const unsigned lo = spread(ownpack & 0xFFFFu) | (spread(othpack & 0xFFFFu) << 4);
                        const unsigned hi = spread(ownpack >> 16) | (spread(othpack >> 16) << 4);
                        *reinterpret_cast<v2u *>(dst) = v2u{lo, hi};
                    } else {
#pragma unroll
                        for (int qb = 0; qb < QW; ++qb)
                            if (row0 + qb < nb)
                                dst[qb] = (uint8_t)(((ownpack >> (4 * qb)) & 15u) | (((othpack >> (4 * qb)) & 15u) << 4));
                    }
                }
            }
        }
        if constexpr (!ITEMS) break;
        else if (++u == uniform32(u_end)) break;
    }
}

// ---------------------------------------------------------------------------------
// Form 2's item sweep on v_mfma_i32_16x16x64_i8 (round 17): the same workgroup (four waves, one
// per SIMD, a 1024-row B slice in the AGPR half, A streamed in 128-row chunks through the same
// stage and swizzle), the same item walk, merge and outputs, bit for bit -- on the MFMA shape the
// chip clocks higher (profiles/r17_ubench_mfma_clock.txt).  Two chained MFMAs (K = 2 x 64) make a
// 16 x 16 tile with Ct as the C operand; 256 MFMAs a chunk and wave.
//   Lane (n = lane & 15, lg = lane >> 4) holds bytes [64 s + 16 lg, +16) of the 16 CONSECUTIVE
//   sorted B rows q0 + 16 rn + block, rn = n's bit 3 moved to the bottom: lanes n and n ^ 8 hold
//   a group of 32 consecutive rows (form 2's groups, so R_w and S_w are form 2's).  An accumulator
//   is query n against train rows 4 lg + i of the tile.
//   Row direction: the v_min3 chain over the 16 blocks is lane local (4 registers a tile); the
//   minimum over the 16 lanes n, with the group floors, goes through LDS (below; until round 21 a
//   transposing butterfly over the DPP row, 16 VALU instructions a tile).
//   Column direction: running minima per block and (tile32 & 3); train row bit 2 is lg & 1, so
//   lane groups lg and lg ^ 2 are merged at the pair's end into form 2's eight groups (k, g).
// The chunk loop is a compiler-scheduled software pipeline: 32 steps of 8 MFMAs (four blocks),
// step s issues the MFMAs of step s + 1 beside the minima of step s, PIPE valu instructions a gap.
//   Row direction, across lanes (round 21): through LDS, which the loop leaves three quarters idle,
//   instead of a butterfly on the vector issue slots that bound it.  A lane stores the four raw
//   registers of a tile with one ds_write_b128 into its wave's area ([tile][lg][n], a combo (tile, lg)
//   every SWEEP16_RAW_COMBO bytes); the wave reads its own chunk back while the next chunk runs (no
//   barrier: a wave's LDS operations complete in order).  Reader lane l takes combo l >> 1 and the four
//   groups {n, n ^ 8} with (n & 7) = 2 j + (l & 1): 8 ds_read_b128, the pair minimum and the floor of
//   every group, the minimum over its groups, one quad_perm minimum with lane l ^ 1, and the even lane
//   stores the combo's four consecutive rows of R_w with one ds_write_b128.
//   The combo stride of 288 bytes (18 slots of 16 bytes) puts the 16 lanes of each ds_read_b128 lane
//   group -- combos {0,1,6,7,10..13} or {2..5,8,9,14,15} (+ 16), both halves -- on 16 different slots
//   of the 256-byte bank row; a writer's 8 contiguous lanes store 128 contiguous bytes.
// ---------------------------------------------------------------------------------
// valu instructions behind MFMA `g` (0..7) of a step of the 16x16x64 chunk loop that has `nv` of them
constexpr int sweep16_gap_valu(int nv, int g) { return nv / 8 + (g < nv % 8 ? 1 : 0); }

// the 16x16x64 item kernel's LDS (dynamic: over the 64 KB of a static array): form 2's layout -- two
// stages, Ct, three R_w buffers, S_w, the dump area -- and behind it the waves' raw row minima, two
// chunks each (the next chunk's writes begin while the reader runs)
constexpr int SWEEP16_RAW_COMBO = 256 + 32;
constexpr int SWEEP16_RAW_CHUNK = (CHUNK / 16) * 4 * SWEEP16_RAW_COMBO;
constexpr int SWEEP16_LDS_FORM2 = 2 * CHUNK * D + 2 * CHUNK * 4 + 3 * 4 * CHUNK * 4 + 2 * 4 * 4 + (2 * 4 * CHUNK + 4 * 256) * 4;
constexpr int SWEEP16_LDS_BYTES = SWEEP16_LDS_FORM2 + 4 * 2 * SWEEP16_RAW_CHUNK;
static_assert(SWEEP16_LDS_FORM2 % 16 == 0 && SWEEP16_LDS_BYTES <= 160 * 1024, "aligned, and inside a compute unit's LDS");

template <int PIPE>
__global__ __launch_bounds__(256, 1) void knn2sym16_kernel(SymArgs A)
{
    constexpr int NW = 4, QB = 16, WGROWS = NW * QB * 16, NT = NW * 64;
    constexpr int PIECES = CHUNK * D / 16 / NT;
    constexpr int NT16 = CHUNK / 16, SPT = 4, QS = QB / SPT, NS = NT16 * SPT;    // tiles, steps a tile, blocks a step
    static_assert(WGROWS == 1024 && PIECES == 4 && NS == 32 && D == 128, "form 2's workgroup");
    extern __shared__ __attribute__((aligned(16))) int8_t lds[];     // SWEEP16_LDS_BYTES
    int8_t *lds_tile = lds;
    int *lds_tb = reinterpret_cast<int *>(lds + 2 * CHUNK * D);      // [2][CHUNK]     Ct
    int *lds_row = lds_tb + 2 * CHUNK;                               // [3][NW][CHUNK] R_w
    int *lds_cq = lds_row + 3 * NW * CHUNK;                          // [NW] (2 NW reserved) S_w
    int *lds_dump = lds_cq + 2 * NW;                                 // [NW][256] (+ 2 buffer strides) unused stores
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, lg = lane >> 4;
    const int rn = ((n & 7) << 1) | (n >> 3);
#if defined(IAMX_T_STAMPS)
    const unsigned long long stamp_entry = __builtin_amdgcn_s_memtime();
#endif

    int vid;
    {
        const int total = A.total_wg, bid = blockIdx.x;
        const int xcd = bid & 7, k = bid >> 3, q = total >> 3, r = total & 7;
        vid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
    }
    int u = A.wg_off[3 * vid], u_end = u + A.wg_off[3 * vid + 1], item_wgi = A.wg_off[3 * vid + 2];
    v4i bq[QB][2];
    int fl[4];                       // the Cq floors of the four groups (n & 7) = 2 j + (lane & 1) this lane reads back
    int bimg_held = -1;              // the B image whose slice bq holds
    asm volatile("" : "+v"(u_end), "+v"(item_wgi), "+v"(bimg_held));
    // a lane's place in its wave's raw row minima: as the writer (n, lg) of a tile, as the reader of combo lane >> 1
    const int raw_wave = SWEEP16_LDS_FORM2 + wave * (2 * SWEEP16_RAW_CHUNK);
    const int raw_wr = raw_wave + lg * SWEEP16_RAW_COMBO + n * 16;
    const int raw_rd = raw_wave + (lane >> 1) * SWEEP16_RAW_COMBO + (lane & 1) * 16;
#if defined(IAMX_T_STAMPS)
    // (the diagnostic build stamps this kernel's whole chunk loop -- chunks, cycles, 100 MHz ticks -- and the
    //  pair tail: the cycles from the end of a pair's chunk loop to the start of the item's next pair's, which
    //  cover the last merge, the column epilogue, the barrier, the first two stages and the first operand reads;
    //  and the ITEM START: the cycles from the kernel's entry to the start of the first pair's chunk loop -- the
    //  table chain, the B slice, the first two stages --, stored behind the [workgroups][waves][4] block)
    unsigned long long stamp_chunks = 0, stamp_cycles = 0, stamp_ticks = 0, stamp_tail = 0, stamp_c1 = 0, stamp_start = 0;
#endif
    // the table entries of the pair the loop runs next, read one pair ahead (see knn2sym_kernel)
    int nx_b = A.upairs[2 * u], nx_a = A.upairs[2 * u + 1];
    int nx_boff = A.img_off[nx_b], nx_nb = A.img_n[nx_b], nx_aoff = A.img_off[nx_a], nx_na = A.img_n[nx_a];
    int64_t nx_rowp = A.rowp_off[u];
    for (;;) {
        const int bimg = uniform32(nx_b);
        const int boff = uniform32(nx_boff), nb = uniform32(nx_nb);
        const int aoff = uniform32(nx_aoff), na = uniform32(nx_na);
        const int capA = (na + CHUNK - 1) / CHUNK * CHUNK;
        const int nchunks = capA / CHUNK;
        const int wgi = uniform32(item_wgi);
        const int q0 = wgi * WGROWS + wave * (QB * 16);
        const bool wave_valid = q0 < nb;
        const int64_t rbase = uniform64(nx_rowp) + (int64_t)wgi * capA;
        // (from the item's second pair on: every wave is past the previous pair's last merge -- its
        //  lds_row reads -- before an invalid wave refills its rows with BIG below)
        if (uniform32(bimg_held) >= 0) __syncthreads();

        const int8_t *tbase = A.sdesc + (int64_t)aoff * D;
        const int32_t *tci = A.sct + aoff;
        // global -> LDS directly; the XOR swizzle of the 16-byte slots is applied on the source side
        typedef __attribute__((address_space(3))) void *lds_ptr;
        // (one lane offset for every piece and chunk beside a scalar base, the wave's LDS destination from a
        //  scalar register: piece j holds rows 32 j + (tid >> 3), slot (tid & 7) ^ ((row >> 1) & 7))
        const int wave_u = uniform32(wave);
        const unsigned stage_voff = (unsigned)((tid >> 3) * D + (((tid & 7) ^ ((tid >> 4) & 7)) * 16));
        const unsigned lds_tile_at = (unsigned)(uintptr_t)(lds_ptr)(lds_tile + wave_u * (64 * 16));
        const unsigned lds_tb_at = (unsigned)(uintptr_t)(lds_ptr)(lds_tb + (wave_u & (CHUNK / 64 - 1)) * 64);
        const unsigned ct_voff = (unsigned)((tid & (CHUNK - 1)) * 4);
        // chunk `ch` into stage buffer `buf`: all 256 threads, five loads a lane
        auto stage_direct = [&](int ch, int buf) {
            const int8_t *const src = tbase + (int64_t)ch * (CHUNK * D) + stage_voff;
#pragma unroll
            for (int j = 0; j < PIECES; ++j)
                stage_piece<16>(src + j * ((NT / 8) * D), lds_tile_at + buf * (CHUNK * D) + j * NT * 16);
            stage_piece<4>(reinterpret_cast<const int8_t *>(tci + ch * CHUNK) + ct_voff, lds_tb_at + buf * (CHUNK * 4));
        };
        auto wait_direct = [&]() { __builtin_amdgcn_s_waitcnt(0x0F70); };       // vmcnt(0)
        // chunks 0 and 1 of the pair, as soon as its A image is known and in front of the B slice's loads: one
        // round trip for the stage, the squared norms and the slice where B changes (the wait and the barrier
        // in front of the first operand reads are below; every wave is past its reads of both stage buffers)
        stage_direct(0, 0);
        stage_direct(nchunks > 1 ? 1 : 0, 1);

        // B operand: rows past the end repeat the last row; the Cq floor of a lane's group of 32 rows
        // and the wave's largest spread S_w as in knn2sym_kernel
        if (bimg != uniform32(bimg_held)) {
            bimg_held = bimg;
            // the squared norms the spread and the floors are made of: loaded in front of the slice, with it
            // and not behind its wait (a wave past the end reads the image's last row and uses nothing of it)
            int sn_lo, sn_hi, sn_fl[4];
            {
                const int g_lo = rn & ~1, g_hi = rn | 1;
                const int r_lo = q0 + QB * g_lo < nb ? q0 + QB * g_lo : nb - 1;
                const int r_hi = q0 + QB * g_hi + QB - 1 < nb ? q0 + QB * g_hi + QB - 1 : nb - 1;
                sn_hi = A.sn2[boff + r_hi];
                sn_lo = A.sn2[boff + r_lo];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int r_fl = q0 + 2 * QB * (2 * j + (lane & 1));
                    sn_fl[j] = A.sn2[boff + (r_fl < nb ? r_fl : nb - 1)];
                }
            }
            // (all 32 loads of a lane are issued before the first is waited for: the registers they land in are
            //  free here, the column minima are not live yet; a wait behind every load made them 32 round trips)
            v4i braw[QB][2];
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
                int row = q0 + QB * rn + qb;
                row = row < nb ? row : nb - 1;
                const v4i *src = reinterpret_cast<const v4i *>(A.sdesc + (int64_t)(boff + row) * D);
#pragma unroll
                for (int s = 0; s < 2; ++s) braw[qb][s] = src[4 * s + lg];
            }
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    bq[qb][s] = ~braw[qb][s];
                    asm volatile("" : "+a"(bq[qb][s]));      // (only ever an MFMA source: the AGPR half)
                }
            }
            {
                int spread = wave_valid ? (sn_hi >> 1) - (sn_lo >> 1) : 0;
#pragma unroll
                for (int sh = 32; sh >= 1; sh >>= 1) spread = max(spread, __shfl_xor(spread, sh));
                if (lane == 0) lds_cq[wave] = spread;
            }
            // (group (n & 7) holds rows q0 + 32 (n & 7) ..: the floor its two lanes n, n ^ 8 share)
#pragma unroll
            for (int j = 0; j < 4; ++j) fl[j] = wave_valid ? sn_fl[j] >> 1 : 0;
        }
        if (!wave_valid) {
#pragma unroll
            for (int k = 0; k < 3 * CHUNK / 64; ++k)
                lds_row[((k / (CHUNK / 64)) * NW + wave) * CHUNK + (k % (CHUNK / 64)) * 64 + lane] = BIG;
        }
        int m[QB][4];
#pragma unroll
        for (int qb = 0; qb < QB; ++qb)
#pragma unroll
            for (int k = 0; k < 4; ++k) m[qb][k] = BIG;

        // per train row: the waves' group minima -> (L, U1, U2), stored by waves 0 and 1 through a buffer
        // resource over this workgroup's partials (an offset past num_records drops the store)
        const int mrow = (wave & 1) * 64 + lane;
        const bool merger = wave < 2;
        constexpr int RSRC_WORD3_DATA_FORMAT_32 = 4 << 15;
        constexpr int RANGE_DROP = 0x7FFFFFF0;
        const __amdgpu_buffer_rsrc_t rowp_rsrc =
            __builtin_amdgcn_make_buffer_rsrc(A.rowp + 2 * rbase, (short)0, capA * 8, RSRC_WORD3_DATA_FORMAT_32);
        int spread_w[NW];
        auto merge_rows = [&](int ch, int rbo, bool store) {
            int L = BIG, U1 = BIG, U2 = BIG;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const int R = lds_row[rbo + w * CHUNK + mrow];
                const int uw = R + spread_w[w];
                L = min(L, R);
                U2 = min(max(U1, uw), U2);
                U1 = min(U1, uw);
            }
            __builtin_amdgcn_raw_buffer_store_b64(v2i{L, pack_row_bounds(L, U1, U2)}, rowp_rsrc,
                                                  store ? (ch * CHUNK + mrow) * 8 : RANGE_DROP, 0, 0);
        };

        // the reader's even lanes hold train rows 4 c .. 4 c + 3 of the chunk, c = lane >> 1, and store them;
        // the odd lanes, and a wave past the end of the B image (its rows of R_w stay BIG), store into the dump
        // area: one ds_write_b128 a chunk.  A predicated store would be a branch in step RSTORE, and a step is
        // one scheduling region (its sched_group_barrier deal ends at a block boundary), so the dump area stays
        int *const row_dst = (lane & 1) == 0 && wave_valid
            ? lds_row + wave * CHUNK + 4 * (lane >> 1)
            : lds_dump + wave * 256 + 4 * lane;             // (+ row buffer offset: inside the dump area)
        typedef __attribute__((address_space(3))) int8_t *lds_wbytes;
        typedef __attribute__((address_space(3))) v4i *lds_v4i;
        // the raw row minima of tile `tile`, into the wave's chunk at byte offset `at` (raw_wr + the buffer)
        auto raw_write = [&](int at, int tile, const int (&rr)[4]) {
            *reinterpret_cast<lds_v4i>((lds_wbytes)lds + at + tile * (4 * SWEEP16_RAW_COMBO)) = v4i{rr[0], rr[1], rr[2], rr[3]};
        };
        // the reader's group j of the chunk at `at` (raw_rd + the buffer): its two lanes' registers, then
        // their minimum above the group's floor
        auto raw_read = [&](int at, int j, v4i (&v)[2]) {
#pragma unroll
            for (int hi = 0; hi < 2; ++hi)
                v[hi] = *reinterpret_cast<lds_v4i>((lds_wbytes)lds + at + j * 32 + hi * 128);
        };
        auto raw_group = [&](int j, const v4i (&v)[2], int (&x)[4]) {
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = min(v[0][i], v[1][i]) + fl[j];
        };
        // the other half of the combo's groups sits in lane ^ 1
        auto raw_store = [&](int rbo_at, int (&x)[4]) {
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = min(x[i], __builtin_amdgcn_update_dpp(0, x[i], 0xB1, 0xF, 0xF, true));   // quad_perm:[1,0,3,2]
            *reinterpret_cast<v4i *>(row_dst + rbo_at) = v4i{x[0], x[1], x[2], x[3]};
        };
        v4i aop[2][2], ct[2];
        v4i accs[2][QS];
        int r[2][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[1][k] = BIG;

        {                                  // (the last pair of the item reads its own entries again)
            const int un = u + 1 < u_end ? u + 1 : u;
            nx_b = A.upairs[2 * un];
            nx_a = A.upairs[2 * un + 1];
            nx_rowp = A.rowp_off[un];
        }
        wait_direct();
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NW; ++w) spread_w[w] = __builtin_amdgcn_readfirstlane(lds_cq[w]);
        {
            const int b = uniform32(nx_b), a = uniform32(nx_a);
            nx_boff = A.img_off[b];
            nx_nb = A.img_n[b];
            nx_aoff = A.img_off[a];
            nx_na = A.img_n[a];
        }
        // a lane's LDS offsets in the stage buffer the operand reads go to, switched by one xor each where
        // the reads move on to the next chunk's buffer; the tile rides in the instruction's offset.  Row
        // 16 T + n sits at slot (4 s + lg) ^ ((n >> 1) & 7): the 16 lanes of a group read 16 different
        // 16-byte slots of a 256-byte line pair (rows n, n ^ 1 share a slot index, 128 bytes apart)
        typedef __attribute__((address_space(3))) const int8_t *lds_bytes;
        int opoff[2], tboff = 2 * CHUNK * D + 16 * lg;
#pragma unroll
        for (int s = 0; s < 2; ++s) opoff[s] = n * D + (((4 * s + lg) ^ ((n >> 1) & 7)) * 16);
        auto load_ops = [&](int tile, v4i (&a)[2], v4i &c) {
            c = *reinterpret_cast<const __attribute__((address_space(3))) v4i *>((lds_bytes)lds + tboff + tile * 64);
#pragma unroll
            for (int s = 0; s < 2; ++s)
                a[s] = *reinterpret_cast<const __attribute__((address_space(3))) v4i *>((lds_bytes)lds + opoff[s] + tile * (16 * D));
        };
        // the MFMAs of a step: blocks qp .. qp + 3 of tile parity tp, the four chains interleaved
        auto issue = [&](auto tp_c, auto qp_c, v4i (&acc)[QS]) {
            constexpr int tp = decltype(tp_c)::value, qp = decltype(qp_c)::value;
#pragma unroll
            for (int j = 0; j < QS; ++j) acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aop[tp][0], bq[qp + j][0], ct[tp], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < QS; ++j) acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aop[tp][1], bq[qp + j][1], acc[j], 0, 0, 0);
        };
        load_ops(0, aop[0], ct[0]);
        load_ops(1, aop[1], ct[1]);
        issue(int_c<0>{}, int_c<0>{}, accs[0]);
        __builtin_amdgcn_sched_barrier(0);
        // row buffers (offsets in ints) of this chunk and of the previous one; "chunk -1" stores its
        // (meaningless) last tile into the buffer chunk 2 overwrites
        int rbo = 0, rbo_prev = 2 * NW * CHUNK;
        // (the stage inside the chunk loop, as in form 2's: the same offsets, one held piece a step)
#if defined(IAMX_T_STAMPS)
        const unsigned long long loop_c0 = __builtin_amdgcn_s_memtime(), loop_r0 = __builtin_amdgcn_s_memrealtime();
        __builtin_amdgcn_s_waitcnt(0xC07F);              // lgkmcnt(0) alone
        if (stamp_c1) stamp_tail += loop_c0 - stamp_c1;
        else stamp_start = loop_c0 - stamp_entry;
#endif
        // a chunk.  STAGE: chunk + 2 of the pair exists and is staged; the pair's last two chunks stage nothing
        auto chunk = [&](int ch, auto stage_c) __attribute__((always_inline)) {
            constexpr bool STAGE = decltype(stage_c)::value != 0;
            const int buf = ch & 1;
            // the barrier step: every read of this chunk's stage has been issued (tile NT16 - 1's in the step
            // in front of it), the next chunk's stage has landed; the stage of chunk + 2 follows it, one piece
            // a step held between two column minima, and the merge of the previous chunk in three steps
            constexpr int BAR = (NT16 - 2) * SPT;
            static_assert(BAR + PIECES < NS, "the stage's five pieces fit behind the barrier");
            const int8_t *const sg_tile = tbase + (int64_t)(ch + 2) * (CHUNK * D);
            const int8_t *const sg_ct = reinterpret_cast<const int8_t *>(tci + (ch + 2) * CHUNK);
            // the raw row minima: this chunk's tiles go to buffer `buf`, the previous chunk's last tile and the
            // reader to the other one
            const int raw_cur = buf * SWEEP16_RAW_CHUNK, raw_prev = SWEEP16_RAW_CHUNK - raw_cur;
            const int wr_cur = raw_wr + raw_cur, wr_prev = raw_wr + raw_prev, rd_prev = raw_rd + raw_prev;
            int mR[NW], mL = BIG, mU1 = BIG, mU2 = BIG;
            constexpr int RSTORE = 4 * SPT + 1;                  // the step of the reader's row store
            static_assert(RSTORE < BAR, "the rows are stored in front of the barrier");
            v4i rdv[2];
            int racc[4], rx[4], rh[4];
            static_for<0, NS>([&](auto st_c) {
                constexpr int st = decltype(st_c)::value;
                constexpr int t = st / SPT, ph = st % SPT, qp = QS * ph, cur = st & 1, kk = (t >> 1) & 3;
                constexpr int nst = st + 1 < NS ? st + 1 : 0;
                constexpr bool staging = STAGE && st >= BAR && st <= BAR + PIECES;
                if constexpr (st == BAR) {
                    __builtin_amdgcn_s_waitcnt(0x0070);              // vmcnt(0) lgkmcnt(0)
                    __syncthreads();
                }
                issue(int_c<(nst / SPT) & 1>{}, int_c<QS * (nst % SPT)>{}, accs[cur ^ 1]);
                // minima of this step, oldest accumulator first: the column minima of its four blocks (two a
                // block), then the row chain
#pragma unroll
                for (int j = 0; j < QS; ++j) {
                    const v4i &a = accs[cur][j];
                    int &mm = m[qp + j][kk];
                    mm = min(min(mm, a[0]), a[1]);
                    if constexpr (staging) {
                        if (j == 1) {
                            if constexpr (st < BAR + PIECES)
                                stage_piece_held<16>(sg_tile + (st - BAR) * ((NT / 8) * D) + stage_voff,
                                                     lds_tile_at + buf * (CHUNK * D) + (st - BAR) * NT * 16, mm);
                            else
                                stage_piece_held<4>(sg_ct + ct_voff, lds_tb_at + buf * (CHUNK * 4), mm);
                        }
                    }
                    mm = min(min(mm, a[2]), a[3]);
                }
                const v4i a0 = accs[cur][0], a1 = accs[cur][1], a2 = accs[cur][2], a3 = accs[cur][3];
                int (&rc_)[4] = r[t & 1];
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    rc_[i] = ph == 0 ? min(min(min(a0[i], a1[i]), a2[i]), a3[i])
                                     : min(min(min(min(rc_[i], a0[i]), a1[i]), a2[i]), a3[i]);
                // the previous tile's raw row minima (tile NT16 - 1 of the previous chunk for t = 0)
                if constexpr (ph == 0) raw_write(t > 0 ? wr_cur : wr_prev, t > 0 ? t - 1 : NT16 - 1, r[(t + 1) & 1]);
                // the reader of the previous chunk: group j's reads behind tile j's write, its minima two steps
                // on, the rows stored well in front of the barrier their merge reads behind
                if constexpr (ph == 0 && t < 4) raw_read(rd_prev, t, rdv);
                if constexpr (ph == 2 && t < 4) {
                    if constexpr (t == 0) raw_group(0, rdv, racc);
                    else raw_group(t, rdv, rx);
                    if constexpr (t == 1) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) racc[i] = min(racc[i], rx[i]);
                    }
                    if constexpr (t == 2) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) rh[i] = rx[i];
                    }
                    if constexpr (t == 3) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) racc[i] = min(min(racc[i], rh[i]), rx[i]);
                    }
                }
                if constexpr (st == RSTORE) raw_store(rbo_prev, racc);
                // the operand reads of tile t + 2 (flattened across chunks), behind the last MFMAs of tile t;
                // from tile NT16 on they read the next chunk's stage
                if constexpr (ph == SPT - 1) {
                    if constexpr (t + 2 == NT16) {
#pragma unroll
                        for (int s = 0; s < 2; ++s) opoff[s] ^= CHUNK * D;
                        tboff ^= CHUNK * 4;
                    }
                    load_ops((t + 2) % NT16, aop[t & 1], ct[t & 1]);
                }
                // the merge of the previous chunk (its rows' last minima were stored in this chunk's first tile)
                if constexpr (st == BAR + 1) {
#pragma unroll
                    for (int w = 0; w < NW; ++w) mR[w] = lds_row[rbo_prev + w * CHUNK + mrow];
                }
                if constexpr (st == BAR + 2) {
#pragma unroll
                    for (int w = 0; w < NW; ++w) {
                        const int uw = mR[w] + spread_w[w];
                        mL = min(mL, mR[w]);
                        mU2 = min(max(mU1, uw), mU2);
                        mU1 = min(mU1, uw);
                    }
                    // (no instruction: it keeps the eleven minima above in this step.  With the chunk instantiated
                    //  twice the compiler otherwise forms them where step BAR + 3's store reads them -- one gap of 23
                    //  and three empty gaps, against tests/test_sweep16_gaps.py's largest gap <= 11 and <= 2 empty
                    //  gaps.  If a change of the `nv` deal makes it unnecessary, that test passes without it.)
                    asm volatile("" : "+v"(mL), "+v"(mU1), "+v"(mU2));
                }
                if constexpr (st == BAR + 3)
                    __builtin_amdgcn_raw_buffer_store_b64(v2i{mL, pack_row_bounds(mL, mU1, mU2)}, rowp_rsrc,
                                                          merger && ch > 0 ? ((ch - 1) * CHUNK + mrow) * 8 : RANGE_DROP, 0, 0);
                // 16 minima a step, the reader's piece, the chunk's own work: spread evenly over the eight gaps
                constexpr int nv = 16 + (ph == 2 && t < 4 ? (t & 1 ? 12 : 8) : 0) + (st == RSTORE ? 4 : 0) + (st == 0 ? 3 : 0) +
                                   (staging ? 2 : 0) + (st == BAR + 2 ? 11 : 0) + (st == BAR + 3 ? 5 : 0) +
                                   (st == NS - 1 ? 2 : 0) + (PIPE - 2);
                static_for<0, 8>([&](auto g_c) {
                    constexpr int g = decltype(g_c)::value;
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, sweep16_gap_valu(nv, g) + (g == 7 ? 3 : 0), 0);
                });
                __builtin_amdgcn_sched_barrier(0);
            });
            rbo_prev = rbo;
            rbo = rbo == 2 * NW * CHUNK ? 0 : rbo + NW * CHUNK;
        };
        int ch = 0;
        for (; ch + 2 < nchunks; ++ch) chunk(ch, int_c<1>{});
        for (; ch < nchunks; ++ch) chunk(ch, int_c<0>{});
#if defined(IAMX_T_STAMPS)
        {
            unsigned long long loop_c1;
            SWEEP_STAMP(loop_c1);
            stamp_cycles += loop_c1 - loop_c0;
            stamp_ticks += __builtin_amdgcn_s_memrealtime() - loop_r0;
            stamp_chunks += (unsigned)nchunks;
            stamp_c1 = loop_c1;
            if (A.stamps && lane == 0) {
                unsigned long long *o = A.stamps + ((size_t)blockIdx.x * NW + wave) * 4;
                o[0] = stamp_tail;
                o[1] = stamp_chunks;
                o[2] = stamp_cycles;
                o[3] = stamp_ticks;
                A.stamps[(size_t)gridDim.x * NW * 4 + (size_t)blockIdx.x * NW + wave] = stamp_start;
            }
        }
#endif
        // this pair's first column-result row (it lands with the vmcnt(0) below)
        const int64_t col_v = A.col_off[u];
        // the last chunk's last tile, its reader, its merge
        {
            const int last = ((nchunks - 1) & 1) * SWEEP16_RAW_CHUNK;
            raw_write(raw_wr + last, NT16 - 1, r[(NT16 - 1) & 1]);
            v4i v[4][2];
            int x[4][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) raw_read(raw_rd + last, j, v[j]);
#pragma unroll
            for (int j = 0; j < 4; ++j) raw_group(j, v[j], x[j]);
#pragma unroll
            for (int i = 0; i < 4; ++i) x[0][i] = min(min(x[0][i], x[1][i]), min(x[2][i], x[3][i]));
            raw_store(rbo_prev, x[0]);
        }
        wait_direct();
        __syncthreads();
        merge_rows(nchunks - 1, rbo_prev, merger);

        const int64_t col_u = uniform64(col_v);
        // ---- column results: lane groups lg and lg ^ 2 hold the same group g = lg & 1 of train rows; merged,
        // a lane has form 2's 4 x 2 group minima of its 16 queries: the two smallest, and the groups whose
        // minimum is <= the second smallest (bit k + 4 g), 4 bits a query
        // Both exchanges are swaps on the VALU (no LDS).  v_permlane32_swap on the registers of blocks j and
        // j + 8 and one minimum leave block j + 8 h merged in half h = lane >> 5; of a lane's two smallest,
        // v_permlane16_swap on the registers of blocks p and p + 4 leaves both sides of block p + 4 c in the
        // DPP rows of parity c = lg & 1.  So lane (n, lg) ends with (v1, v2) of the FOUR CONSECUTIVE queries
        // 16 rn + 4 lg + p, and every lane stores.
        if (wave_valid) {
            int mk[QB / 2][4], a1[QB / 2], a2[QB / 2];
#pragma unroll
            for (int j = 0; j < QB / 2; ++j) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const v2u x = __builtin_amdgcn_permlane32_swap((unsigned)m[j][k], (unsigned)m[j + QB / 2][k], false, false);
                    mk[j][k] = min((int)x[0], (int)x[1]);
                }
                const int lo01 = min(mk[j][0], mk[j][1]), hi01 = max(mk[j][0], mk[j][1]);
                const int lo23 = min(mk[j][2], mk[j][3]), hi23 = max(mk[j][2], mk[j][3]);
                a1[j] = min(lo01, lo23);
                a2[j] = min(max(lo01, lo23), min(hi01, hi23));
            }
            int v1s[4], v2s[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                // ([0]: the even row's side of its block p in the even rows, of the odd rows' block p + 4 in the odd rows)
                const v2u x1 = __builtin_amdgcn_permlane16_swap((unsigned)a1[p], (unsigned)a1[p + 4], false, false);
                const v2u x2 = __builtin_amdgcn_permlane16_swap((unsigned)a2[p], (unsigned)a2[p + 4], false, false);
                v1s[p] = min((int)x1[0], (int)x1[1]);
                v2s[p] = min(max((int)x1[0], (int)x1[1]), min((int)x2[0], (int)x2[1]));
            }
            const int row0 = q0 + QB * rn + 4 * lg;
            unsigned maskw = 0;          // byte p = the nibble of group half 0 | the nibble of group half 1 << 4
            if (A.colmask) {
                // the second smallest of block j in every row: the even rows' v2s[p] is block p's, the odd rows' block p + 4's
                unsigned ownpack = 0;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const v2u w = __builtin_amdgcn_permlane16_swap((unsigned)v2s[p], (unsigned)v2s[p], false, false);
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const int j = p + 4 * c, v2 = (int)w[c];
                        const unsigned own = (mk[j][0] <= v2 ? 1u : 0u) | (mk[j][1] <= v2 ? 2u : 0u) |
                                             (mk[j][2] <= v2 ? 4u : 0u) | (mk[j][3] <= v2 ? 8u : 0u);
                        ownpack |= own << (4 * j);
                    }
                }
                // ([0]: the even rows' words, group half 0, in both rows; [1]: the odd rows')
                const v2u g = __builtin_amdgcn_permlane16_swap(ownpack, ownpack, false, false);
                auto spread = [](unsigned nib4) {    // four nibbles -> the low nibbles of four bytes
                    const unsigned x = (nib4 | (nib4 << 8)) & 0x00FF00FFu;
                    return (x | (x << 4)) & 0x0F0F0F0Fu;
                };
                const int sh = 16 * (lg & 1);
                maskw = spread((g[0] >> sh) & 0xFFFFu) | (spread((g[1] >> sh) & 0xFFFFu) << 4);
            }
            int32_t *const cdst = A.col + 2 * (col_u + row0);
            if (row0 + 4 <= nb) {
                *reinterpret_cast<v4i *>(cdst) = v4i{v1s[0], v2s[0], v1s[1], v2s[1]};
                *reinterpret_cast<v4i *>(cdst + 4) = v4i{v1s[2], v2s[2], v1s[3], v2s[3]};
                if (A.colmask) *reinterpret_cast<unsigned *>(A.colmask + col_u + row0) = maskw;
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    if (row0 + p < nb) {
                        *reinterpret_cast<v2i *>(cdst + 2 * p) = v2i{v1s[p], v2s[p]};
                        if (A.colmask) A.colmask[col_u + row0 + p] = (uint8_t)(maskw >> (8 * p));
                    }
            }
        }
        if (++u == uniform32(u_end)) break;
    }
}

// ---------------------------------------------------------------------------------
// candidates.  Pass 1 (symcand_rows_kernel, one thread per query row) visits the rows in SORTED
// order (the order the sweep wrote its bounds in: coalesced reads) and drops a flag at the row's
// original position; pass 2 (symcand_kernel, one workgroup per ORDERED pair) lists the flagged rows
// in ascending original order at the pair's own slice of cand_q (first entry out_off[p]: a pair
// cannot have more candidates than rows, so no scan over the pairs is needed) and appends the
// pair's tasks to the exact stage's lists (pass 1 ran inside the per-pair workgroups until round 6:
// 21 MB of row bounds per pair of 37 k-row images through ONE workgroup).
// ---------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------
// NARROW exact stage (round 6).  The sweep already knows WHERE a candidate's two smallest
// distances can be: a query that was a B row has eight group minima over the streamed image
// (group = (tile & 3, lane half): `colmask` says which are <= v2), a query that was an A row has one
// (L, U1, U2) per 1024-row block of the register-resident image (`rowp`: block w can hold a row
// at or below the upper bound of the second distance only if L_w <= U2).  Every other train row is
// farther than the candidate's exact second distance.  So a candidate becomes ITEMS (candidate,
// class), the items of an ordered pair are bucketed by class, and a task scans ONE class -- 1/8 of
// the train image for the column direction, 1/nwg for the row direction -- for up to 256 items.
// Each item leaves (best, row, second) of its class; a finish pass merges a candidate's items.
// Results are those of the full scan: every row that can be the best, the second or tied with
// either lies in a class of the candidate's mask ("narrow exact stage").
//
// One device buffer `nar` (iamx_knn2sym_narrow_bytes), carved up by narrow_layout() below.
// ---------------------------------------------------------------------------------
struct NarTask { int p, cls, item0, n; };
struct NarLayout {
    int64_t ctl, pair_base, mask, slot, items, res, tasks, total;
    int64_t item_cap, task_cap;
};
// ctl[0] narrow tasks, ctl[1] items allocated, ctl[2] tasks taken (zero on entry, reset by the finish kernel)
__host__ __device__ inline NarLayout narrow_layout(int64_t rows, int64_t n_pairs)
{
    NarLayout L;
    auto up = [](int64_t v) { return (v + 255) / 256 * 256; };
    L.item_cap = rows;
    L.task_cap = rows / 64 + 80 * n_pairs + 64;
    int64_t o = 0;
    L.ctl = o;        o += 256;
    L.pair_base = o;  o += up(n_pairs * 4);
    L.mask = o;       o += up(rows * 8);
    L.slot = o;       o += up(rows * 8);
    L.items = o;      o += up(L.item_cap * 8);
    L.res = o;        o += up(L.item_cap * 16);
    L.tasks = o;      o += up(L.task_cap * 16);
    L.total = o;
    return L;
}
constexpr int NAR_MIN_TRAIN = 1024;      // narrow scans only for train images of at least this many rows
constexpr int NAR_ITEMS = 256;           // items of a narrow task

struct CandArgs {
    const int32_t *sn2, *sperm, *img_off, *img_n;
    const int32_t *pairs;        // [n_pairs][2] ordered (query image, train image)
    const int32_t *osrc;         // [n_pairs][2]: unordered pair u, role (0: query = B, 1: query = A)
    const int32_t *wg_off;       // [n_u+1]
    const int64_t *col_off, *rowp_off, *out_off;
    const int32_t *col, *rowp;
    double thresh;
    double K;                    // sym_cand_K(thresh), of the reject in front of the rule (sym_cand_rule.h)
    uint8_t *keep;
    int32_t *cand_cnt;           // [n_pairs]: cleared with the keep map, counted by pass 1
    int32_t *cand_q;
    int32_t *task_total;         // [2] wave tasks / workgroup tasks appended so far (zeroed by symcompact_kernel)
    int32_t *tasks;              // [..][2] (ordered pair, block): wave tasks from entry 0, workgroup tasks from entry n_pairs
    int32_t *d2;                 // [rows][2]: [.][1] of a candidate row = upper bound of its exact second distance
    int wg_shift;                // log2 of the candidates of a workgroup task (8; the exact kernels check it)
    // narrow exact stage (nar == NULL: off)
    const uint8_t *colmask;
    int8_t *nar;
    int64_t rows_total;
    int n_pairs, wgrows;
};

// pass 1, one thread per FOUR consecutive sorted query rows of every ordered pair (grid: 1024-row
// chunks of the largest query image x ordered pairs): bounds -> candidate flag at the row's original
// position, the upper bound of its second distance, its class mask, the pair's candidate count.
// Shaped for rows that are thrown away (about 0.1 % of the rows of a survey launch are candidates,
// and the kernel runs beside the next launch's sweep, which is bound by vector issue slots: every
// vector instruction here is taken from it): every load is 16 bytes per lane and all of them are
// issued before the first is unpacked, the decision is sym_cand_reject (two f64 products) with the
// rule's own roots and division behind it for the rows it lets through, and everything a candidate
// alone needs -- sperm, colmask, the second walk over the partials, the stores -- is under its flag.
constexpr int CAND_ROWS = 4;             // rows of a thread (CHUNK is a multiple: a thread's rows end inside cap)

// the four rows' partials of NW workgroups merged into (L, U1, U2) -- the merge of the sorted pairs
// (U1, U2) and (e1, e2) -- with the 2 NW loads in front of the first unpack
template <int NW>
__device__ __forceinline__ void cand_merge_partials(const int32_t *__restrict__ rowq, int64_t cap, int (&L)[CAND_ROWS],
                                                    int (&U1)[CAND_ROWS], int (&U2)[CAND_ROWS])
{
    v4i e[NW][2];
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        e[w][0] = *reinterpret_cast<const v4i *>(rowq + 2 * (w * cap));
        e[w][1] = *reinterpret_cast<const v4i *>(rowq + 2 * (w * cap) + 4);
    }
#pragma unroll
    for (int w = 0; w < NW; ++w)
#pragma unroll
        for (int i = 0; i < CAND_ROWS; ++i) {
            int eL, e1, e2;
            unpack_row_bounds(v2i{e[w][i >> 1][2 * (i & 1)], e[w][i >> 1][2 * (i & 1) + 1]}, eL, e1, e2);
            L[i] = min(L[i], eL);
            const int n1 = min(U1[i], e1);
            U2[i] = min(max(U1[i], e1), min(U2[i], e2));
            U1[i] = n1;
        }
}

__device__ __forceinline__ void symcand_rows_pair(const CandArgs &A, int p, int pos0)
{
    // per-pair constants: one value for the whole workgroup, kept in scalar registers
    const int qimg = uniform32(A.pairs[2 * p]);
    const int u = uniform32(A.osrc[2 * p]), role = uniform32(A.osrc[2 * p + 1]);
    const int soff = uniform32(A.img_off[qimg]), n = uniform32(A.img_n[qimg]);
    if ((int)blockIdx.x * (256 * CAND_ROWS) >= n) return;
    const bool in = pos0 < n;                       // (a thread past the image loads nothing)
    const int64_t cap = (n + CHUNK - 1) / CHUNK * CHUNK;
    const int nwg = uniform32(A.wg_off[u + 1]) - uniform32(A.wg_off[u]);
    const int64_t ob = uniform64(A.out_off[p]);
    const int64_t cb = uniform64(A.col_off[u]);
    const int32_t *rowq = A.rowp + 2 * uniform64(A.rowp_off[u]);
    int U2[CAND_ROWS];
    long long Lb[CAND_ROWS], Ub[CAND_ROWS];
    // (pos0 is a multiple of 4, the image's first sorted row, col_off and rowp_off multiples of
    //  CHUNK: every vector load below is 16-byte aligned and ends at or before row cap - 1)
    v4i n2 = {0, 0, 0, 0};
    if (in) n2 = *reinterpret_cast<const v4i *>(A.sn2 + soff + pos0);
    if (role == 0) {
        v4i c[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        if (in) {
            c[0] = *reinterpret_cast<const v4i *>(A.col + 2 * (cb + pos0));
            c[1] = *reinterpret_cast<const v4i *>(A.col + 2 * (cb + pos0) + 4);
        }
#pragma unroll
        for (int i = 0; i < CAND_ROWS; ++i) {
            const int par = n2[i] & 1;
            const long long cq = n2[i] >> 1;
            U2[i] = 0x7FFFFFFF;
            Lb[i] = 2 * (c[i >> 1][2 * (i & 1)] + cq) + par;
            Ub[i] = 2 * (c[i >> 1][2 * (i & 1) + 1] + cq) + par + 1;
        }
    } else {
        int L[CAND_ROWS], U1[CAND_ROWS];
#pragma unroll
        for (int i = 0; i < CAND_ROWS; ++i) L[i] = U1[i] = U2[i] = 0x7FFFFFFF;
        if (in) {
            const int32_t *rq = rowq + 2 * pos0;
            switch (nwg) {                          // (1024-row workgroups: 4 for a 4096-row image)
            case 1: cand_merge_partials<1>(rq, cap, L, U1, U2); break;
            case 2: cand_merge_partials<2>(rq, cap, L, U1, U2); break;
            case 3: cand_merge_partials<3>(rq, cap, L, U1, U2); break;
            case 4: cand_merge_partials<4>(rq, cap, L, U1, U2); break;
            default: {
                int w = 0;
                for (; w + 4 <= nwg; w += 4) cand_merge_partials<4>(rq + 2 * (w * cap), cap, L, U1, U2);
                for (; w < nwg; ++w) cand_merge_partials<1>(rq + 2 * (w * cap), cap, L, U1, U2);
            }
            }
        }
#pragma unroll
        for (int i = 0; i < CAND_ROWS; ++i) {
            const int par = n2[i] & 1;
            Lb[i] = 2ll * L[i] + par;
            Ub[i] = 2ll * U2[i] + par + 1;
        }
    }
    unsigned kbits = 0u;
#pragma unroll
    for (int i = 0; i < CAND_ROWS; ++i) {
        if (Lb[i] < 0) Lb[i] = 0;
        if (pos0 + i < n && !sym_cand_reject(Lb[i], Ub[i], A.K) && sym_cand_keep(Lb[i], Ub[i], A.thresh))
            kbits |= 1u << i;
    }
    // ---- candidates only (none in nearly every wave of a survey launch)
    if (kbits == 0u) return;
    // the pair's candidate count: one add per wave that holds a candidate
    const unsigned long long holders = __ballot(1);
    int wave_cnt = 0;
#pragma unroll
    for (int i = 0; i < CAND_ROWS; ++i) wave_cnt += __popcll(__ballot((kbits >> i) & 1u));
    if ((int)(threadIdx.x & 63) == __ffsll((long long)holders) - 1) atomicAdd(A.cand_cnt + p, wave_cnt);
    // narrow exact stage: classes of this ordered pair's train image (8 groups of the streamed image
    // when the query was a B row, the nwg row blocks of the register-resident image otherwise)
    const int ncls = role == 0 ? 8 : nwg;
    const bool nar_ok = A.nar != nullptr && A.img_n[A.pairs[2 * p + 1]] >= NAR_MIN_TRAIN && ncls <= 64;
#pragma unroll
    for (int i = 0; i < CAND_ROWS; ++i) {
        if (!((kbits >> i) & 1u)) continue;
        const int pos = pos0 + i;
        const int orig = A.sperm[soff + pos];
        // the flag at the row's ORIGINAL position, one bit per row in a map cleared by the launch (a byte
        // per row until round 6: 33 M scattered byte writes per launch of 4096 synthetic pairs were most of
        // this kernel's time; now only the candidates write)
        atomicOr(reinterpret_cast<unsigned *>(A.keep) + ((ob + orig) >> 5), 1u << ((ob + orig) & 31));
        // what the exact stage prunes its scan with: no row farther than this can be the best or
        // the second of the candidate (replaced by the exact pair of distances there)
        A.d2[2 * (ob + orig) + 1] = (int)(Ub[i] < 0x7FFFFFFFll ? Ub[i] : 0x7FFFFFFFll);
        if (nar_ok) {
            // the classes that can hold a row at or below Ub (every other row is farther than the
            // exact second distance): group minimum <= v2, block lower bound <= U2
            unsigned long long mk = 0ull;
            if (role == 0) {
                mk = A.colmask[cb + pos];
            } else {
                for (int w = 0; w < nwg; ++w)
                    if (rowq[2 * (w * cap + pos)] <= U2[i]) mk |= 1ull << w;
            }
            const NarLayout NL = narrow_layout(A.rows_total, A.n_pairs);
            reinterpret_cast<unsigned long long *>(A.nar + NL.mask)[ob + orig] = mk;
        }
    }
}

__global__ __launch_bounds__(256) void symcand_rows_kernel(CandArgs A)
{
    // (1024 rows per workgroup: beside the next launch's sweep -- whose workgroups own their compute
    //  units -- every workgroup of this grid waits for a unit to come free; 131 k small ones per
    //  launch of 4096 synthetic pairs cost the sweep more than the kernel's own work)
    for (int p = blockIdx.y; p < A.n_pairs; p += gridDim.y)
        symcand_rows_pair(A, p, ((int)blockIdx.x * 256 + (int)threadIdx.x) * CAND_ROWS);
}

// words [0, n_words) of the keep map and the candidate counts of the pairs, cleared in one launch
__global__ __launch_bounds__(256) void symcand_clear_kernel(unsigned *keep, int64_t n_words, int32_t *cand_cnt, int n_pairs)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += stride) keep[i] = 0u;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_pairs; i += stride) cand_cnt[i] = 0;
}

// passes 2 and 3, one workgroup per ordered pair
__global__ __launch_bounds__(256) void symcand_kernel(CandArgs A)
{
    __shared__ int wcnt[4];
    __shared__ int s_base;
    const int p = blockIdx.x;
    const NarLayout NL = narrow_layout(A.rows_total, A.n_pairs);
    // a pair without a candidate (pass 1 counted them; nearly every pair of a survey launch) costs
    // this one load: no scan of the bit map, no barrier
    if (A.cand_cnt[p] == 0) {
        if (threadIdx.x == 0) {
            A.cand_cnt[p] = 0;
            if (A.nar != nullptr) reinterpret_cast<int32_t *>(A.nar + NL.pair_base)[p] = -1;
        }
        return;
    }
    const int qimg = A.pairs[2 * p];
    const int u = A.osrc[2 * p], role = A.osrc[2 * p + 1];
    const int n = A.img_n[qimg];
    const int nwg = A.wg_off[u + 1] - A.wg_off[u];
    const int64_t ob = A.out_off[p];
    const int ncls = role == 0 ? 8 : nwg;
    const bool nar_ok = A.nar != nullptr && A.img_n[A.pairs[2 * p + 1]] >= NAR_MIN_TRAIN && ncls <= 64;
    unsigned long long *maskv = reinterpret_cast<unsigned long long *>(A.nar + NL.mask);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the flagged rows by WORDS of the bit map: a lane takes 32 rows, a popcount prefix runs over the
    // wave and then over the four waves, the set bits expand into the list (8192 rows per pair of
    // barriers; a ballot per 256 rows until round 14).  The pair's bits are [ob, ob + n): its first
    // and last word are shared with its neighbours and masked to its own rows.
    const unsigned *keepw = reinterpret_cast<const unsigned *>(A.keep);
    const int64_t w_first = ob >> 5, w_last = (ob + n - 1) >> 5;
    int out = 0;
    for (int64_t wbase = w_first; wbase <= w_last; wbase += 256) {
        const int64_t w = wbase + threadIdx.x;
        unsigned bits = 0u;
        if (w <= w_last) {
            bits = keepw[w];
            if (w == w_first) bits &= ~0u << (ob & 31);
            if (w == w_last) bits &= ~0u >> (31 - (int)((ob + n - 1) & 31));
        }
        const int c = __popc(bits);
        int x = c;
#pragma unroll
        for (int sft = 1; sft < 64; sft <<= 1) {
            const int y = __shfl_up(x, sft);
            if (lane >= sft) x += y;
        }
        if (lane == 63) wcnt[wave] = x;
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < wave) woff += wcnt[k];
            tot += wcnt[k];
        }
        int at = out + woff + x - c;
        const int row0 = (int)((w << 5) - ob);               // row of bit 0 of this word (negative in the first)
        for (unsigned b = bits; b; b &= b - 1) A.cand_q[ob + at++] = row0 + __ffs((int)b) - 1;
        out += tot;
        __syncthreads();
    }
    // ---- narrow exact stage: items (candidate, class) bucketed by class, tasks of one class
    bool narrow = nar_ok && out > 64;
    if (A.nar != nullptr) {
        __shared__ int cls_cnt[64], cls_off[65], cls_task[65], s_nb;
        int32_t *ctl = reinterpret_cast<int32_t *>(A.nar + NL.ctl);
        int32_t *pair_base = reinterpret_cast<int32_t *>(A.nar + NL.pair_base);
        v2i *slot = reinterpret_cast<v2i *>(A.nar + NL.slot);
        v2i *items = reinterpret_cast<v2i *>(A.nar + NL.items);
        NarTask *ntasks = reinterpret_cast<NarTask *>(A.nar + NL.tasks);
        if (narrow) {
            if (threadIdx.x < 64) cls_cnt[threadIdx.x] = 0;
            __syncthreads();
            int run = 0;                                   // result slots handed out so far
            for (int base = 0; base < out; base += 256) {
                const int i = base + threadIdx.x;
                unsigned long long mk = 0ull;
                if (i < out) mk = maskv[ob + A.cand_q[ob + i]];
                const int nk = __popcll(mk);
                int x = nk;
#pragma unroll
                for (int sft = 1; sft < 64; sft <<= 1) {
                    const int y = __shfl_up(x, sft);
                    if (lane >= sft) x += y;
                }
                if (lane == 63) wcnt[wave] = x;
                __syncthreads();
                int woff = 0, tot = 0;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    if (w < wave) woff += wcnt[w];
                    tot += wcnt[w];
                }
                if (i < out) {
                    slot[ob + i] = v2i{run + woff + x - nk, nk};
                    for (unsigned long long b = mk; b; b &= b - 1) atomicAdd(&cls_cnt[__ffsll((long long)b) - 1], 1);
                }
                run += tot;
                __syncthreads();
            }
            if (threadIdx.x == 0) {
                int o = 0, nt = 0;
                for (int cidx = 0; cidx < 64; ++cidx) {
                    cls_off[cidx] = o;
                    cls_task[cidx] = nt;
                    o += cls_cnt[cidx];
                    nt += (cls_cnt[cidx] + NAR_ITEMS - 1) / NAR_ITEMS;
                }
                cls_off[64] = o;
                cls_task[64] = nt;
                // (a batch whose items or tasks do not fit falls back to the full scan, pair by pair)
                const int b0 = atomicAdd(ctl + 1, run);
                bool ok = (int64_t)b0 + run <= NL.item_cap;
                int t0 = 0;
                if (ok) {
                    t0 = atomicAdd(ctl + 0, nt);
                    ok = (int64_t)t0 + nt <= NL.task_cap;
                }
                s_nb = ok ? b0 : -1;
                s_base = t0;
                pair_base[p] = ok ? b0 : -1;
            }
            __syncthreads();
            narrow = s_nb >= 0;
            if (narrow) {
                const int b0 = s_nb, t0 = s_base;
                if (threadIdx.x < 64) {
                    const int cidx = threadIdx.x, cnt_c = cls_cnt[cidx];
                    for (int t = 0; t * NAR_ITEMS < cnt_c; ++t)
                        ntasks[t0 + cls_task[cidx] + t] =
                            NarTask{p, cidx, b0 + cls_off[cidx] + t * NAR_ITEMS, min(NAR_ITEMS, cnt_c - t * NAR_ITEMS)};
                }
                __syncthreads();
                if (threadIdx.x < 64) cls_cnt[threadIdx.x] = 0;       // now the buckets' cursors
                __syncthreads();
                for (int i = threadIdx.x; i < out; i += 256) {
                    const unsigned long long mk = maskv[ob + A.cand_q[ob + i]];
                    int sl = b0 + slot[ob + i].x;
                    for (unsigned long long b = mk; b; b &= b - 1, ++sl) {
                        const int cidx = __ffsll((long long)b) - 1;
                        const int at = atomicAdd(&cls_cnt[cidx], 1);
                        items[b0 + cls_off[cidx] + at] = v2i{i, sl};
                    }
                }
            }
            __syncthreads();
        } else if (threadIdx.x == 0) {
            pair_base[p] = -1;
        }
    }
    if (narrow) {
        if (threadIdx.x == 0) A.cand_cnt[p] = out;
        return;
    }
    // two task lists in one buffer: a pair with <= 64 candidates is ONE wave's task (entries
    // [0, n_pairs): at most one per pair), a pair with more gets workgroup tasks of 256 candidates
    // whose four waves share every train tile through LDS (entries from n_pairs on)
    const bool small = out <= 64;
    const int ntask = small ? (out > 0 ? 1 : 0) : (out + (1 << A.wg_shift) - 1) >> A.wg_shift;
    if (threadIdx.x == 0) {
        A.cand_cnt[p] = out;
        s_base = ntask ? atomicAdd(A.task_total + (small ? 0 : 1), ntask) + (small ? 0 : (int)gridDim.x) : 0;
    }
    __syncthreads();
    // (a workgroup task carries the granularity it was cut to: the exact kernels check it)
    const int tag = small ? 0 : (A.wg_shift << 24);
    for (int t = threadIdx.x; t < ntask; t += 256)
        *reinterpret_cast<v2i *>(A.tasks + 2 * (s_base + t)) = v2i{p, t | tag};
}

// ---------------------------------------------------------------------------------
// exact top-2 of the candidate rows (original-order store), metric, final keep flag.
// A TASK = up to 32 candidate rows of one ordered pair against every row of its train image,
// on the MFMA like the general kernel (match_knn2.hip: packed key = distance | train row,
// v_med3 / v_min, lowest train row wins ties), run by ONE wave on its own: the candidates are
// the B operand, the train rows come straight from L2 (16 bytes per lane and 32-row tile; all
// tasks of a pair read the same 512 KiB).  Survivors cluster in the few overlapping image pairs
// of a launch, so the tasks of all pairs form one flat list (appended to by symcand_kernel) that
// a persistent grid walks.
// ---------------------------------------------------------------------------------
struct ExactArgs {
    const int8_t *desc;          // original-order store (iamx_desc_pack_*)
    const int32_t *norm_q;       // |s|^2 per row
    const int32_t *norm_t;       // |s|^2 + 2 sum(s) per row
    const int32_t *key_t;        // norm_t * 256 + (store row & 255) per row (symexact_keys_kernel)
    int n_pairs;                 // (the workgroup tasks start at entry n_pairs of `tasks`)
    const int32_t *img_off, *img_n;
    const int32_t *pairs;
    const int64_t *out_off;      // first row of a pair in d2 AND first entry of its candidate list
    const int32_t *cand_cnt;
    const int32_t *cand_q;
    const int32_t *task_total, *tasks;
    double thresh;
    int32_t *d2;                 // [rows][2]: exact (best, second) written for the candidates
    int32_t *cand_t;
    double *cand_metric;
    uint8_t *cand_keep;
    int32_t *zero_div;
};

__device__ __forceinline__ int med3_key(int a, int b, int c)
{
    // `c` is always a compiler-generated VALU result (the packed key), never a raw MFMA
    // accumulator: no MFMA -> VALU hazard hides inside the asm statement
    int r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// key_t[g] = norm_t[g] * 256 + (g & 255) for every row g of the store: the per-row constant of
// the packed key, so that the scan below builds a key with ONE v_lshl_add_u32 per entry
__global__ __launch_bounds__(256) void symexact_keys_kernel(const int32_t *__restrict__ norm_t,
                                                            int64_t total_rows,
                                                            int32_t *__restrict__ key_t)
{
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total_rows;
         g += (int64_t)gridDim.x * 256)
        key_t[g] = norm_t[g] * 256 + (int)(g & 255);
}

__device__ __forceinline__ int lshl9_add(int a, int b)
{
    // (a << 9) + b in one instruction; `a` is a raw MFMA accumulator here: the compiler sees a
    // plain VALU use of it and inserts the MFMA -> VALU wait states itself
    return (int)(((unsigned)a << 9) + (unsigned)b);
}

// the end of a candidate's scan: merge the two lane halves (rows +4) lexicographically by
// (distance, row), write the exact squared distances, the train row, the metric and the keep flag
__device__ __forceinline__ void exact_finish(const ExactArgs &A, int p, int64_t cb, int cnt, int qoff,
                                             int q, int k, int g, int bd1, int bi1, int bd2, int bi2)
{
    const int od1 = __shfl_xor(bd1, 32), oi1 = __shfl_xor(bi1, 32);
    const int od2 = __shfl_xor(bd2, 32), oi2 = __shfl_xor(bi2, 32);
    auto less = [](int da, int ia, int db, int ib) { return da < db || (da == db && ia < ib); };
    int f_d, f_i, s_d;
    if (less(od1, oi1, bd1, bi1)) {
        f_d = od1; f_i = oi1;
        s_d = less(bd1, bi1, od2, oi2) ? bd1 : od2;
    } else {
        f_d = bd1; f_i = bi1;
        s_d = less(od1, oi1, bd2, bi2) ? od1 : bd2;
    }
    if (g == 0 && k < cnt) {
        const int na = A.norm_q[qoff + q];
        const int d1 = f_d + na, d2 = s_d + na;
        *reinterpret_cast<v2i *>(A.d2 + 2 * (A.out_off[p] + q)) = v2i{d1, d2};
        // cv2 L2 distance = float32 sqrt; the rest in float64 like python (matcher.py:253-263)
        const float f0 = (float)sqrt((double)d1);
        const float f1 = (float)sqrt((double)d2);
        double mt;
        bool ok = false;
        if (f1 == 0.0f) {
            mt = __longlong_as_double(0x7FF8000000000000LL);    // python raises ZeroDivisionError
            atomicAdd(A.zero_div, 1);
        } else {
            mt = (double)f0 * ((double)f0 / (double)f1);
            ok = mt < A.thresh;
        }
        A.cand_t[cb + k] = f_i;
        A.cand_metric[cb + k] = mt;
        A.cand_keep[cb + k] = ok ? 1 : 0;
    }
}

// A TASK = up to 64 candidate rows of one ordered pair (two B operands: every train tile that
// comes up from L2 serves both) against every row of its train image.  The scan is written for
// the VALU, which bounds it: per 32 x 32 tile and candidate set 4 MFMAs and 16 x (key, med3, min)
// = 48 VALU instructions -- the first version spent ~200 (key from three terms, a select for the
// ragged last tile in every tile, 32 register copies for the one-tile-ahead prefetch) and ran at
// 0.5 PFLOP/s, a third of the sweep's time on synthetic descriptors but THREE TIMES the sweep on
// real frames, where a third to two thirds of a pair's rows are candidates.
// Epochs of the packed keys follow the store's row numbers (images start on multiples of 128).
__global__ __launch_bounds__(256) void symexact_kernel(ExactArgs A)
{
    constexpr int KEY_INVALID = 0x7FFFFFFF;
    const int total = A.task_total[0];
    const int lane = threadIdx.x & 63;
    const int c = lane & 31, g = lane >> 5;
    const int nwaves = gridDim.x * 4;
    for (int t = blockIdx.x * 4 + (threadIdx.x >> 6); t < total; t += nwaves) {
        // (a task is the whole wave's: its numbers live in scalar registers, the tile loop's tests
        //  are scalar branches)
        const v2i task = *reinterpret_cast<const v2i *>(A.tasks + 2 * t);
        const int p = __builtin_amdgcn_readfirstlane(task.x);
        const int tblk = __builtin_amdgcn_readfirstlane(task.y);
        const int64_t cb = A.out_off[p];
        const int cnt = __builtin_amdgcn_readfirstlane(A.cand_cnt[p]);
        const int qimg = A.pairs[2 * p], timg = A.pairs[2 * p + 1];
        const int qoff = __builtin_amdgcn_readfirstlane(A.img_off[qimg]);
        const int toff = __builtin_amdgcn_readfirstlane(A.img_off[timg]);
        const int nt = __builtin_amdgcn_readfirstlane(A.img_n[timg]);
        int kq[2], q[2];
        v4i bq[2][4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            kq[h] = tblk * 64 + h * 32 + c;
            q[h] = A.cand_q[cb + (kq[h] < cnt ? kq[h] : cnt - 1)];
            const v4i *src = reinterpret_cast<const v4i *>(A.desc + (int64_t)(qoff + q[h]) * D);
#pragma unroll
            for (int s = 0; s < 4; ++s) bq[h][s] = ~src[2 * s + g];
        }
        const int8_t *tbase = A.desc + (int64_t)toff * D;
        const int32_t *tkey = A.key_t + toff;
        const int ntiles = (nt + 31) / 32;
        auto load_tile = [&](int tile, v4i (&a)[4], v4i (&tk)[4]) {
            // rows past the end stay inside the image's 128-row padding; their keys are masked
            const v4i *src = reinterpret_cast<const v4i *>(tbase + (int64_t)(tile * 32 + c) * D);
#pragma unroll
            for (int s = 0; s < 4; ++s) a[s] = src[2 * s + g];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                tk[kk] = *reinterpret_cast<const v4i *>(tkey + tile * 32 + 8 * kk + 4 * g);
        };
        int m1[2] = {KEY_INVALID, KEY_INVALID}, m2[2] = {KEY_INVALID, KEY_INVALID};
        int bd1[2] = {KEY_INVALID, KEY_INVALID}, bi1[2] = {0, 0};
        int bd2[2] = {KEY_INVALID, KEY_INVALID}, bi2[2] = {0, 0};
        // a task at the end of a pair's list (or the only one of a pair with a few candidates --
        // every pair of bench.py's synthetic surveys) fills one candidate set only
        const bool two_sets = cnt - tblk * 64 > 32;
        auto scan_tile = [&](int tile, const v4i (&a)[4], const v4i (&tk)[4]) {
            const bool ragged = tile * 32 + 32 > nt;              // (wave uniform: the last tile only)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (h == 1 && !two_sets) break;
                v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], bq[h][s], acc, 0, 0, 0);
                if (!ragged) {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int key = lshl9_add(acc[reg], tk[reg >> 2][reg & 3]);
                        m2[h] = med3_key(m1[h], m2[h], key);
                        m1[h] = min(m1[h], key);
                    }
                } else {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int row = tile * 32 + 8 * (reg >> 2) + 4 * g + (reg & 3);
                        int key = lshl9_add(acc[reg], tk[reg >> 2][reg & 3]);
                        key = row < nt ? key : KEY_INVALID;
                        m2[h] = med3_key(m1[h], m2[h], key);
                        m1[h] = min(m1[h], key);
                    }
                }
            }
            // fold the packed keys of this 256-row epoch of the STORE into (distance, row) pairs
            const int grow = toff + tile * 32;                    // first store row of the tile
            if (((grow + 32) & 255) == 0 || tile == ntiles - 1) {
                const int sbase = (grow & ~255) - toff;           // epoch start as a row of the image
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int d1k = m1[h] >> 8, i1k = sbase + (m1[h] & 255);
                    const int d2k = m2[h] >> 8, i2k = sbase + (m2[h] & 255);
                    if (d1k < bd1[h]) {
                        if (d2k < bd1[h]) { bd2[h] = d2k; bi2[h] = i2k; }
                        else              { bd2[h] = bd1[h]; bi2[h] = bi1[h]; }
                        bd1[h] = d1k; bi1[h] = i1k;
                    } else if (d1k < bd2[h]) {
                        bd2[h] = d1k; bi2[h] = i1k;
                    }
                    m1[h] = m2[h] = KEY_INVALID;
                }
            }
        };
        // two register sets, tiles alternate between them: the loads of tile + 1 are in flight
        // while tile is scanned, without copying a set into the other
        v4i a0[4], k0[4], a1[4], k1[4];
        load_tile(0, a0, k0);
        for (int tile = 0; tile < ntiles; tile += 2) {
            load_tile(tile + 1 < ntiles ? tile + 1 : tile, a1, k1);
            scan_tile(tile, a0, k0);
            if (tile + 1 < ntiles) {
                load_tile(tile + 2 < ntiles ? tile + 2 : tile + 1, a0, k0);
                scan_tile(tile + 1, a1, k1);
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
            exact_finish(A, p, cb, cnt, qoff, q[h], kq[h], g, bd1[h], bi1[h], bd2[h], bi2[h]);
    }
}

// Workgroup form of the exact stage for pairs with MANY candidates (real frames: a third to two
// thirds of a pair's rows): a task = 256 candidates of one ordered pair, 64 per wave as two B
// operands; the four waves share every 32-row train tile through LDS -- fetched once per
// workgroup, coalesced (thread = 16 bytes of a row, a wave = 8 whole rows) instead of once per wave
// as 64 scattered 16-byte pieces (what bounded the wave form: the CU's texture addresser, not the
// VALU).  LDS rows are XOR-swizzled by 16-byte chunk (chunk j of row r sits at j ^ ((r >> 1) & 7)):
// a ds_read_b128 is served in four groups of 16 lanes -- rows {0-3, 12-15, 20-27} and {4-11, 16-19,
// 28-31} of a lane half -- and two rows share the 64 banks, so the eight row PAIRS of a group must
// land on eight different chunks; r & 7 left them two-way conflicted (26 % of the LDS cycles).  Two tile buffers, one
// barrier per tile; tile T + 1 is in flight from L2 while tile T is scanned.
//
// PRUNE: the scan is bound by the VALU (SQ counters on overlapping frames: 126 VALU instructions
// per wave and tile, 78 % of the SIMD's issue slots; profiles/r5_exact_pmc_unpruned_*.txt), and 96 of the
// 126 keep a best and a second over rows that cannot be either: symcand_kernel knows an upper
// bound U of the candidate's exact second distance (d2[.][1]).  With c = norm_t >> 1 of the train
// row as the MFMA's C operand the accumulator IS the halved distance term h (distance - norm_q =
// 2 h + parity of norm_t), a row with h > (U - norm_q) >> 1 is out, and a tile is scanned the old
// way only if some lane's minimum over its 16 accumulators (8 x v_min3) is not: ~2 rows per
// candidate, ~60 of a wave's ~1150 tiles.  Keys, ties and the result are the unpruned scan's.
//
// SUB tiles are staged per barrier (a PHASE): the waves run that many tiles on their own between
// two workgroup rendezvous.
template <bool PRUNE, int SUB>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void symexact_wg_kernel(ExactArgs A)
{
    constexpr int KEY_INVALID = 0x7FFFFFFF;
    constexpr int PR = 32 * SUB;                                           // rows per phase
    __shared__ __attribute__((aligned(16))) int8_t s_tile[2][PR * D];
    __shared__ __attribute__((aligned(16))) int32_t s_key[2][PR];      // PRUNE: key_t & 511
    __shared__ __attribute__((aligned(16))) int32_t s_half[2][PR];     // PRUNE: key_t >> 9 = norm_t >> 1
    const int total = A.task_total[1];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, g = lane >> 5;
    const int lrow = threadIdx.x >> 3, lchunk = threadIdx.x & 7;      // staging: 16 bytes per thread
    for (int t = blockIdx.x; t < total; t += gridDim.x) {
        const v2i task = *reinterpret_cast<const v2i *>(A.tasks + 2 * ((int64_t)A.n_pairs + t));
        const int p = __builtin_amdgcn_readfirstlane(task.x);
        const int ttag = __builtin_amdgcn_readfirstlane(task.y);
        if ((ttag >> 24) != 8) {        // not cut to 256 candidates: refuse loudly
            if (threadIdx.x == 0) atomicAdd(A.zero_div + 1, 1);
            continue;
        }
        const int tblk = ttag & 0xFFFFFF;
        const int64_t cb = A.out_off[p];
        const int cnt = __builtin_amdgcn_readfirstlane(A.cand_cnt[p]);
        const int qimg = A.pairs[2 * p], timg = A.pairs[2 * p + 1];
        const int qoff = __builtin_amdgcn_readfirstlane(A.img_off[qimg]);
        const int toff = __builtin_amdgcn_readfirstlane(A.img_off[timg]);
        const int nt = __builtin_amdgcn_readfirstlane(A.img_n[timg]);
        const int k_wave = tblk * 256 + wave * 64;                     // first candidate of this wave
        const int n_sets = cnt - k_wave > 32 ? 2 : (cnt - k_wave > 0 ? 1 : 0);
        int kq[2], q[2], hmax[2];
        v4i bq[2][4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            kq[h] = k_wave + h * 32 + c;
            q[h] = A.cand_q[cb + (kq[h] < cnt ? kq[h] : cnt - 1)];
            const v4i *src = reinterpret_cast<const v4i *>(A.desc + (int64_t)(qoff + q[h]) * D);
#pragma unroll
            for (int s = 0; s < 4; ++s) bq[h][s] = ~src[2 * s + g];
            // (read before this task's exact_finish replaces it; a padding lane repeats the
            //  pair's last candidate, which is this task's)
            hmax[h] = PRUNE ? (A.d2[2 * (cb + q[h]) + 1] - A.norm_q[qoff + q[h]]) >> 1 : 0;
        }
        bool dirty = false;                            // (wave-uniform: keys since the last fold)
        const int8_t *tbase = A.desc + (int64_t)toff * D;
        const int32_t *tkey = A.key_t + toff;
        const int ntiles = (nt + 31) / 32;
        int m1[2] = {KEY_INVALID, KEY_INVALID}, m2[2] = {KEY_INVALID, KEY_INVALID};
        int bd1[2] = {KEY_INVALID, KEY_INVALID}, bi1[2] = {0, 0};
        int bd2[2] = {KEY_INVALID, KEY_INVALID}, bi2[2] = {0, 0};
        // (rows past the end stay inside the image's 128-row padding; their keys are masked)
        // (a phase may reach past the last tile: still inside the padding, never scanned)
        auto fetch = [&](int ph, v4i (&row16)[SUB], int &key) {
#pragma unroll
            for (int j = 0; j < SUB; ++j)
                row16[j] = *reinterpret_cast<const v4i *>(tbase + (int64_t)(ph * PR + j * 32 + lrow) * D + 16 * lchunk);
            key = threadIdx.x < PR ? tkey[ph * PR + threadIdx.x] : 0;
        };
        auto stage = [&](int buf, const v4i (&row16)[SUB], int key) {
#pragma unroll
            for (int j = 0; j < SUB; ++j)
                *reinterpret_cast<v4i *>(&s_tile[buf][(j * 32 + lrow) * D + 16 * (lchunk ^ ((lrow >> 1) & 7))]) = row16[j];
            if (threadIdx.x < PR) {
                s_key[buf][threadIdx.x] = PRUNE ? key & 511 : key;
                if (PRUNE) s_half[buf][threadIdx.x] = key >> 9;
            }
        };
        v4i pre[SUB];
        int pre_key;
        const int nph = (ntiles + SUB - 1) / SUB;
        __syncthreads();                               // (the previous task's last tile is consumed)
        fetch(0, pre, pre_key);
        stage(0, pre, pre_key);
        __syncthreads();
        for (int ph = 0; ph < nph; ++ph) {
            const int buf = ph & 1;
            if (ph + 1 < nph) fetch(ph + 1, pre, pre_key);
#pragma unroll
            for (int j = 0; j < SUB; ++j) {
            const int tile = ph * SUB + j;
            if (n_sets > 0 && tile < ntiles) {
                v4i a[4], tk[4];
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    a[s] = *reinterpret_cast<const v4i *>(&s_tile[buf][(j * 32 + c) * D + 16 * ((2 * s + g) ^ ((c >> 1) & 7))]);
                v16i cin = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                if (PRUNE) {
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) {
                        const v4i t = *reinterpret_cast<const v4i *>(&s_half[buf][j * 32 + 8 * kk + 4 * g]);
                        cin[4 * kk] = t.x; cin[4 * kk + 1] = t.y; cin[4 * kk + 2] = t.z; cin[4 * kk + 3] = t.w;
                    }
                } else {
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk)
                        tk[kk] = *reinterpret_cast<const v4i *>(&s_key[buf][j * 32 + 8 * kk + 4 * g]);
                }
                const bool ragged = tile * 32 + 32 > nt;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (h == 1 && n_sets < 2) break;
                    v16i acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[0], bq[h][0], cin, 0, 0, 0);
#pragma unroll
                    for (int s = 1; s < 4; ++s)
                        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], bq[h][s], acc, 0, 0, 0);
                    if (PRUNE) {
                        const int t0 = min(min(acc[0], acc[1]), acc[2]), t1 = min(min(acc[3], acc[4]), acc[5]);
                        const int t2 = min(min(acc[6], acc[7]), acc[8]), t3 = min(min(acc[9], acc[10]), acc[11]);
                        const int t4 = min(min(acc[12], acc[13]), acc[14]);
                        const int lo = min(min(min(t0, t1), t2), min(min(t3, t4), acc[15]));
                        if (__ballot(lo <= hmax[h]) == 0ull) continue;
                        dirty = true;
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk)
                            tk[kk] = *reinterpret_cast<const v4i *>(&s_key[buf][j * 32 + 8 * kk + 4 * g]);
                    }
                    if (!ragged) {
#pragma unroll
                        for (int reg = 0; reg < 16; ++reg) {
                            const int key = lshl9_add(acc[reg], tk[reg >> 2][reg & 3]);
                            m2[h] = med3_key(m1[h], m2[h], key);
                            m1[h] = min(m1[h], key);
                        }
                    } else {
#pragma unroll
                        for (int reg = 0; reg < 16; ++reg) {
                            const int row = tile * 32 + 8 * (reg >> 2) + 4 * g + (reg & 3);
                            int key = lshl9_add(acc[reg], tk[reg >> 2][reg & 3]);
                            key = row < nt ? key : KEY_INVALID;
                            m2[h] = med3_key(m1[h], m2[h], key);
                            m1[h] = min(m1[h], key);
                        }
                    }
                }
                const int grow = toff + tile * 32;
                if ((!PRUNE || dirty) && (((grow + 32) & 255) == 0 || tile == ntiles - 1)) {
                    dirty = false;
                    const int sbase = (grow & ~255) - toff;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int d1k = m1[h] >> 8, i1k = sbase + (m1[h] & 255);
                        const int d2k = m2[h] >> 8, i2k = sbase + (m2[h] & 255);
                        if (d1k < bd1[h]) {
                            if (d2k < bd1[h]) { bd2[h] = d2k; bi2[h] = i2k; }
                            else              { bd2[h] = bd1[h]; bi2[h] = bi1[h]; }
                            bd1[h] = d1k; bi1[h] = i1k;
                        } else if (d1k < bd2[h]) {
                            bd2[h] = d1k; bi2[h] = i1k;
                        }
                        m1[h] = m2[h] = KEY_INVALID;
                    }
                }
            }
            }
            if (ph + 1 < nph) stage(buf ^ 1, pre, pre_key);
            __syncthreads();
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
            exact_finish(A, p, cb, cnt, qoff, q[h], kq[h], g, bd1[h], bi1[h], bd2[h], bi2[h]);
    }
}

// ---------------------------------------------------------------------------------
// narrow exact stage: a task = up to 256 items (candidate, class) of one ordered pair and ONE
// class, four waves x two sets of 32 as in symexact_wg_kernel; the class's rows come from the
// SORTED store (the order the sweep's classes are defined in) as 32-row tiles through LDS:
//   row direction  (query was an A row): class w = sorted rows [w * wgrows, (w + 1) * wgrows) of the
//                  register-resident image, consecutive tiles;
//   column direction (query was a B row): class (k, g) = the rows the sweep's lanes of half g saw
//                  in tiles with (tile & 3) == k: rows 8 i + 4 g + (0..3), i = 0..3, of such a tile
//                  -- a packed tile takes its 16 rows from two of them.
// Per row: C operand = sct (halved norm term; 2^25 on rows past the end: never below a bound,
// still no overflow in the key), parity and the row's position among the lane's 16 accumulators
// (`pk`), the original row number (`idx`: what the reference breaks ties with).  The pruning test
// is symexact_wg_kernel's; a tile that passes builds keys (acc << 5 | parity << 4 | position),
// takes best and second with v_med3 / v_min and folds them at once -- the row number of the best
// from LDS -- unless some lane holds two equal distances among its 16 rows: then every row of the
// tile goes through the full (distance, original row) comparison.
// ---------------------------------------------------------------------------------
struct NarArgs {
    const int8_t *desc;          // original-order store: the candidates' rows
    const int32_t *norm_q, *img_off;
    const int32_t *pairs, *osrc;
    const int64_t *out_off;
    const int32_t *cand_q;
    const int32_t *d2;
    const int8_t *sdesc;         // sorted store: the train rows
    const int32_t *sn2, *sct, *sperm, *img_off3, *img_n;
    int8_t *nar;
    int64_t rows_total;
    int n_pairs, wgrows;
    // finish
    const int32_t *cand_cnt;
    double thresh;
    int32_t *d2w, *cand_t;
    double *cand_metric;
    uint8_t *cand_keep;
    int32_t *zero_div;
};

constexpr int NAR_HALF_INVALID = 1 << 25;
constexpr int NAR_D_INVALID = 0x7FFFFFFF;

template <int WPE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void symnarrow_kernel(NarArgs A)
{
    constexpr int SUB = 2, PR = 32 * SUB;
    __shared__ __attribute__((aligned(16))) int8_t s_tile[2][PR * D];
    __shared__ __attribute__((aligned(16))) int32_t s_half[2][PR];
    __shared__ __attribute__((aligned(16))) int32_t s_pk[2][PR];
    __shared__ __attribute__((aligned(16))) int32_t s_idx[2][PR];
    const NarLayout NL = narrow_layout(A.rows_total, A.n_pairs);
    int32_t *ctl = reinterpret_cast<int32_t *>(A.nar + NL.ctl);
    const NarTask *ntasks = reinterpret_cast<const NarTask *>(A.nar + NL.tasks);
    const v2i *items = reinterpret_cast<const v2i *>(A.nar + NL.items);
    v4i *res = reinterpret_cast<v4i *>(A.nar + NL.res);
    const int total = ctl[0];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, g = lane >> 5;
    const int lrow = threadIdx.x >> 3, lchunk = threadIdx.x & 7;      // staging: 16 bytes per thread
    // tasks are taken from a counter (ctl[2]; reset by the finish kernel): a column-direction task
    // scans 4.5 x the rows of a row-direction one, and only part of the grid is resident at a time
    __shared__ int s_task;
    for (;;) {
        __syncthreads();                               // (the previous task's last tile is consumed)
        if (threadIdx.x == 0) s_task = atomicAdd(ctl + 2, 1);
        __syncthreads();
        const int t = s_task;
        if (t >= total) break;
        const NarTask task = ntasks[t];
        const int p = __builtin_amdgcn_readfirstlane(task.p);
        const int cls = __builtin_amdgcn_readfirstlane(task.cls);
        const int item0 = __builtin_amdgcn_readfirstlane(task.item0);
        const int nit = __builtin_amdgcn_readfirstlane(task.n);
        const int64_t cb = A.out_off[p];
        const int qimg = A.pairs[2 * p], timg = A.pairs[2 * p + 1];
        const int role = __builtin_amdgcn_readfirstlane(A.osrc[2 * p + 1]);
        const int qoff = __builtin_amdgcn_readfirstlane(A.img_off[qimg]);
        const int toff = __builtin_amdgcn_readfirstlane(A.img_off3[timg]);
        const int nt = __builtin_amdgcn_readfirstlane(A.img_n[timg]);
        // class geometry: packed tile j, packed row r -> sorted position (or -1)
        int ntiles, first = 0, ck = 0, cg = 0;
        if (role != 0) {
            first = cls * A.wgrows;
            const int last = min(nt, first + A.wgrows);
            ntiles = last > first ? (last - first + 31) / 32 : 0;
        } else {
            ck = cls & 3;
            cg = cls >> 2;
            const int tt = (nt + 31) / 32;
            const int nk = tt > ck ? (tt - ck + 3) / 4 : 0;
            ntiles = (nk + 1) / 2;
        }
        auto position = [&](int j, int r) -> int {
            int pos;
            if (role != 0) {
                pos = first + j * 32 + r;
                if (pos >= first + A.wgrows) pos = nt;
            } else {
                const int T = 4 * (2 * j + (r >> 4)) + ck, rr = r & 15;
                pos = T * 32 + 8 * (rr >> 2) + 4 * cg + (rr & 3);
            }
            return pos < nt ? pos : -1;
        };
        const int k_wave = wave * 64;                                   // first item of this wave
        const int n_sets = nit - k_wave > 32 ? 2 : (nit - k_wave > 0 ? 1 : 0);
        int slot[2], hmax[2];
        bool live[2];
        v4i bq[2][4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int it = k_wave + h * 32 + c;
            live[h] = it < nit;
            const v2i item = items[item0 + (live[h] ? it : nit - 1)];
            slot[h] = item.y;
            const int q = A.cand_q[cb + item.x];
            const v4i *src = reinterpret_cast<const v4i *>(A.desc + (int64_t)(qoff + q) * D);
#pragma unroll
            for (int s = 0; s < 4; ++s) bq[h][s] = ~src[2 * s + g];
            const int ub = A.d2[2 * (cb + q) + 1];
            int hm = (ub - A.norm_q[qoff + q]) >> 1;
            hm = hm < (1 << 24) ? hm : (1 << 24);
            hmax[h] = live[h] ? hm : -0x40000000;
        }
        const int8_t *tbase = A.sdesc + (int64_t)toff * D;
        int bd1[2] = {NAR_D_INVALID, NAR_D_INVALID}, bi1[2] = {NAR_D_INVALID, NAR_D_INVALID};
        int bd2[2] = {NAR_D_INVALID, NAR_D_INVALID};
        auto fetch = [&](int ph, v4i (&row16)[SUB], v4i &meta) {
#pragma unroll
            for (int j = 0; j < SUB; ++j) {
                const int pos = position(ph * SUB + j, lrow);
                row16[j] = pos >= 0 ? *reinterpret_cast<const v4i *>(tbase + (int64_t)pos * D + 16 * lchunk)
                                    : v4i{0, 0, 0, 0};
            }
            meta = v4i{NAR_HALF_INVALID, 0, NAR_D_INVALID, 0};
            if (threadIdx.x < PR) {
                const int r = threadIdx.x & 31;
                const int pos = position(ph * SUB + (threadIdx.x >> 5), r);
                const int regpos = ((r >> 3) << 2) | (r & 3);
                meta.y = regpos;
                if (pos >= 0) {
                    meta.x = A.sct[toff + pos];
                    meta.y = ((A.sn2[toff + pos] & 1) << 4) | regpos;
                    meta.z = A.sperm[toff + pos];
                }
            }
        };
        auto stage = [&](int buf, const v4i (&row16)[SUB], const v4i &meta) {
#pragma unroll
            for (int j = 0; j < SUB; ++j)
                *reinterpret_cast<v4i *>(&s_tile[buf][(j * 32 + lrow) * D + 16 * (lchunk ^ ((lrow >> 1) & 7))]) = row16[j];
            if (threadIdx.x < PR) {
                s_half[buf][threadIdx.x] = meta.x;
                s_pk[buf][threadIdx.x] = meta.y;
                s_idx[buf][threadIdx.x] = meta.z;
            }
        };
        v4i pre[SUB], pre_meta;
        const int nph = (ntiles + SUB - 1) / SUB;
        if (nph > 0) {
            fetch(0, pre, pre_meta);
            stage(0, pre, pre_meta);
        }
        __syncthreads();
        for (int ph = 0; ph < nph; ++ph) {
            const int buf = ph & 1;
            if (ph + 1 < nph) fetch(ph + 1, pre, pre_meta);
#pragma unroll
            for (int j = 0; j < SUB; ++j) {
                const int tile = ph * SUB + j;
                if (n_sets > 0 && tile < ntiles) {
                    v4i a[4];
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        a[s] = *reinterpret_cast<const v4i *>(&s_tile[buf][(j * 32 + c) * D + 16 * ((2 * s + g) ^ ((c >> 1) & 7))]);
                    v16i cin;
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) {
                        const v4i tv = *reinterpret_cast<const v4i *>(&s_half[buf][j * 32 + 8 * kk + 4 * g]);
                        cin[4 * kk] = tv.x; cin[4 * kk + 1] = tv.y; cin[4 * kk + 2] = tv.z; cin[4 * kk + 3] = tv.w;
                    }
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        if (h == 1 && n_sets < 2) break;
                        v16i acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[0], bq[h][0], cin, 0, 0, 0);
#pragma unroll
                        for (int s = 1; s < 4; ++s)
                            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], bq[h][s], acc, 0, 0, 0);
                        const int t0 = min(min(acc[0], acc[1]), acc[2]), t1 = min(min(acc[3], acc[4]), acc[5]);
                        const int t2 = min(min(acc[6], acc[7]), acc[8]), t3 = min(min(acc[9], acc[10]), acc[11]);
                        const int t4 = min(min(acc[12], acc[13]), acc[14]);
                        const int lo = min(min(min(t0, t1), t2), min(min(t3, t4), acc[15]));
                        if (__ballot(lo <= hmax[h]) == 0ull) continue;
                        v4i tk[4];
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk)
                            tk[kk] = *reinterpret_cast<const v4i *>(&s_pk[buf][j * 32 + 8 * kk + 4 * g]);
                        int m1 = 0x7FFFFFFF, m2 = 0x7FFFFFFF;
#pragma unroll
                        for (int reg = 0; reg < 16; ++reg) {
                            const int key = (int)(((unsigned)acc[reg] << 5) + (unsigned)tk[reg >> 2][reg & 3]);
                            m2 = med3_key(m1, m2, key);
                            m1 = min(m1, key);
                        }
                        const int d1k = m1 >> 4, d2k = m2 >> 4;
                        if (__ballot(d1k == d2k) == 0ull) {
                            const int r1 = m1 & 15;
                            const int i1k = s_idx[buf][j * 32 + 8 * (r1 >> 2) + 4 * g + (r1 & 3)];
                            if (d1k < bd1[h] || (d1k == bd1[h] && i1k < bi1[h])) {
                                bd2[h] = min(bd1[h], d2k);
                                bd1[h] = d1k;
                                bi1[h] = i1k;
                            } else {
                                bd2[h] = min(bd2[h], d1k);
                            }
                        } else {
                            // two equal distances among a lane's 16 rows: every row through the full
                            // (distance, original row) comparison
#pragma unroll
                            for (int reg = 0; reg < 16; ++reg) {
                                const int dk = 2 * acc[reg] + ((tk[reg >> 2][reg & 3] >> 4) & 1);
                                const int ik = s_idx[buf][j * 32 + 8 * (reg >> 2) + 4 * g + (reg & 3)];
                                if (dk < bd1[h] || (dk == bd1[h] && ik < bi1[h])) {
                                    bd2[h] = bd1[h];
                                    bd1[h] = dk;
                                    bi1[h] = ik;
                                } else {
                                    bd2[h] = min(bd2[h], dk);
                                }
                            }
                        }
                    }
                }
            }
            if (ph + 1 < nph) stage(buf ^ 1, pre, pre_meta);
            __syncthreads();
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            // the two lane halves (rows +4 of every group of eight) -> one (best, row, second)
            const int od1 = __shfl_xor(bd1[h], 32), oi1 = __shfl_xor(bi1[h], 32), od2 = __shfl_xor(bd2[h], 32);
            int f_d, f_i, s_d;
            if (od1 < bd1[h] || (od1 == bd1[h] && oi1 < bi1[h])) {
                f_d = od1; f_i = oi1;
                s_d = min(bd1[h], od2);
            } else {
                f_d = bd1[h]; f_i = bi1[h];
                s_d = min(od1, bd2[h]);
            }
            if (g == 0 && live[h] && (h == 0 || n_sets == 2)) res[slot[h]] = v4i{f_d, f_i, s_d, 0};
        }
    }
}

// merge a candidate's items, then what exact_finish does: exact squared distances, train row,
// metric, keep flag.  The pair's workgroup of symcompact_kernel runs it in front of its compaction
// (a kernel of its own until the launch count of the filter stage showed in the sweep running beside
// it); pairs the narrow stage did not take return at once.
__device__ __forceinline__ void narrow_finish_pair(const NarArgs &A, int p)
{
    const NarLayout NL = narrow_layout(A.rows_total, A.n_pairs);
    const int32_t *pair_base = reinterpret_cast<const int32_t *>(A.nar + NL.pair_base);
    const v2i *slot = reinterpret_cast<const v2i *>(A.nar + NL.slot);
    const v4i *res = reinterpret_cast<const v4i *>(A.nar + NL.res);
    if (p == 0 && threadIdx.x == 0) {                   // the scan has consumed tasks and items
        int32_t *ctl = reinterpret_cast<int32_t *>(A.nar + NL.ctl);
        ctl[0] = ctl[1] = ctl[2] = 0;
    }
    const int b0 = pair_base[p];
    if (b0 < 0) return;
    const int64_t cb = A.out_off[p];
    const int cnt = A.cand_cnt[p];
    const int qoff = A.img_off[A.pairs[2 * p]];
    for (int k = threadIdx.x; k < cnt; k += 256) {
        const v2i sl = slot[cb + k];
        int f_d = NAR_D_INVALID, f_i = NAR_D_INVALID, s_d = NAR_D_INVALID;
        for (int j = 0; j < sl.y; ++j) {
            const v4i e = res[b0 + sl.x + j];
            if (e.x < f_d || (e.x == f_d && e.y < f_i)) {
                s_d = min(f_d, e.z);
                f_d = e.x;
                f_i = e.y;
            } else {
                s_d = min(s_d, e.x);
            }
        }
        const int q = A.cand_q[cb + k];
        // (no row at all, or no second one, below 2^26: the classes of the mask hold every row that
        //  can matter, so this is a broken invariant -- flagged like an unresolved row)
        if (f_d >= (1 << 26) || s_d >= (1 << 26)) {
            atomicAdd(A.zero_div + 1, 1);
            A.cand_t[cb + k] = 0;
            A.cand_metric[cb + k] = 0.0;
            A.cand_keep[cb + k] = 0;
            continue;
        }
        const int na = A.norm_q[qoff + q];
        const int d1 = f_d + na, d2 = s_d + na;
        *reinterpret_cast<v2i *>(A.d2w + 2 * (cb + q)) = v2i{d1, d2};
        const float f0 = (float)sqrt((double)d1);
        const float f1 = (float)sqrt((double)d2);
        double mt;
        bool ok = false;
        if (f1 == 0.0f) {
            mt = __longlong_as_double(0x7FF8000000000000LL);    // python raises ZeroDivisionError
            atomicAdd(A.zero_div, 1);
        } else {
            mt = (double)f0 * ((double)f0 / (double)f1);
            ok = mt < A.thresh;
        }
        A.cand_t[cb + k] = f_i;
        A.cand_metric[cb + k] = mt;
        A.cand_keep[cb + k] = ok ? 1 : 0;
    }
}

// in-place, order-preserving compaction of every pair's candidate list to its survivors
// (no __restrict__: narrow_finish_pair writes cand_t / cand_metric / cand_keep through N first)
__global__ __launch_bounds__(256) void symcompact_kernel(const int64_t *cand_off,
                                                         const int32_t *cand_cnt,
                                                         const uint8_t *cand_keep,
                                                         int32_t *q, int32_t *t,
                                                         double *metric,
                                                         int32_t *surv_cnt,
                                                         int32_t *task_total, NarArgs N)
{
    __shared__ int wcnt[4];
    const int p = blockIdx.x;
    // a pair without a candidate has no survivor, nothing to merge and nothing to compact: it leaves
    // before any barrier (pair 0 still resets the lists and the narrow stage's control words)
    if (cand_cnt[p] == 0) {
        if (threadIdx.x == 0) {
            surv_cnt[p] = 0;
            if (p == 0) {
                task_total[0] = task_total[1] = 0;
                if (N.nar != nullptr) {
                    int32_t *ctl = reinterpret_cast<int32_t *>(N.nar + narrow_layout(N.rows_total, N.n_pairs).ctl);
                    ctl[0] = ctl[1] = ctl[2] = 0;
                }
            }
        }
        return;
    }
    if (N.nar != nullptr) {
        narrow_finish_pair(N, p);
        __threadfence_block();
        __syncthreads();
    }
    const int64_t b = cand_off[p];
    const int cnt = cand_cnt[p];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int out = 0;
    for (int base = 0; base < cnt; base += 256) {
        const int i = base + threadIdx.x;
        const bool k = i < cnt && cand_keep[b + i];
        int vq = 0, vt = 0;
        double vm = 0.0;
        if (k) { vq = q[b + i]; vt = t[b + i]; vm = metric[b + i]; }
        const unsigned long long mask = __ballot(k);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[wave] = __popcll(mask);
        __syncthreads();                       // every read of this block precedes its writes
        int woff = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) woff += wcnt[w];
            tot += wcnt[w];
        }
        if (k) {
            const int64_t o = b + out + woff + before;
            q[o] = vq; t[o] = vt; metric[o] = vm;
        }
        out += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        surv_cnt[p] = out;
        if (p == 0) task_total[0] = task_total[1] = 0;   // the exact stage has consumed the lists
    }
}

}  // namespace

// =====================================================================================
// C ABI
// =====================================================================================
extern "C" int64_t iamx_desc3_rows_cap(int64_t n_rows)
{
    if (n_rows <= 0) return 0;
    return (n_rows + CHUNK - 1) / CHUNK * CHUNK;
}

extern "C" int iamx_knn2sym_rows_per_wg(int form)
{
    return form == 2 ? 1024 : (form == 1 ? 512 : (form == 0 ? 256 : 0));
}

template <typename SRC>
static int pack3_launch(Pack3Args P, int64_t total_rows, int max_rows, void *stream, const char *what)
{
    hipStream_t st = iamx::as_stream(stream);
    if (total_rows <= 0 || max_rows <= 0) return IAMX_OK;
    const int cap = (max_rows + CHUNK - 1) / CHUNK * CHUNK;
    hipLaunchKernelGGL(pack3_rows_kernel<SRC>, dim3((unsigned)((total_rows * 8 + 255) / 256)),
                       dim3(256), 0, st, P, total_rows);
    // (few, large images: split every row group's comparisons so that the launch fills the chip)
    const int64_t groups = (int64_t)((max_rows + 255) / 256) * P.n_img;
    int split = 1;
    while (split < 32 && groups * split < 2048 && max_rows > 1024 * split) split *= 2;
    if (split > 1) (void)hipMemsetAsync(P.pos, 0, (size_t)total_rows * sizeof(int32_t), st);
    hipLaunchKernelGGL(pack3_rank_bins_kernel, dim3((unsigned)P.n_img), dim3(1024), 0, st, P);
    hipLaunchKernelGGL(pack3_rank_kernel,
                       dim3((unsigned)((max_rows + 255) / 256), (unsigned)P.n_img, (unsigned)split),
                       dim3(256), 0, st, P);
    hipLaunchKernelGGL(pack3_scatter_kernel<SRC>,
                       dim3((unsigned)(((int64_t)cap * 8 + 255) / 256), (unsigned)P.n_img),
                       dim3(256), 0, st, P);
    return iamx::check_launch(what);
}

template <typename SRC>
static int pack3_single(const SRC *src, int64_t n_rows, int8_t *dst, int32_t *sn2, int32_t *sct,
                        int32_t *sperm, int32_t *sinv, int32_t *scratch, void *stream,
                        const char *what)
{
    if (n_rows < 0 || n_rows > (1 << 24) || (n_rows > 0 && !src) || !dst || !sn2 || !sct || !sperm ||
        !sinv || !scratch)
        return iamx::fail(IAMX_EINVAL, "%s: null pointer or bad row count", what);
    Pack3Args P{src, nullptr, n_rows, nullptr, dst, sn2, sct, sperm, sinv,
                scratch, scratch + n_rows, scratch + 2 * n_rows, 1};
    return pack3_launch<SRC>(P, n_rows, (int)n_rows, stream, what);
}

extern "C" int iamx_desc3_pack_u8(const uint8_t *src, int64_t n_rows, int8_t *dst, int32_t *sn2,
                                  int32_t *sct, int32_t *sperm, int32_t *sinv, int32_t *scratch,
                                  void *stream)
{
    return pack3_single(src, n_rows, dst, sn2, sct, sperm, sinv, scratch, stream, "iamx_desc3_pack_u8");
}

extern "C" int iamx_desc3_pack_f32(const float *src, int64_t n_rows, int8_t *dst, int32_t *sn2,
                                   int32_t *sct, int32_t *sperm, int32_t *sinv, int32_t *scratch,
                                   void *stream)
{
    return pack3_single(src, n_rows, dst, sn2, sct, sperm, sinv, scratch, stream, "iamx_desc3_pack_f32");
}

extern "C" int iamx_desc3_pack_batch_u8(const uint8_t *src, const int64_t *src_off,
                                        const int32_t *dst_off, int n_img, int64_t total_rows,
                                        int max_rows_per_image, int8_t *dst, int32_t *sn2,
                                        int32_t *sct, int32_t *sperm, int32_t *sinv,
                                        int32_t *scratch, void *stream)
{
    IAMX_REQUIRE(src && src_off && dst_off && dst && sn2 && sct && sperm && sinv && scratch,
                 "null pointer");
    IAMX_REQUIRE(n_img > 0 && total_rows >= 0 && max_rows_per_image >= 0, "bad count");
    Pack3Args P{src, src_off, 0, dst_off, dst, sn2, sct, sperm, sinv,
                scratch, scratch + total_rows, scratch + 2 * total_rows, n_img};
    return pack3_launch<uint8_t>(P, total_rows, max_rows_per_image, stream, "iamx_desc3_pack_batch_u8");
}

// template arguments of the shipped sweep, one place for the launch and for iamx_knn2sym_kernel_id()
// (form 2: eight query blocks per wave, ONE wave per SIMD, B operand in AGPRs -- see the kernel and
//  profiles/r3_knn2sym_onewave.txt; compiled with -mllvm -amdgpu-mfma-vgpr-form, csrc/build.sh)
#define SWEEP_FORM2 8, 4, 0, 5, 2, 0, true, 128, 1
#define SWEEP_FORM1 4, 4, 0, 6, 2, 0, true, 128, 2
#define SWEEP_FORM0 2, 4, 0, 6, 2, 0, true, 128, 2
#define SWEEP_ITEMS2 8, 4, 1, 5, 2, 0, true, 128, 1      // form 2 walking items (VARIANT 1)
#define SWEEP_STR2(...) #__VA_ARGS__
#define SWEEP_STR(...) SWEEP_STR2(__VA_ARGS__)

#if defined(IAMX_T_STAMPS)
// the diagnostic build's stamp buffer ([workgroups][4 waves][4] u64 of the next launches; NULL: none)
static unsigned long long *g_sweep_stamps = nullptr;
extern "C" int iamx_knn2sym_set_stamps(void *buf)
{
    g_sweep_stamps = static_cast<unsigned long long *>(buf);
    return IAMX_OK;
}
#define SWEEP_STAMPS_ARG , g_sweep_stamps
#else
#define SWEEP_STAMPS_ARG
#endif

extern "C" const char *iamx_knn2sym_kernel_id(int form)
{
    switch (form) {
    case 2: return "knn2sym_kernel<" SWEEP_STR(SWEEP_ITEMS2) ">";     // (PairBatch: the item entry)
    case 1: return "knn2sym_kernel<" SWEEP_STR(SWEEP_FORM1) ">";
    case 0: return "knn2sym_kernel<" SWEEP_STR(SWEEP_FORM0) ">";
    default: return "";
    }
}

extern "C" int iamx_knn2sym_sweep(const int8_t *sdesc, const int32_t *sn2, const int32_t *sct,
                                  const int32_t *img_off, const int32_t *img_n,
                                  const int32_t *upairs, const int32_t *wg_off,
                                  const int64_t *col_off, const int64_t *rowp_off, int n_u,
                                  int total_wg, int form, int32_t *col, int32_t *rowp,
                                  uint8_t *colmask, void *stream)
{
    IAMX_REQUIRE(sdesc && sn2 && sct && img_off && img_n && upairs && wg_off && col_off && rowp_off &&
                     col && rowp,
                 "null pointer");
    IAMX_REQUIRE(n_u >= 0 && total_wg >= 0, "negative count");
    IAMX_REQUIRE(form >= 0 && form <= 2, "form must be 0 (256 rows), 1 (512) or 2 (1024)");
    if (n_u == 0 || total_wg == 0) return IAMX_OK;
    SymArgs a{sdesc, sn2, sct, img_off, img_n, upairs, wg_off, col_off, rowp_off, col, rowp, n_u, total_wg,
              colmask SWEEP_STAMPS_ARG};
    const dim3 g((unsigned)total_wg);
    hipStream_t st = iamx::as_stream(stream);
    // PIPE = 6: six epilogue VALU instructions beside every MFMA of the next pair of query
    // blocks (profiles/r2_knn2sym_ablate.txt: 1.83 -> 1.78 us per image pair)
    if (form == 2) hipLaunchKernelGGL((knn2sym_kernel<SWEEP_FORM2>), g, dim3(256), 0, st, a);
    else if (form == 1) hipLaunchKernelGGL((knn2sym_kernel<SWEEP_FORM1>), g, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((knn2sym_kernel<SWEEP_FORM0>), g, dim3(256), 0, st, a);
    return iamx::check_launch("iamx_knn2sym_sweep");
}

extern "C" int iamx_knn2sym_sweep_items(const int8_t *sdesc, const int32_t *sn2, const int32_t *sct,
                                        const int32_t *img_off, const int32_t *img_n,
                                        const int32_t *upairs, const int32_t *items,
                                        const int64_t *col_off, const int64_t *rowp_off, int n_u,
                                        int n_items, int32_t *col, int32_t *rowp, uint8_t *colmask,
                                        void *stream)
{
    IAMX_REQUIRE(sdesc && sn2 && sct && img_off && img_n && upairs && items && col_off && rowp_off &&
                     col && rowp,
                 "null pointer");
    IAMX_REQUIRE(n_u >= 0 && n_items >= 0, "negative count");
    if (n_u == 0 || n_items == 0) return IAMX_OK;
    // (the item walk reads its table through wg_off, its count through total_wg)
    SymArgs a{sdesc, sn2, sct, img_off, img_n, upairs, items, col_off, rowp_off, col, rowp, n_u, n_items,
              colmask SWEEP_STAMPS_ARG};
    hipLaunchKernelGGL((knn2sym_kernel<SWEEP_ITEMS2>), dim3((unsigned)n_items), dim3(256), 0,
                       iamx::as_stream(stream), a);
    return iamx::check_launch("iamx_knn2sym_sweep_items");
}

// the item walk on v_mfma_i32_16x16x64_i8 (knn2sym16_kernel): the arguments and the outputs of
// iamx_knn2sym_sweep_items, bit for bit
#define SWEEP16_PIPE 2
extern "C" const char *iamx_knn2sym_items16_kernel_id(void)
{
    return "knn2sym16_kernel<" SWEEP_STR(SWEEP16_PIPE) ">";
}

extern "C" int iamx_knn2sym_sweep_items16(const int8_t *sdesc, const int32_t *sn2, const int32_t *sct,
                                          const int32_t *img_off, const int32_t *img_n,
                                          const int32_t *upairs, const int32_t *items,
                                          const int64_t *col_off, const int64_t *rowp_off, int n_u,
                                          int n_items, int32_t *col, int32_t *rowp, uint8_t *colmask,
                                          void *stream)
{
    IAMX_REQUIRE(sdesc && sn2 && sct && img_off && img_n && upairs && items && col_off && rowp_off &&
                     col && rowp,
                 "null pointer");
    IAMX_REQUIRE(n_u >= 0 && n_items >= 0, "negative count");
    if (n_u == 0 || n_items == 0) return IAMX_OK;
    SymArgs a{sdesc, sn2, sct, img_off, img_n, upairs, items, col_off, rowp_off, col, rowp, n_u, n_items,
              colmask SWEEP_STAMPS_ARG};
    // (dynamic LDS above the 64 KB a launch gets by default: raised where a thread first launches on a device;
    //  setting the same value again, from another thread, is harmless)
    static thread_local int raised_dev = -1;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess)
        return iamx::fail(IAMX_ELAUNCH, "iamx_knn2sym_sweep_items16: no current device");
    if (dev != raised_dev) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&knn2sym16_kernel<SWEEP16_PIPE>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, SWEEP16_LDS_BYTES);
        if (e != hipSuccess)
            return iamx::fail(IAMX_ELAUNCH, "iamx_knn2sym_sweep_items16: dynamic LDS: %s", hipGetErrorString(e));
        raised_dev = dev;
    }
    hipLaunchKernelGGL((knn2sym16_kernel<SWEEP16_PIPE>), dim3((unsigned)n_items), dim3(256), SWEEP16_LDS_BYTES,
                       iamx::as_stream(stream), a);
    return iamx::check_launch("iamx_knn2sym_sweep_items16");
}

// IAMX_EXACT_NARROW=0: every candidate through the full scan (A/B, tests)
static bool narrow_enabled()
{
    const char *e = getenv("IAMX_EXACT_NARROW");
    return !(e && e[0] == '0');
}

extern "C" int64_t iamx_knn2sym_narrow_bytes(int64_t rows, int n_pairs)
{
    if (rows <= 0 || n_pairs <= 0) return 0;
    return narrow_layout(rows, n_pairs).total;
}

extern "C" int iamx_knn2sym_candidates(const int32_t *sn2, const int32_t *sperm,
                                       const int32_t *img_off, const int32_t *img_n,
                                       const int32_t *pairs, const int32_t *osrc,
                                       const int32_t *wg_off, const int64_t *col_off,
                                       const int64_t *rowp_off, const int64_t *out_off,
                                       const int32_t *col, const int32_t *rowp, int n_pairs,
                                       double thresh, uint8_t *keep, int32_t *cand_cnt,
                                       int32_t *cand_q, int32_t *task_total, int32_t *tasks,
                                       int32_t *d2, const uint8_t *colmask, void *nar,
                                       int64_t rows_total, int max_query_rows, int form, void *stream)
{
    IAMX_REQUIRE(sn2 && sperm && img_off && img_n && pairs && osrc && wg_off && col_off && rowp_off &&
                     out_off && col && rowp && keep && cand_cnt && cand_q && task_total && tasks && d2,
                 "null pointer");
    IAMX_REQUIRE(!nar || colmask, "narrow workspace without colmask");
    IAMX_REQUIRE(form >= 0 && form <= 2, "form must be 0, 1 or 2");
    if (n_pairs <= 0) return IAMX_OK;
    CandArgs a{sn2, sperm, img_off, img_n, pairs, osrc, wg_off, col_off, rowp_off, out_off, col, rowp,
               thresh, sym_cand_K(thresh), keep, cand_cnt, cand_q, task_total, tasks, d2, 8,
               colmask, narrow_enabled() ? static_cast<int8_t *>(nar) : nullptr, rows_total, n_pairs,
               iamx_knn2sym_rows_per_wg(form)};
    IAMX_REQUIRE(rows_total > 0 && rows_total < (1ll << 31), "rows_total = rows of all ordered pairs");
    IAMX_REQUIRE(max_query_rows > 0, "max_query_rows = rows of the largest query image");
    // (the keep map and the pairs' candidate counts in ONE launch: every launch of this stage shows in
    //  the sweep running beside it)
    const int64_t keep_words = (rows_total + 31) / 32;
    const int64_t clear_wg = (keep_words + 4095) / 4096;
    hipLaunchKernelGGL(symcand_clear_kernel, dim3((unsigned)(clear_wg < 256 ? clear_wg : 256)), dim3(256), 0,
                       iamx::as_stream(stream), reinterpret_cast<unsigned *>(keep), keep_words, cand_cnt, n_pairs);
    hipLaunchKernelGGL(symcand_rows_kernel,
                       dim3((unsigned)((max_query_rows + 1023) / 1024), (unsigned)(n_pairs < 65535 ? n_pairs : 65535)),
                       dim3(256), 0, iamx::as_stream(stream), a);
    hipLaunchKernelGGL(symcand_kernel, dim3((unsigned)n_pairs), dim3(256), 0, iamx::as_stream(stream), a);
    return iamx::check_launch("iamx_knn2sym_candidates");
}

extern "C" int iamx_knn2sym_exact(const int8_t *desc, const int32_t *norm_q, const int32_t *norm_t,
                                  int32_t *key_t, int64_t total_rows,
                                  const int32_t *img_off, const int32_t *img_n, const int32_t *pairs,
                                  const int64_t *out_off, const int32_t *cand_cnt,
                                  int32_t *task_total, const int32_t *tasks, int32_t *cand_q,
                                  int n_pairs, double thresh, int32_t *d2, int32_t *cand_t,
                                  double *cand_metric, uint8_t *cand_keep, int32_t *surv_cnt,
                                  int32_t *zero_div, const int8_t *sdesc, const int32_t *sn2,
                                  const int32_t *sct, const int32_t *sperm, const int32_t *img_off3,
                                  const int32_t *osrc, void *nar, int64_t rows_total, int form,
                                  void *stream)
{
    IAMX_REQUIRE(desc && norm_q && norm_t && key_t && img_off && img_n && pairs && out_off && cand_cnt &&
                     task_total && tasks && cand_q && d2 && cand_t && cand_metric && cand_keep &&
                     surv_cnt && zero_div,
                 "null pointer");
    IAMX_REQUIRE(total_rows >= 0, "negative row count");
    if (n_pairs <= 0) return IAMX_OK;
    hipStream_t st = iamx::as_stream(stream);
    // (46 MB each way for the 2812-image store of configs[2]: ~20 us beside a 7 ms round; rebuilt
    //  every call, so the keys can never be stale against a re-packed store)
    if (total_rows > 0) {
        int64_t gk = (total_rows + 255) / 256;
        hipLaunchKernelGGL(symexact_keys_kernel, dim3((unsigned)(gk > 4096 ? 4096 : gk)), dim3(256), 0, st,
                           norm_t, total_rows, key_t);
    }
    ExactArgs a{desc, norm_q, norm_t, key_t, n_pairs, img_off, img_n, pairs, out_off, cand_cnt, cand_q,
                task_total, tasks, thresh, d2, cand_t, cand_metric, cand_keep, zero_div};
    hipLaunchKernelGGL(symexact_kernel, dim3(1024), dim3(256), 0, st, a);       // pairs with <= 64 candidates
    // the others, 256 per workgroup (IAMX_EXACT_PRUNE=0: the unpruned scan, for A/B and tests)
    const char *prune = getenv("IAMX_EXACT_PRUNE");
    if (prune && prune[0] == '0')
        hipLaunchKernelGGL((symexact_wg_kernel<false, 1>), dim3(2048), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((symexact_wg_kernel<true, 2>), dim3(2048), dim3(256), 0, st, a);
    NarArgs nfin{};                                      // (nar == NULL: symcompact_kernel has nothing to merge)
    if (nar && narrow_enabled()) {
        // (the same switch and the same buffer as iamx_knn2sym_candidates: pairs it bucketed have
        //  no task in the two lists above)
        if (!(sdesc && sn2 && sct && sperm && img_off3 && osrc && rows_total > 0 && form >= 0 && form <= 2))
            return iamx::fail(IAMX_EINVAL, "iamx_knn2sym_exact: narrow workspace without the sorted store");
        NarArgs na{desc, norm_q, img_off, pairs, osrc, out_off, cand_q, d2, sdesc, sn2, sct, sperm, img_off3,
                   img_n, static_cast<int8_t *>(nar), rows_total, n_pairs, iamx_knn2sym_rows_per_wg(form),
                   cand_cnt, thresh, d2, cand_t, cand_metric, cand_keep, zero_div};
        hipLaunchKernelGGL(symnarrow_kernel<3>, dim3(768), dim3(256), 0, st, na);
        nfin = na;
    }
    hipLaunchKernelGGL(symcompact_kernel, dim3((unsigned)n_pairs), dim3(256), 0, st, out_off,
                       cand_cnt, cand_keep, cand_q, cand_t, cand_metric, surv_cnt, task_total, nfin);
    return iamx::check_launch("iamx_knn2sym_exact");
}
