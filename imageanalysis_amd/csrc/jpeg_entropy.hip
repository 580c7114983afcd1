// Device entropy decoder for baseline JPEG (the missing half of csrc/jpeg.hip's split decoder):
// the Huffman-coded scan is decoded on gfx950 into exactly the int16 [blocks][64] coefficients
// iamx_jpeg_decode_coefficients writes on the host, so iamx_jpeg_reconstruct consumes them
// unchanged.  Method, state and the proof that the result is exact or refused: jpeg_entropy.h (the
// per-symbol routine there is shared with the host driver under tools/).  Here: one lane per
// sub-sequence (128 bytes or more), 256 lanes per workgroup, the flat header (six Huffman tables in
// look-up form, geometry) staged in LDS once per workgroup, the scan read in 16-byte pieces.
//   jpeg_sync_pass      one pass of the synchronisation (launched max_passes times; a pass that
//                       finds the previous one changed nothing returns at once)
//   jpeg_count_partial  per-workgroup sums of the completed-block counts
//   jpeg_top_scan       exclusive (segmented) scan of per-workgroup aggregates, one workgroup
//   jpeg_write_pass     decode from the verified states, store coefficients (DC as differences)
//   jpeg_dc_scan<false / true>   segmented integer scan of the DC differences per component:
//                       per-workgroup aggregates, then (behind jpeg_top_scan) the prediction
//   jpeg_finish         the status word
// No launch waits for another workgroup; the phases are ordered by the stream alone.  The call
// validates the geometry of the host header; it trusts the six tables in it and that d_header is
// a copy of it (a header of iamx_jpeg_entropy_prepare, unchanged, is the caller's contract).
#include "iamx_common.h"
#include "jpeg_entropy.h"

namespace {

using namespace iamx_jpeg;

constexpr int LANES = 256;
constexpr int CTRL_WORDS = 64;             // changed[0 .. MAX_PASSES), then:
constexpr int CTRL_FLAGS = MAX_PASSES;     // damaged
constexpr int CTRL_TOTAL = MAX_PASSES + 1; // blocks completed by all lanes
constexpr int CTRL_DECODED = MAX_PASSES + 2;   // sub-sequences decoded by the sync passes, all together
static_assert(MAX_PASSES + 3 <= CTRL_WORDS, "control words");
static_assert(sizeof(ScanHeader) % 16 == 0, "header is copied in 16-byte pieces");

__device__ __forceinline__ void stage_header(ScanHeader *dst, const ScanHeader *src)
{
    const uint4 *s = reinterpret_cast<const uint4 *>(src);
    uint4 *d = reinterpret_cast<uint4 *>(dst);
    for (int i = threadIdx.x; i < (int)(sizeof(ScanHeader) / 16); i += LANES) d[i] = s[i];
    __syncthreads();
}

// inclusive segmented scan over the workgroup: (f, v) o (g, w) = g ? (g, w) : (f, v + w)
__device__ __forceinline__ int2 wg_segscan(int f, int v, int *sf, int *sv)
{
    const int t = threadIdx.x;
    sf[t] = f;
    sv[t] = v;
    __syncthreads();
    for (int d = 1; d < LANES; d <<= 1) {
        int lf = 0, lv = 0;
        if (t >= d) {
            lf = sf[t - d];
            lv = sv[t - d];
        }
        __syncthreads();
        if (t >= d && !f) {
            v = (int)((unsigned)v + (unsigned)lv);
            f = lf;
        }
        sf[t] = f;
        sv[t] = v;
        __syncthreads();
    }
    return make_int2(f, v);
}

__global__ __launch_bounds__(LANES) void jpeg_sync_pass(const uint8_t *__restrict__ data,
                                                        const ScanHeader *__restrict__ gh, int pass,
                                                        const uint2 *__restrict__ prev,
                                                        uint2 *__restrict__ cur,
                                                        uint2 *__restrict__ inused,
                                                        uint32_t *__restrict__ cnt, uint32_t *ctrl)
{
    __shared__ ScanHeader H;
    if (pass >= 2 && ctrl[pass - 1] == 0) return;          // (uniform) already a fixed point
    stage_header(&H, gh);
    const uint32_t i = blockIdx.x * LANES + threadIdx.x;
    if (i >= (uint32_t)H.n_subseq) return;
    const uint32_t endpos = i + 1 == (uint32_t)H.n_subseq ? NO_END : (i + 1) * (8u * (uint32_t)H.subseq_bytes);
    State in, out, before;
    before.pos = before.bk = COLD_INPUT;
    if (pass == 0) {
        Reader R;
        reader_init(R, &H, data);
        in = cold_state(R, i, (uint32_t)H.subseq_bytes);
    } else {
        in.pos = in.bk = 0;
        if (i > 0) {
            const uint2 s = prev[i - 1];
            in.pos = s.x;
            in.bk = s.y;
        }
        const uint2 s = prev[i];
        before.pos = s.x;
        before.bk = s.y;
    }
    bool decode = true;
    if (pass >= 2) {
        const uint2 u = inused[i];
        decode = !(u.x == in.pos && u.y == in.bk);
    }
    if (decode) {
        uint32_t n;
        bool damaged;
        decode_lane<false>(&H, data, in, endpos, 0u, nullptr, 0, out, n, damaged);
        cnt[i] = n;
        atomicAdd(&ctrl[CTRL_DECODED], 1u);
        inused[i] = pass == 0 ? make_uint2(COLD_INPUT, COLD_INPUT) : make_uint2(in.pos, in.bk);
    } else {
        out = before;
    }
    cur[i] = make_uint2(out.pos, out.bk);
    if (pass > 0 && !same(out, before)) atomicAdd(&ctrl[pass], 1u);
}

__global__ __launch_bounds__(LANES) void jpeg_count_partial(const uint32_t *__restrict__ cnt, int n,
                                                            int2 *__restrict__ carry)
{
    __shared__ int sf[LANES], sv[LANES];
    const int i = blockIdx.x * LANES + threadIdx.x;
    const int2 r = wg_segscan(0, i < n ? (int)cnt[i] : 0, sf, sv);
    if (threadIdx.x == LANES - 1) carry[blockIdx.x] = make_int2(0, r.y);
}

struct ScanRanges {
    int off[4], n[4];
};

// aggregates -> exclusive carries in place; workgroup g works on [off[g], off[g] + n[g])
__global__ __launch_bounds__(LANES) void jpeg_top_scan(int2 *__restrict__ agg, ScanRanges rg,
                                                       uint32_t *total_out)
{
    __shared__ int sf[LANES], sv[LANES];
    const int n = rg.n[blockIdx.x];
    int2 *a = agg + rg.off[blockIdx.x];
    const int per = (n + LANES - 1) / LANES;
    const int lo = min(n, (int)threadIdx.x * per), hi = min(n, lo + per);
    int f = 0, v = 0;
    for (int j = lo; j < hi; ++j) {
        const int2 e = a[j];
        if (e.x) { f = 1; v = e.y; } else v = (int)((unsigned)v + (unsigned)e.y);
    }
    const int2 inc = wg_segscan(f, v, sf, sv);
    __syncthreads();
    sf[threadIdx.x] = inc.x;
    sv[threadIdx.x] = inc.y;
    __syncthreads();
    f = 0;
    v = 0;
    if (threadIdx.x > 0) {
        f = sf[threadIdx.x - 1];
        v = sv[threadIdx.x - 1];
    }
    for (int j = lo; j < hi; ++j) {
        const int2 e = a[j];
        a[j] = make_int2(f, v);
        if (e.x) { f = 1; v = e.y; } else v = (int)((unsigned)v + (unsigned)e.y);
    }
    if (total_out && threadIdx.x == LANES - 1) *total_out = (uint32_t)inc.y;
}

__global__ __launch_bounds__(LANES) void jpeg_write_pass(const uint8_t *__restrict__ data,
                                                         const ScanHeader *__restrict__ gh,
                                                         const uint2 *__restrict__ fin,
                                                         const uint32_t *__restrict__ cnt,
                                                         const int2 *__restrict__ carry,
                                                         int16_t *__restrict__ coef,
                                                         int64_t coef_blocks, uint32_t *ctrl)
{
    __shared__ ScanHeader H;
    __shared__ int sf[LANES], sv[LANES];
    if (ctrl[gh->max_passes - 1] != 0) return;             // (uniform) not verified: write nothing
    stage_header(&H, gh);
    const uint32_t i = blockIdx.x * LANES + threadIdx.x;
    const bool on = i < (uint32_t)H.n_subseq;
    const int mine = on ? (int)cnt[i] : 0;
    const int2 inc = wg_segscan(0, mine, sf, sv);
    if (!on) return;
    const uint32_t blk = (uint32_t)carry[blockIdx.x].y + (uint32_t)inc.y - (uint32_t)mine;
    const uint32_t endpos = i + 1 == (uint32_t)H.n_subseq ? NO_END : (i + 1) * (8u * (uint32_t)H.subseq_bytes);
    State in, out;
    in.pos = in.bk = 0;
    if (i > 0) {
        const uint2 s = fin[i - 1];
        in.pos = s.x;
        in.bk = s.y;
    }
    uint32_t n;
    bool damaged;
    decode_lane<true>(&H, data, in, endpos, blk, coef, coef_blocks, out, n, damaged);
    if (damaged) atomicOr(&ctrl[CTRL_FLAGS], 1u);
}

struct DcPlan {
    int chunk_off[4];                      // first chunk of component c; [ncomp] = all chunks
};

// element e of component c in scan order: where its DC value lives, whether a restart interval
// starts there
__device__ __forceinline__ int64_t dc_element(const ScanHeader *gh, int c, int e, int &flag)
{
    const int h = gh->comp_h[c], v = gh->comp_v[c], hv = h * v;
    const int m = e / hv, j = e - m * hv;
    const int by = j / h, bx = j - by * h;
    const int my = m / gh->mcus_x, mx = m - my * gh->mcus_x;
    flag = gh->restart > 0 && j == 0 && m % gh->restart == 0;
    return ((int64_t)gh->comp_base[c] + (int64_t)(my * v + by) * gh->comp_bw[c] + mx * h + bx) * 64;
}

template <bool APPLY>
__global__ __launch_bounds__(LANES) void jpeg_dc_scan(int16_t *__restrict__ coef, int64_t coef_blocks,
                                                      const ScanHeader *__restrict__ gh, DcPlan plan,
                                                      int2 *__restrict__ agg, const uint32_t *ctrl)
{
    __shared__ int sf[LANES], sv[LANES];
    if (ctrl[gh->max_passes - 1] != 0) return;
    const int g = blockIdx.x;
    int c = 0;
    if (gh->ncomp > 1 && g >= plan.chunk_off[1]) c = g >= plan.chunk_off[2] ? 2 : 1;
    const int e = (g - plan.chunk_off[c]) * LANES + threadIdx.x;
    const int ne = gh->n_mcus * gh->comp_h[c] * gh->comp_v[c];
    int flag = 0, val = 0;
    int64_t at = -1;
    if (e < ne) {
        at = dc_element(gh, c, e, flag);
        if (at < 0 || at / 64 >= coef_blocks || at / 64 >= gh->total_blocks) at = -1;
        if (at >= 0) val = coef[at];
    }
    const int2 inc = wg_segscan(flag, val, sf, sv);
    if (!APPLY) {
        if (threadIdx.x == LANES - 1) agg[g] = inc;
    } else if (at >= 0) {
        const int2 cr = agg[g];
        const int sum = inc.x ? inc.y : (int)((unsigned)inc.y + (unsigned)cr.y);
        coef[at] = (int16_t)sum;
    }
}

__global__ void jpeg_finish(const ScanHeader *__restrict__ gh, const uint32_t *__restrict__ ctrl,
                            int32_t *__restrict__ status)
{
    const int P = gh->max_passes;
    int passes = P;
    for (int j = 1; j < P; ++j)
        if (ctrl[j] == 0) { passes = j; break; }
    status[1] = passes;
    status[2] = (int32_t)ctrl[CTRL_DECODED];
    status[3] = 0;
    if (ctrl[P - 1] != 0)
        status[0] = ST_NOT_SYNCED;
    else
        status[0] = (ctrl[CTRL_FLAGS] || ctrl[CTRL_TOTAL] != (uint32_t)gh->total_blocks) ? ST_DAMAGED : ST_SYNCED;
}

inline int64_t up256(int64_t x) { return (x + 255) / 256 * 256; }

struct Layout {
    int64_t ctrl, state_a, state_b, inused, cnt, carry, dcagg, bytes;
    int n, n_wg, dc_chunks[3], dc_total;
};

bool header_ok(const ScanHeader *h)
{
    if (h->magic != HEADER_MAGIC) return false;
    if (h->ncomp != 1 && h->ncomp != 3) return false;
    if (h->blocks_per_mcu < 1 || h->blocks_per_mcu > MAX_MCU_BLOCKS) return false;
    if (h->mcus_x < 1 || h->mcus_y < 1 || h->n_mcus != h->mcus_x * h->mcus_y) return false;
    if (h->total_blocks < 1 || h->restart < 0) return false;
    if (h->scan_len < 1 || h->scan_len > MAX_SCAN_BYTES) return false;
    if ((uint64_t)h->scan_off + h->scan_len > h->file_len) return false;
    const int S = h->subseq_bytes;
    if (S < MIN_SUBSEQ_BYTES || S > MAX_SUBSEQ_BYTES || (S & (S - 1))) return false;
    if (h->n_subseq != (int)((h->scan_len + (uint32_t)S - 1) / (uint32_t)S)) return false;
    if (h->max_passes < 2 || h->max_passes > MAX_PASSES) return false;
    int64_t blocks = 0;
    for (int c = 0; c < h->ncomp; ++c) {
        if (h->comp_h[c] < 1 || h->comp_h[c] > 2 || h->comp_v[c] < 1 || h->comp_v[c] > 2) return false;
        if (h->comp_bw[c] != h->mcus_x * h->comp_h[c] || h->comp_base[c] != blocks) return false;
        blocks += (int64_t)h->comp_bw[c] * h->mcus_y * h->comp_v[c];
    }
    if (blocks != h->total_blocks) return false;
    for (int b = 0; b < h->blocks_per_mcu; ++b) {
        const int c = h->mcu_comp[b];
        if (c < 0 || c >= h->ncomp || h->mcu_bx[b] < 0 || h->mcu_bx[b] >= h->comp_h[c] ||
            h->mcu_by[b] < 0 || h->mcu_by[b] >= h->comp_v[c])
            return false;
    }
    for (int k = 0; k < 64; ++k)
        if (h->natural[k] > 63) return false;
    return true;
}

Layout layout(const ScanHeader *h)
{
    Layout L;
    L.n = h->n_subseq;
    L.n_wg = (L.n + LANES - 1) / LANES;
    L.dc_total = 0;
    for (int c = 0; c < 3; ++c) {
        L.dc_chunks[c] = c < h->ncomp ? (h->n_mcus * h->comp_h[c] * h->comp_v[c] + LANES - 1) / LANES : 0;
        L.dc_total += L.dc_chunks[c];
    }
    int64_t o = 0;
    L.ctrl = o;    o += up256(CTRL_WORDS * 4);
    L.state_a = o; o += up256((int64_t)L.n * 8);
    L.state_b = o; o += up256((int64_t)L.n * 8);
    L.inused = o;  o += up256((int64_t)L.n * 8);
    L.cnt = o;     o += up256((int64_t)L.n * 4);
    L.carry = o;   o += up256((int64_t)L.n_wg * 8);
    L.dcagg = o;   o += up256((int64_t)L.dc_total * 8);
    L.bytes = o;
    return L;
}

}  // namespace

extern "C" int64_t iamx_jpeg_entropy_workspace_bytes(const void *header)
{
    const ScanHeader *h = static_cast<const ScanHeader *>(header);
    if (!h || !header_ok(h)) return 0;
    return layout(h).bytes;
}

extern "C" int iamx_jpeg_entropy_decode(const uint8_t *data, int64_t data_bytes, const void *header,
                                        const void *d_header, void *workspace, int64_t workspace_bytes,
                                        int16_t *coef, int64_t coef_blocks, int32_t *status,
                                        void *stream)
{
    IAMX_REQUIRE(data && header && d_header && workspace && coef && status, "null pointer");
    const ScanHeader *h = static_cast<const ScanHeader *>(header);
    IAMX_REQUIRE(header_ok(h), "not a header of iamx_jpeg_entropy_prepare");
    IAMX_REQUIRE(((uintptr_t)data & 15) == 0 && ((uintptr_t)d_header & 15) == 0 &&
                     ((uintptr_t)workspace & 15) == 0,
                 "data, header and workspace must be 16-byte aligned");
    IAMX_REQUIRE(data_bytes >= ((int64_t)h->file_len + 15) / 16 * 16,
                 "file buffer too small (the file length rounded up to 16 bytes)");
    IAMX_REQUIRE(coef_blocks >= h->total_blocks, "coefficient buffer too small (info[11])");
    const Layout L = layout(h);
    IAMX_REQUIRE(workspace_bytes >= L.bytes, "workspace too small");
    hipStream_t st = iamx::as_stream(stream);
    char *ws = static_cast<char *>(workspace);
    uint32_t *ctrl = reinterpret_cast<uint32_t *>(ws + L.ctrl);
    uint2 *buf[2] = {reinterpret_cast<uint2 *>(ws + L.state_a), reinterpret_cast<uint2 *>(ws + L.state_b)};
    uint2 *inused = reinterpret_cast<uint2 *>(ws + L.inused);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(ws + L.cnt);
    int2 *carry = reinterpret_cast<int2 *>(ws + L.carry);
    int2 *dcagg = reinterpret_cast<int2 *>(ws + L.dcagg);
    const ScanHeader *dh = static_cast<const ScanHeader *>(d_header);
    if (hipMemsetAsync(status, 0, 16, st) != hipSuccess || hipMemsetAsync(ctrl, 0, CTRL_WORDS * 4, st) != hipSuccess ||
        hipMemsetAsync(coef, 0, (size_t)h->total_blocks * 128, st) != hipSuccess)
        return iamx::check_launch("iamx_jpeg_entropy_decode (memset)");
    const dim3 grid(L.n_wg), wg(LANES);
    for (int pass = 0; pass < h->max_passes; ++pass)
        hipLaunchKernelGGL(jpeg_sync_pass, grid, wg, 0, st, data, dh, pass, buf[(pass + 1) & 1], buf[pass & 1],
                           inused, cnt, ctrl);
    hipLaunchKernelGGL(jpeg_count_partial, grid, wg, 0, st, cnt, L.n, carry);
    ScanRanges rg = {};
    rg.n[0] = L.n_wg;
    hipLaunchKernelGGL(jpeg_top_scan, dim3(1), wg, 0, st, carry, rg, ctrl + CTRL_TOTAL);
    hipLaunchKernelGGL(jpeg_write_pass, grid, wg, 0, st, data, dh, buf[(h->max_passes - 1) & 1], cnt, carry, coef,
                       coef_blocks, ctrl);
    DcPlan plan;
    ScanRanges dr = {};
    int off = 0;
    for (int c = 0; c < 3; ++c) {
        plan.chunk_off[c] = off;
        dr.off[c] = off;
        dr.n[c] = L.dc_chunks[c];
        off += L.dc_chunks[c];
    }
    plan.chunk_off[3] = off;
    hipLaunchKernelGGL(jpeg_dc_scan<false>, dim3(L.dc_total), wg, 0, st, coef, coef_blocks, dh, plan, dcagg, ctrl);
    hipLaunchKernelGGL(jpeg_top_scan, dim3(h->ncomp), wg, 0, st, dcagg, dr, (uint32_t *)nullptr);
    hipLaunchKernelGGL(jpeg_dc_scan<true>, dim3(L.dc_total), wg, 0, st, coef, coef_blocks, dh, plan, dcagg, ctrl);
    hipLaunchKernelGGL(jpeg_finish, dim3(1), dim3(1), 0, st, dh, ctrl, status);
    return iamx::check_launch("iamx_jpeg_entropy_decode");
}
