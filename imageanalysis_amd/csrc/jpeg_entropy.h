// Entropy decoding of a baseline JPEG scan by self-synchronising sub-sequences: the ONE decode
// routine, compiled for the device (csrc/jpeg_entropy.hip: one lane per sub-sequence) and for the
// host (tools/jpeg_entropy_host.cpp: the same phases sub-sequence by sub-sequence, test
// infrastructure -- the python package never binds it).
//
// The scan is cut into sub-sequences of subseq_bytes bytes counted from its first byte (a power of
// two of at least two average MCUs, never below MIN_SUBSEQ_BYTES: the distance a cold decoder
// needs to fall into step is a number of MCUs, about forty at worst on the files studied, so the
// number of passes stays the same whatever the quality the file was written at).  A decoder
// state at a symbol boundary is (raw bit position, block index inside the MCU, zigzag index);
// lane i decodes the symbols that START inside sub-sequence i and hands the state behind them to
// lane i + 1.  Phases (every one a launch of its own, no waiting between workgroups):
//   sync   pass 0 starts every lane cold at its boundary; pass j >= 1 starts lane i from the end
//          state lane i - 1 stored in pass j - 1 (lane 0 from the true start of the scan).  A lane
//          whose input did not change keeps its output.  changed[j] counts the lanes whose output
//          differs from pass j - 1.  changed[last] == 0 means "end[i] == decode(end[i - 1]) for
//          every i", and since lane 0 starts true, induction makes every state true: the fixed
//          point is a proof.  Anything else is reported as NOT_SYNCED and nothing is written.
//   scan   exclusive prefix sum of the completed-block counts: the scan-order number of the
//          block each lane starts in.
//   write  every lane decodes once more from its true state and stores coefficients at their final
//          places, the DC value as the difference it decoded.
//   dc     segmented inclusive integer scan of the DC differences per component in scan order,
//          segments = restart intervals.
// Positions are RAW bit positions (stuffed FF 00 pairs included), so a sub-sequence boundary is a
// fixed byte of the file; the reader undoes the stuffing and keeps the raw position of the next
// unread bit exact (a mark on the last bit of every buffered FF data byte adds the 8 skipped bits).
// Markers: RSTn (files with a restart interval) is met by the symbol that runs into it; that symbol
// is void, and the state behind the marker is known: byte aligned, start of an MCU.  Any other
// marker, or the end of the data, is terminal: decoding ends there.  The header's scan_len ends at
// the first such marker (iamx_jpeg_entropy_prepare looks for it), so no lane starts behind it.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define IAMX_HD __host__ __device__ __forceinline__
#else
#define IAMX_HD inline
#endif

namespace iamx_jpeg {

constexpr int LOOK = 9;                   // bits of the first-level table (as the host half)
constexpr int MIN_SUBSEQ_BYTES = 128;     // one lane's share of the scan, at least
constexpr int MAX_SUBSEQ_BYTES = 4096;
constexpr int MAX_PASSES = 48;            // sync passes per call (pass 0 = cold); DESIGN.md section 4
constexpr int MAX_MCU_BLOCKS = 6;         // 4:2:0
constexpr uint32_t HEADER_MAGIC = 0x4a454e54u;
constexpr uint32_t MAX_SCAN_BYTES = 1u << 27;   // raw bit positions stay below 2^30

// status word of a decode
constexpr int32_t ST_PENDING = 0;         // the launches have not finished
constexpr int32_t ST_SYNCED = 1;          // fixed point reached, every block decoded from real bits
constexpr int32_t ST_NOT_SYNCED = 2;      // no fixed point inside the pass bound: nothing written
constexpr int32_t ST_DAMAGED = 3;         // fixed point reached, but the data ended early or a marker
                                          // stood out of place: coefficients as far as they go,
                                          // zeros behind them

struct Table {                            // one Huffman table in look-up form
    uint16_t fast[1 << LOOK];             // (length << 8) | symbol on LOOK bits, 0 = longer code
    int32_t maxcode[18];
    int32_t valoffset[18];
    uint8_t huffval[256];
};

struct alignas(16) ScanHeader {
    uint32_t magic;
    int32_t ncomp, restart, mcus_x, mcus_y, blocks_per_mcu;
    int32_t total_blocks, n_mcus;
    uint32_t file_len, scan_off, scan_len;
    int32_t n_subseq, max_passes, subseq_bytes;
    int32_t mcu_comp[8], mcu_bx[8], mcu_by[8];     // block b of an MCU: component, place inside it
    int32_t comp_h[4], comp_v[4], comp_bw[4], comp_base[4];
    uint8_t natural[64];                           // zigzag index -> natural (row major) index
    Table dc[3], ac[3];                            // per component
};

struct State {
    uint32_t pos;                          // raw bit position of the next unread bit
    uint32_t bk;                           // block in MCU | zigzag index << 3 | terminal << 9
};
constexpr uint32_t BK_TERMINAL = 1u << 9;
constexpr uint32_t COLD_INPUT = 0xffffffffu;       // "input" of a cold start (no real state has it)
constexpr uint32_t NO_END = 0xffffffffu;           // end position of the last lane

IAMX_HD bool same(State a, State b) { return a.pos == b.pos && a.bk == b.bk; }

// forward bit reader over the raw scan bytes, 16 bytes per load
struct Reader {
    const uint8_t *data;                   // the file (device: 16-byte aligned, padded to 16)
    uint32_t file_len, scan_off, scan_len;
    int restart;
    uint64_t acc, ffm;                     // bits, left aligned; marks on the last bit of FF data bytes
    int bits;
    uint32_t p;                            // next raw scan byte to load
    uint32_t pos;                          // raw bit position of the next unread bit
    int mk;                                // 0: data, 1: RSTn at byte mpos, 2: terminal at byte mpos
    uint32_t mpos;
    uint32_t c0, c1, c2, c3, cidx;         // the 16 bytes at file offset 16 * cidx

    IAMX_HD uint32_t byte_at(uint32_t q)   // q < scan_len
    {
        const uint32_t a = scan_off + q, ci = a >> 4;
        if (ci != cidx) {
            cidx = ci;
#if defined(__HIP_DEVICE_COMPILE__)
            const uint4 v = *reinterpret_cast<const uint4 *>(data + 16u * ci);
            c0 = v.x; c1 = v.y; c2 = v.z; c3 = v.w;
#else
            uint32_t w[4] = {0, 0, 0, 0};
            const uint32_t off = 16u * ci, n = file_len - off < 16u ? file_len - off : 16u;
            memcpy(w, data + off, n);
            c0 = w[0]; c1 = w[1]; c2 = w[2]; c3 = w[3];
#endif
        }
        const uint32_t wi = (a >> 2) & 3u;
        const uint32_t w = wi == 0 ? c0 : (wi == 1 ? c1 : (wi == 2 ? c2 : c3));
        return (w >> (8u * (a & 3u))) & 255u;
    }

    // afterwards more than 56 bits are buffered: a code (<= 16) and its magnitude bits (<= 15)
    IAMX_HD void fill()
    {
        while (bits <= 56) {
            uint32_t b = 0;
            if (mk == 0) {
                if (p >= scan_len) {
                    mk = 2;
                    mpos = scan_len;
                } else {
                    b = byte_at(p);
                    if (b == 0xFFu) {
                        const uint32_t nx = p + 1 < scan_len ? byte_at(p + 1) : 0x100u;
                        if (nx == 0) {
                            ffm |= 1ull << (56 - bits);
                            p += 2;
                        } else {
                            mk = (restart && nx >= 0xD0u && nx <= 0xD7u) ? 1 : 2;
                            mpos = p;
                            b = 0;
                        }
                    } else {
                        ++p;
                    }
                }
            }
            acc |= (uint64_t)b << (56 - bits);
            bits += 8;
        }
    }

    IAMX_HD void skip(int n)               // 0 <= n <= 31
    {
        if (n == 0) return;
        pos += (uint32_t)n + 8u * (uint32_t)__builtin_popcountll(ffm >> (64 - n));
        acc <<= n;
        ffm <<= n;
        bits -= n;
    }

    IAMX_HD void start(uint32_t at)        // raw bit position; at / 8 <= scan_len
    {
        acc = 0; ffm = 0; bits = 0; mk = 0; mpos = 0;
        p = at >> 3;
        pos = p * 8u;
        fill();
        skip((int)(at & 7u));
    }

    // true once the next unread bit lies behind the marker / the end of the data
    IAMX_HD bool past_marker() const { return mk != 0 && pos > 8u * mpos; }
};

IAMX_HD void reader_init(Reader &R, const ScanHeader *H, const uint8_t *data)
{
    R.data = data;
    R.file_len = H->file_len;
    R.scan_off = H->scan_off;
    R.scan_len = H->scan_len;
    R.restart = H->restart;
    R.cidx = 0xffffffffu;
    R.c0 = R.c1 = R.c2 = R.c3 = 0;
}

// the state a lane guesses at its boundary: first bit of the sub-sequence, start of an MCU.  A
// boundary between FF and its stuffed 00 (or the second byte of a marker) starts one byte later.
IAMX_HD State cold_state(Reader &R, uint32_t lane, uint32_t subseq_bytes)
{
    uint32_t B = lane * subseq_bytes;
    if (B > 0 && B < R.scan_len && R.byte_at(B - 1) == 0xFFu) {
        const uint32_t b = R.byte_at(B);
        if (b == 0 || (b >= 0xD0u && b <= 0xD7u)) ++B;
    }
    State s;
    s.pos = B * 8u;
    s.bk = 0;
    return s;
}

// code + magnitude bits of one symbol from the buffered bits (R.fill() done): the symbol, the
// extended value and the number of bits used
IAMX_HD int decode_code(const Reader &R, const Table *T, int &len)
{
    const int f = T->fast[(uint32_t)(R.acc >> (64 - LOOK))];
    if (f) {
        len = f >> 8;
        return f & 255;
    }
    int l = LOOK + 1;
    int code = (int)(R.acc >> (64 - l));
    while (l <= 16 && code > T->maxcode[l]) {
        ++l;
        code = (int)(R.acc >> (64 - l));
    }
    if (l > 16) {                          // corrupt: the host half uses 0 and drops 16 bits
        len = 16;
        return 0;
    }
    len = l;
    return T->huffval[(code + T->valoffset[l]) & 255];
}

IAMX_HD int magnitude(const Reader &R, int len, int sz)   // 1 <= sz <= 15
{
    const int v = (int)((R.acc << len) >> (64 - sz));
    return v < (1 << (sz - 1)) ? v - (1 << sz) + 1 : v;
}

// index (in blocks) of scan-order block `blk` whose place inside the MCU is b, or -1 outside
IAMX_HD int64_t block_index(const ScanHeader *H, uint32_t blk, int b, int64_t coef_blocks)
{
    const uint32_t m = blk / (uint32_t)H->blocks_per_mcu;
    if (m >= (uint32_t)H->n_mcus) return -1;
    const int c = H->mcu_comp[b];
    const int my = (int)(m / (uint32_t)H->mcus_x), mx = (int)(m - (uint32_t)my * (uint32_t)H->mcus_x);
    const int64_t i = (int64_t)H->comp_base[c] +
                      (int64_t)(my * H->comp_v[c] + H->mcu_by[b]) * H->comp_bw[c] + mx * H->comp_h[c] +
                      H->mcu_bx[b];
    return (i >= 0 && i < coef_blocks && i < (int64_t)H->total_blocks) ? i : -1;
}

// One lane: decode from `in` the symbols that start before raw bit `endpos`.
//   WRITE = false (sync): nothing is stored.
//   WRITE = true: coefficients go to coef (every store checked against coef_blocks), `blk` is the
//     scan-order number of the block the lane starts in.
// Both stop at the end of the scan (the terminal marker): the symbol that runs into it is void.
// A frame whose blocks are not all decoded by then is DAMAGED and keeps the cleared zeros behind
// the last decoded block -- the host half goes on with zero bits there, block after block, which
// is work set by the frame size the file claims and not by the bytes it holds; no lane does that.
// out = state behind the last symbol, nblocks = blocks completed, damaged = data ended early or
// a marker stood inside an MCU.  Every loop iteration consumes at least one bit or jumps behind a
// restart marker, and a lane starts at or behind its own first bit: at most 8 * subseq_bytes + 64
// iterations per lane, whatever the frame size.
template <bool WRITE>
IAMX_HD void decode_lane(const ScanHeader *H, const uint8_t *data, State in, uint32_t endpos,
                         uint32_t blk, int16_t *coef, int64_t coef_blocks, State &out,
                         uint32_t &nblocks, bool &damaged)
{
    out = in;
    nblocks = 0;
    damaged = false;
    if (in.bk & BK_TERMINAL) return;
    const uint32_t total = (uint32_t)H->total_blocks, bpm = (uint32_t)H->blocks_per_mcu;
    Reader R;
    reader_init(R, H, data);
    if ((in.pos >> 3) > R.scan_len) in.pos = R.scan_len * 8u;
    R.start(in.pos);
    int b = (int)(in.bk & 7u), k = (int)((in.bk >> 3) & 63u);
    if (b >= (int)bpm) b = 0;
    int64_t at = WRITE ? block_index(H, blk, b, coef_blocks) : -1;
    uint32_t budget = 8u * (uint32_t)H->subseq_bytes + 64u;
    while (budget-- > 0) {
        if (R.pos >= endpos) break;
        if (WRITE && blk >= total) break;
        R.fill();
        const int c = H->mcu_comp[b];
        int len, sz, run = 0, val = 0;
        bool eob = false;
        if (k == 0) {
            sz = decode_code(R, &H->dc[c], len);
            if (sz > 15) sz = 0;           // corrupt table entry (as the host half)
        } else {
            const int rs = decode_code(R, &H->ac[c], len);
            run = rs >> 4;
            sz = rs & 15;
            if (sz == 0) {
                eob = run != 15;
                run = 15;                  // ZRL: sixteen zeros (k += run + 1)
            }
        }
        if (sz) val = magnitude(R, len, sz);
        R.skip(len + sz);
        if (R.past_marker()) {
            if (R.mk == 1) {
                // ran into RSTn: the symbol is void; behind the marker an MCU starts
                if (b != 0 || k != 0) damaged = true;
                const uint32_t q = R.mpos + 2u;
                b = 0;
                k = 0;
                R.start((q > R.scan_len ? R.scan_len : q) * 8u);
                if (WRITE) at = block_index(H, blk, b, coef_blocks);
                continue;
            }
            // terminal: the symbol is void, nothing behind it is decoded
            if (WRITE) damaged = true;     // (blk < total: blocks are missing)
            out.pos = R.mpos * 8u;
            out.bk = BK_TERMINAL;
            return;
        }
        if (k == 0) {
            if (WRITE && at >= 0) coef[at * 64] = (int16_t)val;
            k = 1;
        } else if (eob) {
            k = 64;
        } else {
            k += run;
            if (sz) {
                if (WRITE && at >= 0 && k < 64) coef[at * 64 + H->natural[k]] = (int16_t)val;
            }
            ++k;
        }
        if (k >= 64) {
            k = 0;
            b = b + 1 == (int)bpm ? 0 : b + 1;
            ++nblocks;
            ++blk;
            if (WRITE) at = block_index(H, blk, b, coef_blocks);
        }
    }
    out.pos = R.pos;
    out.bk = (uint32_t)b | ((uint32_t)k << 3);
}

}  // namespace iamx_jpeg
