// Host driver of the device JPEG entropy decoder's shared decode routine
// (imageanalysis_amd/csrc/jpeg_entropy.h): the same phases -- synchronise, scan, write, DC
// prediction -- run sub-sequence by sub-sequence on the CPU.  Test infrastructure: this is how the
// algorithm is debugged without a GPU and fuzzed under the host AddressSanitizer / UBSan
// (tests/test_jpeg_entropy.py builds it); the python package never binds it.
//
//   jpeg_entropy_host HEADER FILE OUT [MAX_PASSES]
// HEADER: the flat header iamx_jpeg_entropy_prepare wrote, FILE: the JPEG, MAX_PASSES: pass bound
// (default: the header's; the tests set it to the number of sub-sequences for files that never
// synchronise).  OUT: int32 status (IAMX_JPEG_*), int32 passes, int32 blocks, int32 sub-sequences,
// then int16 [blocks + 1][64]: the coefficients and a guard row of 12345 behind them.
// The file buffer is exactly as long as the file and the coefficient buffer ends behind the guard
// row, so a wild index is the sanitizer's to find.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../imageanalysis_amd/csrc/jpeg_entropy.h"

using namespace iamx_jpeg;

static std::vector<uint8_t> slurp(const char *path)
{
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: %s HEADER FILE OUT [MAX_PASSES]\n", argv[0]); return 2; }
    const std::vector<uint8_t> hb = slurp(argv[1]);
    const std::vector<uint8_t> file = slurp(argv[2]);
    if (hb.size() < sizeof(ScanHeader)) { fprintf(stderr, "short header\n"); return 2; }
    ScanHeader *H = new ScanHeader;
    memcpy(H, hb.data(), sizeof(ScanHeader));
    if (H->magic != HEADER_MAGIC || H->file_len != file.size() ||
        (uint64_t)H->scan_off + H->scan_len > file.size() || H->blocks_per_mcu < 1 ||
        H->blocks_per_mcu > MAX_MCU_BLOCKS || H->total_blocks < 1 || H->n_subseq < 1 || H->subseq_bytes < MIN_SUBSEQ_BYTES ||
        (uint64_t)H->n_subseq * (uint32_t)H->subseq_bytes < H->scan_len) {
        fprintf(stderr, "header does not belong to this file\n");
        return 2;
    }
    if (argc > 4) H->max_passes = atoi(argv[4]);
    if (H->max_passes < 2) H->max_passes = 2;
    // (pass 0 is the cold pass and the last pass only confirms that nothing changed: a scan of n
    // sub-sequences that never synchronises needs n + 1 passes to be verified)
    const int n = H->n_subseq, P = H->max_passes;
    const int64_t blocks = H->total_blocks;
    const uint8_t *data = file.data();
    std::vector<int16_t> coef((size_t)(blocks + 1) * 64, 0);
    for (int i = 0; i < 64; ++i) coef[(size_t)blocks * 64 + i] = 12345;

    auto endpos = [&](int i) { return i + 1 == n ? NO_END : (uint32_t)(i + 1) * (8u * (uint32_t)H->subseq_bytes); };
    const State cold_in = {COLD_INPUT, COLD_INPUT};
    std::vector<State> buf[2] = {std::vector<State>(n), std::vector<State>(n)}, inused(n);
    std::vector<uint32_t> cnt(n, 0);
    // ---- synchronise
    uint32_t changed = 1;
    int passes = P;
    for (int pass = 0; pass < P; ++pass) {
        if (pass >= 2 && changed == 0) { passes = pass - 1; break; }
        std::vector<State> &prev = buf[(pass + 1) & 1], &cur = buf[pass & 1];
        changed = 0;
        for (int i = 0; i < n; ++i) {
            State in, out, before = cold_in;
            if (pass == 0) {
                Reader R;
                reader_init(R, H, data);
                in = cold_state(R, (uint32_t)i, (uint32_t)H->subseq_bytes);
            } else {
                in.pos = in.bk = 0;
                if (i > 0) in = prev[i - 1];
                before = prev[i];
            }
            if (pass >= 2 && same(in, inused[i])) {
                out = before;
            } else {
                uint32_t nb;
                bool damaged;
                decode_lane<false>(H, data, in, endpos(i), 0u, nullptr, 0, out, nb, damaged);
                cnt[i] = nb;
                inused[i] = pass == 0 ? cold_in : in;
            }
            cur[i] = out;
            if (pass > 0 && !same(out, before)) ++changed;
        }
    }
    if (changed == 0 && passes == P) passes = P - 1;
    int32_t status;
    if (changed != 0) {
        status = ST_NOT_SYNCED;            // nothing is written from an unverified state
    } else {
        // (a converged run left both buffers equal)
        const std::vector<State> &fin = buf[(P - 1) & 1];
        // ---- scan
        std::vector<uint32_t> first(n);
        uint32_t total = 0;
        for (int i = 0; i < n; ++i) { first[i] = total; total += cnt[i]; }
        // ---- write
        bool any_damaged = false;
        for (int i = 0; i < n; ++i) {
            State in = {0, 0}, out;
            if (i > 0) in = fin[i - 1];
            uint32_t nb;
            bool damaged;
            decode_lane<true>(H, data, in, endpos(i), first[i], coef.data(), blocks, out, nb, damaged);
            any_damaged |= damaged;
        }
        // ---- DC prediction: segmented inclusive sum per component in scan order
        for (int c = 0; c < H->ncomp; ++c) {
            const int h = H->comp_h[c], v = H->comp_v[c];
            uint32_t pred = 0;
            for (int m = 0; m < H->n_mcus; ++m) {
                if (H->restart > 0 && m % H->restart == 0) pred = 0;
                const int my = m / H->mcus_x, mx = m % H->mcus_x;
                for (int by = 0; by < v; ++by)
                    for (int bx = 0; bx < h; ++bx) {
                        const int64_t at = (int64_t)H->comp_base[c] + (int64_t)(my * v + by) * H->comp_bw[c] + mx * h + bx;
                        if (at < 0 || at >= blocks) continue;
                        pred += (uint32_t)(int32_t)coef[(size_t)at * 64];
                        coef[(size_t)at * 64] = (int16_t)(int32_t)pred;
                    }
            }
        }
        status = (any_damaged || total != (uint32_t)blocks) ? ST_DAMAGED : ST_SYNCED;
    }
    FILE *f = fopen(argv[3], "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    const int32_t head[4] = {status, passes, (int32_t)blocks, n};
    fwrite(head, sizeof head, 1, f);
    fwrite(coef.data(), 2, coef.size(), f);
    fclose(f);
    delete H;
    return 0;
}
