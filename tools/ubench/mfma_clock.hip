// micro-benchmark: sustained v_mfma_i32_32x32x32_i8 rate and shader clock on gfx950 for
//   (a) independent accumulators vs dependent chains of 4, (b) zero vs random operand data,
//   (c) 2 vs 4 waves per SIMD.  clock = s_memtime ticks / s_memrealtime (100 MHz) ticks.
//   (d) round 16: v_mfma_i32_16x16x64_i8 on the same output tile per wave (two 32 x 32 tiles as 2 x 4
//       accumulators of 16 x 16, K = 128 a round: 16 MFMAs of half the work each), random data, ONE
//       wave per SIMD -- beside 32x32x32 at one wave per SIMD.  Rates are per 32x32x32 of work.
//   (e) round 17, the gate of a 16x16x64 sweep form: the two shapes alternating in one process, three
//       repeats each, on operands with the bit patterns of the sorted store (descriptor rows made the way
//       tests/test_sweep_raw_gpu.py::_rows makes them; value - 128 is the A operand, its complement the B
//       operand) and on random data; then the same pair of loops carrying the sweep's vector load per
//       unit of work: 5 independent v_min3_i32 after every 32x32x32, 2 and 3 alternating after every
//       16x16x64 (40 per 8 x 32x32x32 of work either way).  The minima read registers no MFMA writes:
//       they price the vector port, not a dependency.  Every measurement is the third of three
//       back-to-back launches; the clock is the median over workgroups.
//   Build: hipcc --offload-arch=gfx950 -O3 -mllvm -amdgpu-mfma-vgpr-form -o mfma_clock mfma_clock.hip
//   (the library's flag for the sweep).  Without it the compiler keeps the v4i accumulators of (d) in AGPRs
//   and shifts the result tuples: 56 v_accvgpr copies an iteration beside the 16 MFMAs, and the figure is
//   theirs.  With it the loops are bare: 8 MFMAs (32x32x32), 16 MFMAs (16x16x64) and the loop counter;
//   the loaded loops of (e) hold those, 40 v_min3_i32 and the loop counter.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <random>
#include <vector>
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// one of five independent running minima; a sched_barrier after each gap's minima keeps them in that gap
#define MIN3(c) asm volatile("v_min3_i32 %0, %0, %1, %2" : "+v"(m[c]) : "v"(a[1][c & 3]), "v"(b[2][(c + 1) & 3]))

// MODE 0: 2 independent accumulators  1: dependent chain of 4 then new C  2: 16x16x64, 8 accumulators
// VALU: the sweep's minima beside the MFMAs (modes 0 and 2)
template <int MODE, bool VALU>
__global__ __launch_bounds__(256) void k(const v4i *data, int iters, long long *clk, int *sink)
{
    v4i a[4], b[4];
    for (int s = 0; s < 4; ++s) {
        a[s] = data[(blockIdx.x * 256 + threadIdx.x) * 8 + s];
        b[s] = data[(blockIdx.x * 256 + threadIdx.x) * 8 + 4 + s];
    }
    v16i acc0 = {0}, acc1 = {0};
    v16i c0 = {0};
    int m[5] = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
    long long t0 = clock64(), w0 = wall_clock64();
    int keep = 0;
    v4i q[8] = {{0}, {0}, {0}, {0}, {0}, {0}, {0}, {0}};
    for (int i = 0; i < iters; ++i) {
        if (MODE == 2) {
            // tile j of the two 32 x 32 outputs: operand halves differ per 16 x 16 sub-tile in a real kernel;
            // here every sub-tile takes its own pair of registers so that no two MFMAs are identical
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    q[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[(j + 2 * s) & 3], b[(j >> 1) & 3], q[j], 0, 0, 0);
                    if (VALU) {
                        const int c = 2 * (j & 1);             // 2, 3, 2, 3, ...: chains 0 1 | 2 3 4
                        MIN3(c); MIN3(c + 1);
                        if (j & 1) MIN3(c + 2);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
        } else if (MODE == 0) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], b[s], acc0, 0, 0, 0);
                if (VALU) { MIN3(0); MIN3(1); MIN3(2); MIN3(3); MIN3(4); __builtin_amdgcn_sched_barrier(0); }
                acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(b[s], a[s], acc1, 0, 0, 0);
                if (VALU) { MIN3(0); MIN3(1); MIN3(2); MIN3(3); MIN3(4); __builtin_amdgcn_sched_barrier(0); }
            }
        } else {
            v16i x = c0, y = c0;
#pragma unroll
            for (int s = 0; s < 4; ++s) x = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], b[s], x, 0, 0, 0);
#pragma unroll
            for (int s = 0; s < 4; ++s) y = __builtin_amdgcn_mfma_i32_32x32x32_i8(b[s], a[s], y, 0, 0, 0);
            keep ^= x[0] ^ y[5];
            a[0][0] += 1;          // new operands every round (no CSE)
        }
    }
    long long t1 = clock64(), w1 = wall_clock64();
    if (threadIdx.x == 0) { clk[2 * blockIdx.x] = t1 - t0; clk[2 * blockIdx.x + 1] = w1 - w0; }
    int s = keep;
    for (int e = 0; e < 16; ++e) s += acc0[e] + acc1[e];
    for (int j = 0; j < 8; ++j) s += q[j][0] + q[j][1] + q[j][2] + q[j][3];
    for (int c = 0; c < 5; ++c) s += m[c];
    if (s == 0x12345678) sink[0] = s;
}

struct Result { double ms, ns, ghz; };

template <int MODE, bool VALU>
Result run(const char *name, const v4i *d, int blocks_per_cu, int iters = 200000, int launches = 1)
{
    long long *clk; int *sink;
    const int nb = 256 * blocks_per_cu;
    (void)hipMalloc(&clk, nb * 16); (void)hipMalloc(&sink, 4);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    // 200000 iterations: 1.6 M MFMAs per wave, ~30-50 ms
    hipLaunchKernelGGL((k<MODE, VALU>), dim3(nb), dim3(256), 0, 0, d, 1000, clk, sink);
    (void)hipDeviceSynchronize();
    for (int l = 1; l < launches; ++l) hipLaunchKernelGGL((k<MODE, VALU>), dim3(nb), dim3(256), 0, 0, d, iters, clk, sink);
    hipEventRecord(e0);
    hipLaunchKernelGGL((k<MODE, VALU>), dim3(nb), dim3(256), 0, 0, d, iters, clk, sink);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    std::vector<long long> h(2 * nb); (void)hipMemcpy(h.data(), clk, nb * 16, hipMemcpyDeviceToHost);
    std::vector<double> g(nb);
    for (int w = 0; w < nb; ++w) g[w] = (double)h[2 * w] / ((double)h[2 * w + 1] / 100e6) / 1e9;
    std::sort(g.begin(), g.end());
    const double mfma_per_simd = (double)iters * 8 * blocks_per_cu;      // (in 32x32x32 of work: 16 of 16x16x64 = 8)
    const double ghz = g[nb / 2];
    printf("%-44s %d waves/SIMD: %7.2f ms  %.2f ns/MFMA/SIMD  shader clock %.3f GHz  => %.1f cycles/MFMA\n",
           name, blocks_per_cu, ms, ms * 1e6 / mfma_per_simd, ghz, ms * 1e6 / mfma_per_simd * ghz);
    fflush(stdout);
    (void)hipFree(clk); (void)hipFree(sink);
    hipEventDestroy(e0); hipEventDestroy(e1);
    return {ms, ms * 1e6 / mfma_per_simd, ghz};
}

// one pair of loops, the two shapes alternating, REPS repeats each; prints the decision rule's figures
template <bool VALU>
void gate_pair(const char *what, const char *dname, const v4i *d)
{
    const int REPS = 3, iters = 600000;
    char n32[96], n16[96];
    snprintf(n32, sizeof n32, "32x32x32%s, %s", VALU ? " + 5 v_min3" : "", dname);
    snprintf(n16, sizeof n16, "16x16x64%s, %s", VALU ? " + 2/3 v_min3" : "", dname);
    double lo32 = 1e30, hi32 = 0, lo16 = 1e30, hi16 = 0;
    for (int r = 0; r < REPS; ++r) {
        const Result p = run<0, VALU>(n32, d, 1, iters, 3);
        const Result s = run<2, VALU>(n16, d, 1, iters, 3);
        lo32 = std::min(lo32, p.ms); hi32 = std::max(hi32, p.ms);
        lo16 = std::min(lo16, s.ms); hi16 = std::max(hi16, s.ms);
    }
    const double spread = std::max(hi32 - lo32, hi16 - lo16);
    printf("# %s, %s: 32x32x32 %.2f .. %.2f ms, 16x16x64 %.2f .. %.2f ms, larger within-shape spread %.2f ms;\n"
           "#   slowest 16x16x64 ahead of fastest 32x32x32 by %+.2f ms (%+.1f %%), 3 x spread = %.2f ms\n",
           what, dname, lo32, hi32, lo16, hi16, spread, lo32 - hi16, 100.0 * (lo32 - hi16) / lo32, 3 * spread);
    fflush(stdout);
}

// descriptor rows as tests/test_sweep_raw_gpu.py::_rows makes them: gamma(0.6) magnitudes, unit norm, clipped at
// 0.2, times 640, as bytes.  A thread's first 64 bytes are value - 128 (the A operand of the sweep), its last 64
// the complement of value - 128 (the B operand).
static void descriptor_operands(unsigned char *p, size_t threads)
{
    std::mt19937 rng(1);
    std::gamma_distribution<double> gamma(0.6, 1.0);
    for (size_t t = 0; t < threads; ++t) {
        double g[128], n2 = 0;
        for (int e = 0; e < 128; ++e) { g[e] = gamma(rng); n2 += g[e] * g[e]; }
        const double inv = 1.0 / sqrt(n2);
        for (int e = 0; e < 128; ++e) {
            const int v = std::min(255, std::max(0, (int)nearbyint(std::min(g[e] * inv, 0.2) * 640.0)));
            const int s = v - 128;
            p[t * 128 + e] = (unsigned char)(e < 64 ? s : ~s);
        }
    }
}

int main()
{
    const size_t n = 256 * 4 * 256 * 8;
    v4i *h = (v4i *)malloc(n * sizeof(v4i)), *dz, *dr, *dd;
    (void)hipMalloc(&dz, n * sizeof(v4i)); (void)hipMalloc(&dr, n * sizeof(v4i)); (void)hipMalloc(&dd, n * sizeof(v4i));
    (void)hipMemset(dz, 0, n * sizeof(v4i));
    descriptor_operands((unsigned char *)h, n / 8);
    (void)hipMemcpy(dd, h, n * sizeof(v4i), hipMemcpyHostToDevice);
    srand(1);
    for (size_t i = 0; i < n * 4; ++i) ((int *)h)[i] = (rand() << 16) ^ rand();
    (void)hipMemcpy(dr, h, n * sizeof(v4i), hipMemcpyHostToDevice);
    // (e) the gate: bare pair, then the pair that carries the sweep's minima; descriptor bits, then random
    gate_pair<false>("bare", "descriptor bits", dd);
    gate_pair<false>("bare", "random data", dr);
    gate_pair<true>("with minima", "descriptor bits", dd);
    gate_pair<true>("with minima", "random data", dr);
    run<0, false>("32x32x32, independent accumulators, random data", dr, 1);
    run<2, false>("16x16x64, 8 accumulators, random data", dr, 1);
    run<0, false>("32x32x32, independent accumulators, random data", dr, 1);
    run<2, false>("16x16x64, 8 accumulators, random data", dr, 1);
    for (int w : {2, 4}) {
        run<0, false>("independent accumulators, zero data", dz, w);
        run<0, false>("independent accumulators, random data", dr, w);
        run<1, false>("chains of 4 (fresh C), zero data", dz, w);
        run<1, false>("chains of 4 (fresh C), random data", dr, w);
    }
    return 0;
}
