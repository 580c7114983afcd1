// The sampling rule of the RANSAC match verification (match_verify.hip, verify_pairs_kernel), in one
// place for the kernel and for the host function that tests walk (iamx_verify_sample,
// tests/verify_reference.py restates it in Python integers).
//
// Hypothesis `hyp` of a pair with n matches draws k distinct match indices.  There is no state: the
// draw is a counter-based hash of (seed, n, hyp, draw number), 64-bit unsigned arithmetic that wraps,
// nothing else.
//
//     mix(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;
//              z ^= z >> 31                                          (the splitmix64 finaliser)
//     key   =  mix(mix(mix(seed + G) ^ n) + hyp * G),                 G = 0x9E3779B97F4A7C15
//     r_d   =  mix(key + (d + 1) * 0xD1B54A32D192ED03)                d = 0 .. k-1
//     j_d   =  ((r_d >> 32) * (n - d)) >> 32                          in [0, n - d),  n < 2^31
//
// Fisher-Yates without the array: j_d counts among the n - d indices not taken by draws 0 .. d-1, in
// ascending order.  With the taken indices sorted ascending, each one that is <= the running index
// moves it up by one.  out[d] is the index draw d took; out is in draw order, not sorted.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VERIFY_RULE_FN __host__ __device__ inline
#else
#define VERIFY_RULE_FN inline
#endif

#define VERIFY_MAX_SAMPLE 8

VERIFY_RULE_FN uint64_t verify_mix(uint64_t z)
{
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

VERIFY_RULE_FN uint64_t verify_key(uint64_t seed, uint64_t n, uint64_t hyp)
{
    const uint64_t G = 0x9E3779B97F4A7C15ull;
    return verify_mix(verify_mix(verify_mix(seed + G) ^ n) + hyp * G);
}

// k <= VERIFY_MAX_SAMPLE, k <= n < 2^31.  Every loop has constant bounds and every array index is a
// constant after unrolling, so on the device `out` and the sorted list stay in registers.
VERIFY_RULE_FN void verify_sample(int64_t n, int k, int64_t hyp, uint64_t seed,
                                  int32_t (&out)[VERIFY_MAX_SAMPLE])
{
    const uint64_t key = verify_key(seed, (uint64_t)n, (uint64_t)hyp);
    int32_t s[VERIFY_MAX_SAMPLE];
#pragma unroll
    for (int d = 0; d < VERIFY_MAX_SAMPLE; ++d) {
        out[d] = -1;
        s[d] = 0x7fffffff;
    }
#pragma unroll
    for (int d = 0; d < VERIFY_MAX_SAMPLE; ++d) {
        if (d < k) {
            const uint64_t r = verify_mix(key + (uint64_t)(d + 1) * 0xD1B54A32D192ED03ull);
            int32_t j = (int32_t)(((r >> 32) * (uint64_t)(n - d)) >> 32);
#pragma unroll
            for (int i = 0; i < d; ++i)
                if (j >= s[i]) ++j;
            out[d] = j;
            // insert j into the sorted list s[0 .. d]
            int32_t v = j;
#pragma unroll
            for (int i = 0; i <= d; ++i) {
                const int32_t lo = s[i] < v ? s[i] : v, hi = s[i] < v ? v : s[i];
                s[i] = lo;
                v = hi;
            }
        }
    }
}
