// First-come-wins de-duplication of a match list on the "%.2f-%.2f" keys of either end point
// (scripts/lib/matcher.py:157-182 filter_duplicates), with the order-preserving compaction and the
// workgroup sum it is built from: what the select stages of the 'bestratio', 'smart' and 'bruteforce'
// strategies take a list with (bin_select.h).  A workgroup of NT threads calls these, all threads together.
#pragma once
#include "iamx_common.h"

namespace iamx_kd {

constexpr int NT = 256;                    // threads of the calling workgroup
constexpr int ID_MASK = (1 << 25) - 1;     // list position + 1 (a list has at most 2^24 entries)
constexpr int MULTI = 1 << 29;             // the slot's key is carried by more than one entry
constexpr int USED = 1 << 30;              // the replay has reserved the slot's key

__device__ __forceinline__ unsigned hash32(unsigned k)
{
    k ^= k >> 16; k *= 0x7feb352du; k ^= k >> 15; k *= 0x846ca68bu; k ^= k >> 16;
    return k;
}

// a key-table slot as the atomics of the workgroup's other waves left it (those are performed in L2:
// the load must not be served from a line the CU's vector cache read before them)
__device__ __forceinline__ int slot_now(const int32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int block_sum(int v, int *red)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// order-preserving compaction: write(new position, i) for every i < m with keep(i); returns the
// new length (the same value in every thread), writes visible to the workgroup
template <typename K, typename W>
__device__ int compact(int *red, int m, K keep, W write)
{
    int base = 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int s = 0; s < m; s += NT) {
        const int i = s + threadIdx.x;
        const bool k = i < m && keep(i);
        const unsigned long long bal = __ballot(k);
        __syncthreads();
        if (lane == 0) red[wave] = __popcll(bal);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += red[w];
        if (k) write(off + __popcll(bal & ((1ull << lane) - 1)), i);
        base += red[0] + red[1] + red[2] + red[3];
    }
    __syncthreads();
    return base;
}

// filter_duplicates (matcher.py:157-182) over list[0..m): keep[i] = 1 where the sequential
// first-come-wins loop on the "%.2f-%.2f" keys of either end keeps entry i (a dropped entry
// reserves no key); returns the number kept.  A parallel pass gives every entry the table slot of
// its query key and of its train key (equal keys <=> equal slots) and marks the slots more than one
// entry carries; an entry with no such slot is kept whatever the others do, and only the rest --
// in list order -- is replayed by one thread.
__device__ int dedupe(int *red, const int32_t *kq, const int32_t *kt, const int32_t *list, int m,
                      int32_t *tabq, int32_t *tabt, int32_t *slotq, int32_t *slott, int32_t *cont,
                      int32_t *keep, int tab_size)
{
    if (m == 0) return 0;
    int T = 64;
    while (T < 2 * m && T < tab_size) T <<= 1;
    for (int i = threadIdx.x; i < T; i += NT) { tabq[i] = 0; tabt[i] = 0; }
    __syncthreads();
    auto same = [](const int32_t *k, int a, int b) { return k[2 * a] == k[2 * b] && k[2 * a + 1] == k[2 * b + 1]; };
    for (int i = threadIdx.x; i < m; i += NT) {
        for (int side = 0; side < 2; ++side) {
            const int32_t *k = side ? kt : kq;
            int32_t *tab = side ? tabt : tabq;
            const int row = list[2 * i + side];
            unsigned h = hash32((unsigned)k[2 * row] * 0x9E3779B1u ^ (unsigned)k[2 * row + 1]) & (T - 1);
            while (true) {
                const int prev = atomicCAS(&tab[h], 0, i + 1);
                if (prev == 0) break;
                if (same(k, list[2 * ((prev & ID_MASK) - 1) + side], row)) { atomicOr(&tab[h], MULTI); break; }
                h = (h + 1) & (T - 1);
            }
            (side ? slott : slotq)[i] = (int)h;
        }
    }
    __syncthreads();
    const int nc = compact(red, m,
                           [&](int i) {
                               const bool c = ((slot_now(tabq + slotq[i]) | slot_now(tabt + slott[i])) & MULTI) != 0;
                               keep[i] = c ? 0 : 1;
                               return c;
                           },
                           [&](int pos, int i) { cont[pos] = i; });
    if (nc == 0) return m;
    if (threadIdx.x == 0) {
        for (int j = 0; j < nc; ++j) {
            const int i = cont[j], hq = slotq[i], ht = slott[i];
            if (!((slot_now(tabq + hq) | slot_now(tabt + ht)) & USED)) {
                atomicOr(&tabq[hq], USED);
                atomicOr(&tabt[ht], USED);
                keep[i] = 1;
            }
        }
    }
    __syncthreads();
    int c = 0;
    for (int i = threadIdx.x; i < m; i += NT) c += keep[i];
    return block_sum(c, red);
}

}  // namespace iamx_kd
