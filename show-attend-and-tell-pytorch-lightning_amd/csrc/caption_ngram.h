// Device helpers shared by caption_consensus.hip and caption_mbr.hip: the n-gram key of the document-frequency table (layout and
// hash: include/sat_hip.h, sat_ngram_table_add), its probe with plain loads, the CIDEr-D weight of one n-gram position and the wave
// forms both kernels reduce with.  One definition: both files see the same keys, the same probe order and the same fp64 roundings
// (each is built without FMA contraction).
#pragma once
#include "caption_score.h"

#include <math.h>

namespace sat {

typedef unsigned long long u64;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// tokens as the keys see them: 1..65535 (0 is "no token")
__device__ __forceinline__ int key_token(int tok) { return clampi(tok, 0, 65534) + 1; }

__device__ __forceinline__ u64 pack_ngram(const int* g, int n) {
    u64 k = 0;
    for (int q = 0; q < n; ++q) k |= (u64)(unsigned)g[q] << (16 * q);
    return k;
}

__device__ __forceinline__ bool same_ngram(const int* a, const int* b, int n) {
    bool eq = true;
    for (int q = 0; q < n; ++q) eq = eq && (a[q] == b[q]);
    return eq;
}

// murmur3's 64-bit finaliser
__device__ __forceinline__ u64 hash_key(u64 k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// document frequency of `key`: plain loads, the table is complete
__device__ __forceinline__ unsigned table_lookup(const u64* __restrict__ keys, const unsigned* __restrict__ counts, long capacity, u64 key) {
    const u64 mask = (u64)capacity - 1;
    u64 slot = hash_key(key) & mask;
    for (long probe = 0; probe < capacity; ++probe) {
        const u64 k = keys[slot];
        if (k == key) return counts[slot];
        if (k == 0ULL) return 0u;
        slot = (slot + 1) & mask;
    }
    return 0u;
}

// weight of the n-gram at position i of seq[0..len): tf * (log N - log max(1, df)) at its first occurrence (`first`), else 0
__device__ __forceinline__ double ngram_weight(const int* seq, int len, int i, int n, const u64* __restrict__ keys,
                                               const unsigned* __restrict__ counts, long capacity, double log_n, bool& first) {
    first = false;
    if (i + n > len) return 0.0;
    const int* g = seq + i;
    for (int j = 0; j < i; ++j)
        if (same_ngram(seq + j, g, n)) return 0.0;
    first = true;
    int tf = 1;
    for (int j = i + 1; j + n <= len; ++j) tf += same_ngram(seq + j, g, n) ? 1 : 0;
    const unsigned df = table_lookup(keys, counts, capacity, pack_ngram(g, n));
    return (double)tf * (log_n - log(df > 1u ? (double)df : 1.0));
}

__device__ __forceinline__ int wave_prefix_max(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v = t > v ? t : v;
    }
    return v;
}

// LCS length of a[0..la) and b[0..lb), lb <= 128, by one wave (every lane gets it): lane l holds the cells j = l and j = 64 + l of
// the LCS row over b, one token of a per step: new[j] = max over k <= j of (match ? old[k-1] + 1 : old[k]), a wave prefix maximum
__device__ __forceinline__ int wave_lcs(const int* a, int la, const int* b, int lb, int lane) {
    const int t0 = lane < lb ? b[lane] : -1, t1 = 64 + lane < lb ? b[64 + lane] : -1;      // -1 matches nothing
    int c0 = 0, c1 = 0;
    for (int i = 0; i < la; ++i) {
        const int h = a[i];
        const int u0 = __shfl_up(c0, 1, 64), u1 = __shfl_up(c1, 1, 64), e0 = __shfl(c0, 63, 64);
        const int d0 = lane ? u0 : 0, d1 = lane ? u1 : e0;                 // the old row one cell to the left
        const int p0 = wave_prefix_max(h == t0 ? d0 + 1 : c0, lane);
        const int p1 = wave_prefix_max(h == t1 ? d1 + 1 : c1, lane);
        const int top = __shfl(p0, 63, 64);
        c0 = p0; c1 = p1 > top ? p1 : top;
    }
    return __shfl(c1, 63, 64);                         // cells beyond b's end never match: the last cell holds the result
}

}  // namespace sat
