// CIDEr-D and ROUGE-L of decoded captions on the device, next to caption_score.hip's BLEU / GLEU statistics (metrics.py is the
// specification: document_frequency, cider_d, rouge_l).
//
//   The document-frequency table: open addressing, linear probing, a power-of-two capacity; keys[capacity] (64 bit) followed by
//   counts[capacity] (32 bit) in one allocation.  A key packs an n-gram exactly: (token + 1) in 16 bits per position, first token
//   lowest, unused positions 0 -- the order n is implicit, two different n-grams never share a key and 0 means "empty slot".
//
//   ngram_table_add_kernel   one workgroup per image: the references (c[1:l], tokens clamped into [0, 65534]) staged in LDS; one
//                            thread per (reference, position) walks every earlier position of the image (all references) once and
//                            learns for the four orders together whether its n-gram occurred before; a first occurrence is inserted:
//                            64-bit atomicCAS on the key slot (empty -> claimed, equal -> found, else the next slot), then
//                            atomicAdd(count, 1).  Every look at a slot during the build is the value the CAS returned, never a plain
//                            load: the chip's eight L2s are not coherent within a launch, device-scope atomics are.  The probe loop is
//                            bounded by the capacity; a full table raises the error flag and drops the n-gram.  Counts are integers:
//                            the key -> count mapping does not depend on arrival order (the slot positions may).
//   caption_consensus_kernel one workgroup per image, all CIDEr arithmetic in fp64 (this file is built without FMA contraction).
//                            Thread t owns position t & 127 of the orders (t >> 7) + 1 and (t >> 7) + 3, so a wave holds one order
//                            at a time and every sum below is two wave sums added in a fixed order: the same table content gives the
//                            same bits.  Hypothesis weights tf * (log N - log max(1, df)) once (tf by brute-force compares, df by a
//                            probe with plain loads: the table was built by earlier launches), zero off the first occurrence; then
//                            reference by reference its weights into LDS, its norms, and for every hypothesis first occurrence the
//                            match in the reference.  ROUGE-L: one wave per reference, the LCS row (<= 128 cells, two per lane) in
//                            registers, one hypothesis token per step: new[j] = max over k <= j of (match ? old[k-1] + 1 : old[k]),
//                            a wave prefix maximum.
// The key packing, the hash, the plain-load probe, the n-gram weight and the wave LCS live in caption_ngram.h, shared with caption_mbr.hip.
// Kernel launches only, no allocation, no host read: capturable.  Lengths read from device memory are clamped before they address
// anything; the only other index that comes from memory is the hash, masked by the capacity.
#include "caption_ngram.h"

namespace sat {
namespace {

__global__ __launch_bounds__(256) void ngram_table_clear_kernel(u64* __restrict__ keys, unsigned* __restrict__ counts, long capacity) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < capacity; i += (long)gridDim.x * 256) { keys[i] = 0; counts[i] = 0; }
}

__global__ __launch_bounds__(256) void ngram_table_add_kernel(const int* __restrict__ refs, const int* __restrict__ ref_len, int R, int T,
                                                              u64* __restrict__ keys, unsigned* __restrict__ counts, long capacity,
                                                              int* __restrict__ error_flag) {
    __shared__ int s_ref[kCaptionMaxRefs * kCaptionMaxLen];
    __shared__ int s_rl[kCaptionMaxRefs];
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int r = 0; r < R; ++r) {
        const int rl = clampi(ref_len[b * R + r], 1, T) - 1;
        if (tid == 0) s_rl[r] = rl;
        for (int j = tid; j < rl; j += 256) s_ref[r * T + j] = key_token(refs[((long)b * R + r) * T + 1 + j]);
    }
    __syncthreads();
    const u64 mask = (u64)capacity - 1;
    for (int it = tid; it < R * T; it += 256) {
        const int r = it / T, i = it - r * T;
        const int left = s_rl[r] - i;                  // tokens from position i to the end of the reference
        if (left < 1) continue;
        const int nmax = left < 4 ? left : 4;
        const int* g = s_ref + r * T + i;
        int seen = 0;                                  // the longest order whose n-gram occurred at an earlier position of the image
        for (int r2 = 0; r2 <= r && seen < nmax; ++r2) {
            const int* o = s_ref + r2 * T;
            const int rl2 = s_rl[r2], end = r2 < r ? rl2 : i;
            for (int j = 0; j < end && seen < nmax; ++j) {
                const int lim = rl2 - j < nmax ? rl2 - j : nmax;
                int m = 0;
                while (m < lim && o[j + m] == g[m]) ++m;
                seen = m > seen ? m : seen;
            }
        }
        for (int n = seen + 1; n <= nmax; ++n) {       // an earlier (n+1)-gram match is an earlier n-gram match: the new ones are a suffix
            const u64 key = pack_ngram(g, n);
            u64 slot = hash_key(key) & mask;
            bool done = false;
            for (long probe = 0; probe < capacity; ++probe) {
                const u64 was = atomicCAS(&keys[slot], 0ULL, key);
                if (was == 0ULL || was == key) { atomicAdd(&counts[slot], 1u); done = true; break; }
                slot = (slot + 1) & mask;
            }
            if (!done) atomicOr(error_flag, 1);
        }
    }
}

// v[k] of thread t belongs to order (t >> 7) + 2 k: out[n] = the sum over the two waves that own order n, every thread gets all four
__device__ __forceinline__ void order_sums(const double (&v)[2], double (*s_red)[2], double (&out)[4]) {
    const double a = wave_sum_f64(v[0]), c = wave_sum_f64(v[1]);
    if ((threadIdx.x & 63) == 0) { s_red[threadIdx.x >> 6][0] = a; s_red[threadIdx.x >> 6][1] = c; }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < 4; ++n) out[n] = s_red[2 * (n & 1)][n >> 1] + s_red[2 * (n & 1) + 1][n >> 1];
    __syncthreads();
}

__global__ __launch_bounds__(256) void caption_consensus_kernel(const int* __restrict__ cap_tokens, const int* __restrict__ cap_len, int W,
                                                                const int* __restrict__ refs, const int* __restrict__ ref_len, int R, int T,
                                                                const u64* __restrict__ keys, const unsigned* __restrict__ counts, long capacity,
                                                                long n_images, double sigma, double* __restrict__ scores) {
    __shared__ int s_hyp[kCaptionMaxLen];
    __shared__ int s_ref[kCaptionMaxRefs * kCaptionMaxLen];
    __shared__ int s_rl[kCaptionMaxRefs];
    __shared__ int s_lcs[kCaptionMaxRefs];
    __shared__ double s_rw[4][kCaptionMaxLen];
    __shared__ double s_red[4][2];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = clampi(cap_len[b], 0, W);
    for (int j = tid; j < H; j += 256) s_hyp[j] = key_token(cap_tokens[(long)b * W + j]);
    for (int r = 0; r < R; ++r) {
        const int rl = clampi(ref_len[b * R + r], 1, T) - 1;
        if (tid == 0) s_rl[r] = rl;
        for (int j = tid; j < rl; j += 256) s_ref[r * T + j] = key_token(refs[((long)b * R + r) * T + 1 + j]);
    }
    __syncthreads();

    // ROUGE-L: wave w takes the references w, w + 4, ...; lane l holds the cells j = l and j = 64 + l of the LCS row
    for (int r = wave; r < R; r += 4) {
        const int lcs = wave_lcs(s_hyp, H, s_ref + r * T, s_rl[r], lane);
        if (lane == 0) s_lcs[r] = lcs;
    }

    // CIDEr-D
    const int pos = tid & 127;
    const double log_n = log((double)n_images);       // on the device, as log(df) is: an n-gram of every image weighs exactly 0
    bool fh[2], fr;
    double wh[2], sq[2], norm_h[4], acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        wh[k] = ngram_weight(s_hyp, H, pos, (tid >> 7) + 2 * k + 1, keys, counts, capacity, log_n, fh[k]);
        sq[k] = wh[k] * wh[k];
    }
    order_sums(sq, s_red, norm_h);                     // (its barriers also publish s_lcs)
#pragma unroll
    for (int n = 0; n < 4; ++n) norm_h[n] = sqrt(norm_h[n]);
    const int len_h = H > 1 ? H - 1 : 0;               // the scorer's "length": the number of bigram positions
    for (int r = 0; r < R; ++r) {
        const int rl = s_rl[r];
        const int* ref = s_ref + r * T;
        double norm_r[4], dot[4], part[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int n = (tid >> 7) + 2 * k + 1;
            const double w = ngram_weight(ref, rl, pos, n, keys, counts, capacity, log_n, fr);
            s_rw[n - 1][pos] = w;
            part[k] = w * w;
        }
        order_sums(part, s_red, norm_r);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int n = (tid >> 7) + 2 * k + 1;
            part[k] = 0.0;
            if (fh[k]) {
                for (int j = 0; j + n <= rl; ++j) {
                    if (same_ngram(ref + j, s_hyp + pos, n)) {                 // the first match is the first occurrence: it holds the weight
                        const double wr = s_rw[n - 1][j];
                        part[k] = (wh[k] < wr ? wh[k] : wr) * wr;
                        break;
                    }
                }
            }
        }
        order_sums(part, s_red, dot);
        const double delta = (double)(len_h - (rl > 1 ? rl - 1 : 0));
        const double penalty = exp(-(delta * delta) / (2.0 * sigma * sigma));
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            double v = dot[n];
            const double nr = sqrt(norm_r[n]);
            if (norm_h[n] != 0.0 && nr != 0.0) v /= norm_h[n] * nr;
            acc[n] += v * penalty;
        }
    }
    if (tid == 0) {
        scores[(long)b * 2] = 10.0 * ((((acc[0] + acc[1]) + acc[2]) + acc[3]) / 4.0 / (double)R);
        double prec = 0.0, rec = 0.0;
        for (int r = 0; r < R && H > 0; ++r) {
            const double p = (double)s_lcs[r] / (double)H, q = s_rl[r] > 0 ? (double)s_lcs[r] / (double)s_rl[r] : 0.0;
            prec = p > prec ? p : prec;
            rec = q > rec ? q : rec;
        }
        const double beta2 = 1.2 * 1.2;
        scores[(long)b * 2 + 1] = prec != 0.0 && rec != 0.0 ? ((1.0 + beta2) * prec * rec) / (rec + beta2 * prec) : 0.0;
    }
}

}  // namespace

size_t ngram_table_bytes(long capacity) { return (size_t)capacity * (sizeof(u64) + sizeof(unsigned)); }

int ngram_table_clear(void* table, long capacity, hipStream_t st) {
    const long blocks = (capacity + 255) / 256;
    hipLaunchKernelGGL(ngram_table_clear_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, (u64*)table,
                       (unsigned*)((u64*)table + capacity), capacity);
    return launch_ok("ngram_table_clear");
}

int ngram_table_add(const int* refs, const int* ref_len, int B, int R, int T, void* table, long capacity, int* error_flag, hipStream_t st) {
    hipLaunchKernelGGL(ngram_table_add_kernel, dim3(B), dim3(256), 0, st, refs, ref_len, R, T, (u64*)table, (unsigned*)((u64*)table + capacity), capacity,
                       error_flag);
    return launch_ok("ngram_table_add");
}

int caption_consensus(const int* cap_tokens, const int* cap_len, int W, const int* refs, const int* ref_len, int B, int R, int T, const void* table,
                      long capacity, long n_images, double sigma, double* scores, hipStream_t st) {
    hipLaunchKernelGGL(caption_consensus_kernel, dim3(B), dim3(256), 0, st, cap_tokens, cap_len, W, refs, ref_len, R, T, (const u64*)table,
                       (const unsigned*)((const u64*)table + capacity), capacity, n_images, sigma, scores);
    return launch_ok("caption_consensus");
}

}  // namespace sat
