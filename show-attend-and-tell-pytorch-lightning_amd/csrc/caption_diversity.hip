// Diversity of the finished beam on the device: the integers distinct-n, mBLEU (self-BLEU) and the share of unique captions are made of
// (metrics.diversity_stats / diversity_per_hypothesis are the specification; the column table is in include/sat_hip.h,
// sat_caption_diversity), and the vocabulary the selected captions use (sat_caption_vocab_usage).
//
//   caption_diversity_kernel   one workgroup of 256 threads per image, integers only.  LDS: the K x W tokens as the n-gram keys see them
//                              (16 bit, 8 KB), one order's sort pairs (64-bit packed key, 32 KB; hypothesis << 7 | position, 8 KB), the
//                              per-hypothesis counts of the sorted runs (4 KB) and the clipped counts back in hypothesis order (4 KB):
//                              56 KB, 58 KB with the reduction scratch, of the 64.
//     lengths                  one thread per hypothesis: the closest other length (a tie goes to the shorter); one thread per pair
//                              j < i marks i as a duplicate of an earlier hypothesis (equal length, equal tokens).
//     per order n = 1..4       every n-gram position writes one (key, hypothesis << 7 | position) pair, padded to a power of two with
//                              pairs that sort last; a bitonic network sorts them in LDS by key, then hypothesis, then position.  On the
//                              sorted pairs a run of equal keys is one distinct n-gram, and inside it the positions of one hypothesis are
//                              contiguous: the first position of each such stretch counts it (c_i, at most W), the first position of each
//                              run walks its stretches (at most K) for the largest and second-largest c and the owner of the largest, and
//                              leaves min(c_i, owner == i ? second : largest) -- the count clipped by the best OTHER hypothesis -- at
//                              the stretch's first position in hypothesis order, where one wave per hypothesis sums them.
//                              O(P log^2 P) for P <= 4096 positions; nothing compares every position with every other.
//   caption_vocab_usage_kernel one thread per token slot, counts[token] += 1 by integer atomicAdd (a sum: the order does not matter).
// The diversity kernel has no atomics and no floating point: the same input gives the same bits.  Lengths and counts read from device
// memory are clamped before they address anything, tokens are clamped by key_token; every LDS index is below K * W <= 4096 or below the
// padded sort size <= 4096 by construction.  One launch each, no allocation, no host read: capturable.
#include "caption_ngram.h"

namespace sat {
namespace {

constexpr int kDivMaxPos = kMbrMaxHyps * kCaptionMaxLen;       // 4096 n-gram positions per image and order at the limits
static_assert(kCaptionMaxLen == 128 && kMbrMaxHyps == 32, "hypothesis << 7 | position is 12 bits; a count fits 8 bits");

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void caption_diversity_kernel(const int* __restrict__ hyp_tokens, const int* __restrict__ hyp_len,
                                                                const int* __restrict__ hyp_count, int K, int W, int* __restrict__ stats,
                                                                int* __restrict__ per_hyp) {
    __shared__ u64 s_key[kDivMaxPos];                  // sort pair: the packed n-gram
    __shared__ unsigned short s_at[kDivMaxPos];        // sort pair: hypothesis << 7 | position
    __shared__ unsigned short s_tok[kDivMaxPos];       // [k * W + j]: 1..65535
    __shared__ unsigned char s_cnt[kDivMaxPos];        // [sorted index of a stretch's first pair]: its length
    __shared__ unsigned char s_clip[kDivMaxPos];       // [hypothesis << 7 | position]: the clipped count of the stretch that starts there
    __shared__ int s_red[256];
    __shared__ int s_len[kMbrMaxHyps], s_off[kMbrMaxHyps + 1], s_dup[kMbrMaxHyps], s_close[kMbrMaxHyps];
    __shared__ int s_clipped[4 * kMbrMaxHyps], s_distinct[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = clampi(hyp_count[b], 0, K);
    if (tid < kMbrMaxHyps) {
        s_len[tid] = tid < F ? clampi(hyp_len[(long)b * K + tid], 0, W) : 0;
        s_dup[tid] = 0;
    }
    if (tid < 4 * kMbrMaxHyps) s_clipped[tid] = 0;
    if (tid < 4) s_distinct[tid] = 0;
    __syncthreads();
    for (int it = tid; it < F * W; it += 256) {
        const int k = it / W, j = it - k * W;
        if (j < s_len[k]) s_tok[it] = (unsigned short)key_token(hyp_tokens[(long)b * K * W + it]);
    }
    __syncthreads();

    if (tid < F) {                                     // closest_ref_length over the others: min by (|l_j - l_i|, l_j)
        const int li = s_len[tid];
        int best = 0, best_d = 1 << 30;
        for (int j = 0; j < F; ++j) {
            if (j == tid) continue;
            const int lj = s_len[j], d = lj > li ? lj - li : li - lj;
            if (d < best_d || (d == best_d && lj < best)) { best_d = d; best = lj; }
        }
        s_close[tid] = best;
    }
    for (int p = tid; p < kMbrMaxHyps * kMbrMaxHyps; p += 256) {          // pair (i, j < i): is i a copy of j
        const int i = p >> 5, j = p & 31;
        if (i >= F || j >= i || s_len[i] != s_len[j]) continue;
        const unsigned short *hi = s_tok + i * W, *hj = s_tok + j * W;
        bool eq = true;
        for (int g = 0; g < s_len[i] && eq; ++g) eq = hi[g] == hj[g];
        if (eq) s_dup[i] = 1;                          // several pairs may store the same 1
    }

    for (int n = 1; n <= 4; ++n) {
        __syncthreads();                               // the previous order is read off
        if (tid == 0) {
            int o = 0;
            for (int k = 0; k < F; ++k) { s_off[k] = o; o += s_len[k] >= n ? s_len[k] - n + 1 : 0; }
            s_off[kMbrMaxHyps] = o;
        }
        __syncthreads();
        const int P = s_off[kMbrMaxHyps];              // <= F * W <= 4096
        if (P == 0) continue;                          // the same for every thread
        int N = 2;
        while (N < P) N <<= 1;                         // <= 4096
        for (int it = tid; it < F * W; it += 256) {
            const int k = it / W, j = it - k * W;
            if (j + n > s_len[k]) continue;
            u64 key = 0;
            for (int q = 0; q < n; ++q) key |= (u64)s_tok[it + q] << (16 * q);
            s_key[s_off[k] + j] = key;
            s_at[s_off[k] + j] = (unsigned short)(k << 7 | j);
        }
        for (int it = P + tid; it < N; it += 256) { s_key[it] = ~0ULL; s_at[it] = 0xFFFF; }     // after every real pair, the all-ones key included
        for (int it = tid; it < F * kCaptionMaxLen; it += 256) s_clip[it] = 0;
        __syncthreads();

        for (int k = 2; k <= N; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (N >> 1); t += 256) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;            // i < l < N
                    const u64 ka = s_key[i], kb = s_key[l];
                    const unsigned short aa = s_at[i], ab = s_at[l];
                    const bool after = ka > kb || (ka == kb && aa > ab);
                    if (after == ((i & k) == 0)) { s_key[i] = kb; s_key[l] = ka; s_at[i] = ab; s_at[l] = aa; }
                }
                __syncthreads();
            }
        }

        int runs = 0;
        for (int t = tid; t < P; t += 256) {
            const u64 key = s_key[t];
            const int h = s_at[t] >> 7;
            const bool new_key = t == 0 || s_key[t - 1] != key;
            runs += new_key ? 1 : 0;
            if (new_key || (s_at[t - 1] >> 7) != h) {
                int c = 1;
                while (t + c < P && s_key[t + c] == key && (s_at[t + c] >> 7) == h) ++c;      // <= W positions of one hypothesis
                s_cnt[t] = (unsigned char)c;
            }
        }
        s_red[tid] = runs;
        __syncthreads();
        for (int t = tid; t < P; t += 256) {
            const u64 key = s_key[t];
            if (t != 0 && s_key[t - 1] == key) continue;
            int largest = 0, second = 0, owner = -1;
            for (int u = t; u < P && s_key[u] == key;) {                                   // the stretches of the run: <= F
                const int c = s_cnt[u] > 0 ? s_cnt[u] : 1;
                if (c > largest) { second = largest; largest = c; owner = s_at[u] >> 7; }
                else if (c > second) second = c;
                u += c;
            }
            for (int u = t; u < P && s_key[u] == key;) {
                const int c = s_cnt[u] > 0 ? s_cnt[u] : 1, lim = (s_at[u] >> 7) == owner ? second : largest;
                s_clip[s_at[u] & (kDivMaxPos - 1)] = (unsigned char)(c < lim ? c : lim);
                u += c;
            }
        }
        __syncthreads();
        for (int i = wave; i < F; i += 4) {
            const int v = wave_sum_i32((int)s_clip[i * kCaptionMaxLen + lane] + (int)s_clip[i * kCaptionMaxLen + 64 + lane]);
            if (lane == 0) s_clipped[(n - 1) * kMbrMaxHyps + i] = v;
        }
        if (wave == 0) {
            const int v = wave_sum_i32(s_red[lane] + s_red[64 + lane] + s_red[128 + lane] + s_red[192 + lane]);
            if (lane == 0) s_distinct[n - 1] = v;
        }
    }
    __syncthreads();

    const bool others = F >= 2;                        // fewer than two hypotheses: nothing to compare with, columns 10..19 are 0
    if (tid == 0) {
        int* out = stats + (long)b * 20;
        int unique = 0, len_sum = 0, close_sum = 0;
        for (int k = 0; k < F; ++k) { unique += s_dup[k] ? 0 : 1; len_sum += s_len[k]; close_sum += s_close[k]; }
        for (int n = 1; n <= 4; ++n) {
            int positions = 0, clipped = 0, total = 0;
            for (int k = 0; k < F; ++k) {
                const int p = s_len[k] - n + 1;
                positions += p > 0 ? p : 0;
                total += p > 1 ? p : 1;
                clipped += s_clipped[(n - 1) * kMbrMaxHyps + k];
            }
            out[n - 1] = s_distinct[n - 1];
            out[3 + n] = positions;
            out[9 + n] = others ? clipped : 0;
            out[13 + n] = others ? total : 0;
        }
        out[8] = F;
        out[9] = unique;
        out[18] = others ? len_sum : 0;
        out[19] = others ? close_sum : 0;
    }
    if (per_hyp != nullptr && tid < K) {
        int* row = per_hyp + ((long)b * K + tid) * 10;
        const bool live = others && tid < F;
        for (int n = 1; n <= 4; ++n) {
            const int p = s_len[tid] - n + 1;
            row[n - 1] = live ? s_clipped[(n - 1) * kMbrMaxHyps + tid] : 0;
            row[3 + n] = live ? (p > 1 ? p : 1) : 0;
        }
        row[8] = live ? s_len[tid] : 0;
        row[9] = live ? s_close[tid] : 0;
    }
}

__global__ __launch_bounds__(256) void caption_vocab_usage_kernel(const int* __restrict__ cap_tokens, const int* __restrict__ cap_len, int W, long total,
                                                                  int V, int* __restrict__ counts) {
    const long it = (long)blockIdx.x * 256 + threadIdx.x;
    if (it >= total) return;
    const long b = it / W;
    const int j = (int)(it - b * W);
    if (j >= clampi(cap_len[b], 0, W)) return;
    const int t = cap_tokens[it];
    if (t >= 0 && t < V) atomicAdd(counts + t, 1);
}

}  // namespace

int caption_diversity(const int* hyp_tokens, const int* hyp_len, const int* hyp_count, int B, int K, int W, int* stats, int* per_hyp, hipStream_t st) {
    hipLaunchKernelGGL(caption_diversity_kernel, dim3(B), dim3(256), 0, st, hyp_tokens, hyp_len, hyp_count, K, W, stats, per_hyp);
    return launch_ok("caption_diversity");
}

int caption_vocab_usage(const int* cap_tokens, const int* cap_len, int W, int B, int V, int* counts, hipStream_t st) {
    const long total = (long)B * W;
    hipLaunchKernelGGL(caption_vocab_usage_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, cap_tokens, cap_len, W, total, V, counts);
    return launch_ok("caption_vocab_usage");
}

}  // namespace sat
