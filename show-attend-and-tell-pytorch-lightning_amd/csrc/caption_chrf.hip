// chrF of decoded captions on the device, next to caption_score.hip's BLEU / GLEU statistics and caption_consensus.hip's CIDEr-D /
// ROUGE-L (metrics.py is the specification: chrf_text, chrf_stats, chrf_sentence, chrf).
//
//   A sentence is the code points of its tokens' spellings, whitespace already stripped, concatenated without a separator: character
//   n-grams (n = 1..6) run across word boundaries.  The spelling of the vocabulary lives on the device: word_offsets (V + 1) and
//   word_chars (evaluation.VocabChars).
//
//   caption_chrf_kernel   one workgroup per image.  The hypothesis's characters are gathered into LDS once (a wave prefix sum of the
//                         word lengths places every token), followed by six sentinels that match nothing.  Thread i (strided when the
//                         sentence has more than 256 characters) owns hypothesis position i and walks every earlier position j with a
//                         sliding window of six characters: the length m <= 6 of the common run at (i, j) says for all six orders at
//                         once whether the n-gram at j equals the one at i, and prev[n][i] = the number of earlier positions with the
//                         same n-gram goes to LDS.  Then reference by reference: its characters into LDS, the same walk over the
//                         reference's positions gives c_r[n] = the number of reference positions with i's n-gram, and position i adds
//                         1 to tp_n iff prev[n][i] < c_r[n]; summed over i that is sum over distinct n-grams of min(c_h, c_r).  A run
//                         never extends over a sentence's end (the sentinels), so a position without an n-gram of order n counts
//                         nothing.  tp_n: integer wave sums, then four partial sums in LDS added by thread 0, which also takes the six
//                         F-scores and the running maximum over the references in fp64 (this file is built without FMA contraction).
//                         Everything before the F-scores is integer arithmetic: the same input gives the same bits.
// Kernel launches only, no allocation, no host read: capturable.  Lengths, token ids and offsets read from device memory are clamped
// before they address anything, and characters beyond kChrfMaxChars are dropped (the C ABI refuses sizes that could reach it).
#include "caption_score.h"

namespace sat {
namespace {

constexpr int kOrders = kChrfMaxOrder;
constexpr int kPad = 8;                      // sentinels behind a sentence: a window of six never leaves the array
constexpr int kHypEnd = -2, kRefEnd = -1;    // code points are stored as non-negative ints: the sentinels match nothing, nor each other

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The characters of tokens toks[0..ntok) (ntok <= 128 <= the workgroup) into s_dst, then kPad times `sentinel`; returns their number.
// All 256 threads call it; it ends with a barrier.
__device__ int gather_chars(const int* __restrict__ toks, int ntok, const int* __restrict__ word_offsets, const int* __restrict__ word_chars,
                            int V, int max_word_chars, int total, int* s_dst, int* s_wave, int sentinel) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int start = 0, wl = 0;
    if (tid < ntok) {
        const int tok = toks[tid];
        if (tok >= 0 && tok < V) {                       // a token outside the vocabulary has no characters
            start = clampi(word_offsets[tok], 0, total);
            const int room = total - start < max_word_chars ? total - start : max_word_chars;
            wl = clampi(word_offsets[tok + 1] - start, 0, room);
        }
    }
    int inc = wl;                                        // inclusive prefix sum over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int base = 0, len = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const int t = s_wave[w]; base += w < wave ? t : 0; len += t; }
    len = len < kChrfMaxChars ? len : kChrfMaxChars;
    const int off = base + inc - wl;
    for (int k = 0; k < wl; ++k)
        if (off + k < kChrfMaxChars) s_dst[off + k] = word_chars[start + k] & 0x7fffffff;
    if (tid < kPad) s_dst[len + tid] = sentinel;
    __syncthreads();
    return len;
}

// c[n - 1] += 1 for every n <= the common run of window w (a sentence's position j) and the hypothesis's n-gram h (position i)
__device__ __forceinline__ void count_run(int (&c)[kOrders], const int (&w)[kOrders], const int (&h)[kOrders]) {
    bool eq = true;
#pragma unroll
    for (int n = 0; n < kOrders; ++n) {
        eq = eq && (w[n] == h[n]);
        c[n] += eq ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void caption_chrf_kernel(const int* __restrict__ cap_tokens, const int* __restrict__ cap_len, int W,
                                                           const int* __restrict__ refs, const int* __restrict__ ref_len, int R, int T,
                                                           const int* __restrict__ word_offsets, const int* __restrict__ word_chars, int V,
                                                           int max_word_chars, double beta, double* __restrict__ scores, int* __restrict__ stats) {
    __shared__ int s_hyp[kChrfMaxChars + kPad];
    __shared__ int s_ref[kChrfMaxChars + kPad];
    __shared__ unsigned short s_prev[kOrders][kChrfMaxChars];
    __shared__ int s_wave[4];
    __shared__ int s_red[4][kOrders];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long most = (long)V * max_word_chars;
    const int total = clampi(word_offsets[V], 0, most < 0x7fffffffL ? (int)most : 0x7fffffff);
    const int H = clampi(cap_len[b], 0, W);
    const int Lh = gather_chars(cap_tokens + (long)b * W, H, word_offsets, word_chars, V, max_word_chars, total, s_hyp, s_wave, kHypEnd);

    // the number of earlier hypothesis positions with the same n-gram, all six orders from one walk
    for (int i = tid; i < Lh; i += 256) {
        int h[kOrders], w[kOrders], c[kOrders];
#pragma unroll
        for (int n = 0; n < kOrders; ++n) { h[n] = s_hyp[i + n]; w[n] = s_hyp[n]; c[n] = 0; }
        for (int j = 0; j < i; ++j) {
            count_run(c, w, h);
#pragma unroll
            for (int n = 0; n + 1 < kOrders; ++n) w[n] = w[n + 1];
            w[kOrders - 1] = s_hyp[j + kOrders];
        }
#pragma unroll
        for (int n = 0; n < kOrders; ++n) s_prev[n][i] = (unsigned short)c[n];
    }
    // (every thread reads back only the s_prev entries it wrote itself: no barrier needed here)

    const double beta2 = beta * beta;
    double best = 0.0;
    for (int r = 0; r < R; ++r) {
        const int rl = clampi(ref_len[b * R + r], 1, T) - 1;
        const int Lr = gather_chars(refs + ((long)b * R + r) * T + 1, rl, word_offsets, word_chars, V, max_word_chars, total, s_ref, s_wave, kRefEnd);
        int tp[kOrders];
#pragma unroll
        for (int n = 0; n < kOrders; ++n) tp[n] = 0;
        for (int i = tid; i < Lh; i += 256) {
            int h[kOrders], w[kOrders], c[kOrders];
#pragma unroll
            for (int n = 0; n < kOrders; ++n) { h[n] = s_hyp[i + n]; w[n] = s_ref[n]; c[n] = 0; }
            for (int j = 0; j < Lr; ++j) {
                count_run(c, w, h);
#pragma unroll
                for (int n = 0; n + 1 < kOrders; ++n) w[n] = w[n + 1];
                w[kOrders - 1] = s_ref[j + kOrders];
            }
#pragma unroll
            for (int n = 0; n < kOrders; ++n) tp[n] += (int)s_prev[n][i] < c[n] ? 1 : 0;
        }
#pragma unroll
        for (int n = 0; n < kOrders; ++n) {
            int v = tp[n];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) s_red[wave][n] = v;
        }
        __syncthreads();
        if (tid == 0) {
            double sum = 0.0;
            for (int n = 0; n < kOrders; ++n) {
                const int t = ((s_red[0][n] + s_red[1][n]) + s_red[2][n]) + s_red[3][n];
                const int nh = Lh - n > 0 ? Lh - n : 0, nr = Lr - n > 0 ? Lr - n : 0;      // positions of order n + 1
                double f = 1e-16;
                if (nh != 0 && nr != 0 && t != 0) {
                    const double p = (double)t / (double)nh, q = (double)t / (double)nr;
                    f = ((1.0 + beta2) * (p * q)) / (beta2 * p + q);
                }
                sum += f;
                if (stats) stats[((long)b * R + r) * 8 + n] = t;
            }
            if (stats) { stats[((long)b * R + r) * 8 + 6] = Lh; stats[((long)b * R + r) * 8 + 7] = Lr; }
            const double s = sum / 6.0;
            if (r == 0 || s > best) best = s;              // the first maximum wins
        }
        // the next gather's first barrier orders thread 0's reads of s_red before the next writes; s_ref is rewritten only behind it
    }
    if (tid == 0) scores[b] = best;
}

}  // namespace

int caption_chrf(const int* cap_tokens, const int* cap_len, int W, const int* refs, const int* ref_len, int B, int R, int T, const int* word_offsets,
                 const int* word_chars, int V, int max_word_chars, double beta, double* scores, int* stats, hipStream_t st) {
    hipLaunchKernelGGL(caption_chrf_kernel, dim3(B), dim3(256), 0, st, cap_tokens, cap_len, W, refs, ref_len, R, T, word_offsets, word_chars, V,
                       max_word_chars, beta, scores, stats);
    return launch_ok("caption_chrf");
}

}  // namespace sat
