// Consensus (minimum-Bayes-risk) reranking of the finished beam on the device: every hypothesis of an image is scored against the
// image's other hypotheses with the metric the captions are evaluated on, and the one that agrees most with the rest wins
// (metrics.consensus_utilities is the specification; the definition is in include/sat_hip.h, sat_caption_mbr).
//
//   caption_mbr_kernel   one workgroup of 256 threads per image, all arithmetic in fp64 (this file is built without FMA contraction).
//                        LDS: the K x W tokens as the keys see them (<= 16 KB), one order's weights (K x W fp64, <= 32 KB) with their
//                        first-occurrence flags (4 KB), the K x K LCS lengths (1 KB): 54 KB of the 64.
//     ROUGE-L            (skipped when w_rouge == 0) one wave per unordered pair i < j, the LCS row in registers (wave_lcs); the LCS is
//                        symmetric, rouge(i|j) and rouge(j|i) differ in which length is the precision's.
//     CIDEr-D            (skipped when w_cider == 0) order by order, n = 1..4: every hypothesis's weights tf * (log N - log max(1, df))
//                        at the first occurrence of each n-gram, one probe per distinct n-gram with plain loads (the table was built
//                        by earlier launches); the norms, one thread per hypothesis summing in position order; then one thread per
//                        ordered pair (i, j), at most four pairs a thread, sums min(w_i[g], w_j[g]) * w_j[g] over the first
//                        occurrences g of h_i in position order -- the order metrics.cider_d sums in -- divides by the norms and
//                        applies the Gaussian length penalty.  The four orders add up in a register: ((t1 + t2) + t3) + t4.
//     utilities          the gains go to LDS (over the weights, which are done), one thread per hypothesis takes the q-weighted mean
//                        over j != i in ascending j; thread 0 takes the first maximum.
// No atomics and no cross-thread floating-point reduction: every sum is one thread's loop in a fixed order, the same inputs give the
// same bits.  Lengths and counts read from device memory are clamped before they address anything; the only other index that comes
// from memory is the hash, masked by the capacity.  One launch, no allocation, no host read: capturable.
#include "caption_ngram.h"

namespace sat {
namespace {

__global__ __launch_bounds__(256) void caption_mbr_kernel(const int* __restrict__ hyp_tokens, const int* __restrict__ hyp_len, const int* __restrict__ hyp_count,
                                                          const float* __restrict__ hyp_logp, int K, int W, const u64* __restrict__ keys,
                                                          const unsigned* __restrict__ counts, long capacity, long n_images, double sigma, double w_cider,
                                                          double w_rouge, double alpha, double* __restrict__ utilities, int* __restrict__ winner) {
    __shared__ int s_tok[kMbrMaxHyps * kCaptionMaxLen];
    __shared__ double s_w[kMbrMaxHyps * kCaptionMaxLen];
    __shared__ unsigned char s_first[kMbrMaxHyps * kCaptionMaxLen];
    __shared__ unsigned char s_lcs[kMbrMaxHyps * kMbrMaxHyps];
    __shared__ int s_len[kMbrMaxHyps];
    __shared__ double s_norm[kMbrMaxHyps];
    __shared__ double s_q[kMbrMaxHyps];
    __shared__ double s_util[kMbrMaxHyps];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = clampi(hyp_count[b], 0, K);
    if (tid < K) s_len[tid] = tid < F ? clampi(hyp_len[(long)b * K + tid], 0, W) : 0;
    __syncthreads();
    for (int it = tid; it < F * W; it += 256) {
        const int k = it / W, j = it - k * W;
        if (j < s_len[k]) s_tok[it] = key_token(hyp_tokens[(long)b * K * W + it]);
    }
    __syncthreads();

    if (w_rouge != 0.0) {                              // wave w takes the pairs w, w + 4, ... of (0,1), (0,2), ..., (F-2,F-1)
        int u = 0;
        for (int i = 0; i < F; ++i)
            for (int j = i + 1; j < F; ++j, ++u) {
                if ((u & 3) != wave) continue;
                const int lcs = wave_lcs(s_tok + i * W, s_len[i], s_tok + j * W, s_len[j], lane);
                if (lane == 0) { s_lcs[i * K + j] = (unsigned char)lcs; s_lcs[j * K + i] = (unsigned char)lcs; }
            }
    }

    double acc[4] = {0.0, 0.0, 0.0, 0.0};              // pair tid + 256 q: the sum over the orders so far
    if (w_cider != 0.0) {
        const double log_n = log((double)n_images);   // on the device, as log(df) is: an n-gram of every image weighs exactly 0
#pragma unroll
        for (int n = 1; n <= 4; ++n) {
            for (int it = tid; it < F * W; it += 256) {
                const int k = it / W;
                bool first;
                s_w[it] = ngram_weight(s_tok + k * W, s_len[k], it - k * W, n, keys, counts, capacity, log_n, first);
                s_first[it] = first ? 1 : 0;
            }
            __syncthreads();
            if (tid < F) {
                double sq = 0.0;
                for (int g = 0; g + n <= s_len[tid]; ++g) { const double w = s_w[tid * W + g]; sq += w * w; }     // off the first occurrences: + 0
                s_norm[tid] = sqrt(sq);
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int p = tid + 256 * q, i = p / K, j = p - i * K;
                if (i >= F || j >= F || i == j) continue;
                const int li = s_len[i], lj = s_len[j];
                const int *hi = s_tok + i * W, *hj = s_tok + j * W;
                double val = 0.0;
                for (int g = 0; g + n <= li; ++g) {
                    if (!s_first[i * W + g]) continue;
                    for (int m = 0; m + n <= lj; ++m) {
                        if (same_ngram(hj + m, hi + g, n)) {                   // the first match is the first occurrence: it holds the weight
                            const double wh = s_w[i * W + g], wr = s_w[j * W + m];
                            val += (wh < wr ? wh : wr) * wr;
                            break;
                        }
                    }
                }
                const double ni = s_norm[i], nj = s_norm[j];
                if (ni != 0.0 && nj != 0.0) val /= ni * nj;
                const double delta = (double)((li > 1 ? li - 1 : 0) - (lj > 1 ? lj - 1 : 0));
                acc[q] = acc[q] + val * exp(-(delta * delta) / (2.0 * sigma * sigma));
            }
            __syncthreads();                           // the next order overwrites the weights
        }
    }
    __syncthreads();                                   // publishes s_lcs when the CIDEr phase is skipped

    double* s_gain = s_w;                              // K x K gains over the weights, which nobody reads any more
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int p = tid + 256 * q, i = p / K, j = p - i * K;
        if (i >= F || j >= F || i == j) continue;
        double gain = 0.0;
        if (w_cider != 0.0) gain = gain + w_cider * (10.0 * (acc[q] / 4.0 / 1.0));
        if (w_rouge != 0.0) {
            const int li = s_len[i], lj = s_len[j], lcs = s_lcs[i * K + j];
            double rouge = 0.0;
            if (li > 0) {
                const double prec = (double)lcs / (double)li, rec = lj > 0 ? (double)lcs / (double)lj : 0.0;
                const double beta2 = 1.2 * 1.2;
                if (prec != 0.0 && rec != 0.0) rouge = ((1.0 + beta2) * prec * rec) / (rec + beta2 * prec);
            }
            gain = gain + w_rouge * rouge;
        }
        s_gain[p] = gain;
    }
    if (tid < F) {
        double q = 1.0;
        if (alpha != 0.0) {
            double top = (double)hyp_logp[(long)b * K];
            for (int k = 1; k < F; ++k) { const double s = (double)hyp_logp[(long)b * K + k]; top = s > top ? s : top; }
            q = exp(alpha * ((double)hyp_logp[(long)b * K + tid] - top));
        }
        s_q[tid] = q;
    }
    __syncthreads();
    if (tid < K) {
        double u = 0.0;
        if (tid < F) {
            double num = 0.0, den = 0.0;
            for (int j = 0; j < F; ++j) {
                if (j == tid) continue;
                num += s_q[j] * s_gain[tid * K + j];
                den += s_q[j];
            }
            if (den != 0.0) u = num / den;             // F == 1, or every other weight underflowed: 0
        }
        s_util[tid] = u;
        utilities[(long)b * K + tid] = u;
    }
    __syncthreads();
    if (tid == 0) {
        int best = 0;
        for (int i = 1; i < F; ++i) best = s_util[i] > s_util[best] ? i : best;       // the first maximum in append order
        winner[b] = best;
    }
}

}  // namespace

int caption_mbr(const int* hyp_tokens, const int* hyp_len, const int* hyp_count, const float* hyp_logp, int B, int K, int W, const void* table, long capacity,
                long n_images, double sigma, double w_cider, double w_rouge, double alpha, double* utilities, int* winner, hipStream_t st) {
    hipLaunchKernelGGL(caption_mbr_kernel, dim3(B), dim3(256), 0, st, hyp_tokens, hyp_len, hyp_count, hyp_logp, K, W, (const u64*)table,
                       (const unsigned*)((const u64*)table + capacity), capacity, n_images, sigma, w_cider, w_rouge, alpha, utilities, winner);
    return launch_ok("caption_mbr");
}

}  // namespace sat
