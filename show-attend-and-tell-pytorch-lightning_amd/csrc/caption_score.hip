// Scoring of decoded captions on the device (the reference's evaluate.ipynb loop: SAT.val_batch = forward + score_captions,
// model.py:449-472 and 646-682), so that a validation batch goes from image to metric statistics without a host round trip.
//
//   beam_select_kernel     one workgroup per image: rescore the finished hypotheses the batched search left on the device
//                          (model.py:341-348: none / LN / WR / BAR, fp32, this file is built without FMA contraction), take the
//                          first maximum in append order (list.index(max(...))), walk the parent rows from the step it ended at
//                          down to step 1 (at most max_gen_length + 1 dependent loads, one lane) and gather its tokens and,
//                          when asked, its attention maps.
//   beam_select_at_kernel  the same back-trace and gather (beam_trace_gather) for a winner the caller names (consensus reranking).
//   beam_hypotheses_kernel one thread per (image, finished slot): the back-trace of every finished hypothesis, tokens only.
//   caption_stats_kernel   one workgroup per image: the integers nltk's corpus BLEU and GLEU sum per segment (metrics.py is the
//                          specification).  Hypothesis and references are staged in LDS; one thread per (order n, hypothesis
//                          position i): if i is the first occurrence of its n-gram in the hypothesis it counts the n-gram in the
//                          hypothesis and in every reference (brute force: tens of thousands of short compares per image) and adds
//                          min(count, max over references) to the clipped matches of order n and min(count, count in reference r)
//                          to the GLEU true positives of reference r.  Integer LDS atomics: the sums do not depend on the order.
//   caption_cosine_kernel  one workgroup per image: mean embedding of the hypothesis and of each reference (rows gathered in
//                          fp32, summed in token order, coalesced over the embedding dimension), F.cosine_similarity as torch 2
//                          defines it: sum_d (a_d / max(|a|, eps)) (b_d / max(|b|, eps)), eps = 1e-8; the maximum over the
//                          references (NaN propagates, as torch.max does).
// Kernel launches only, no allocation, no host read beyond the sizes: capturable.  Indices that come from device memory are
// clamped to their ranges before they address anything (a corrupt back-trace gives a wrong caption, never a stray access); a
// token outside [0, V) contributes NaN to the cosine instead of being read.
#include "caption_score.h"

#include <math.h>

namespace sat {
namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The back-trace and the gather of hypothesis `bi` of image b (-1: none, an empty caption), shared by beam_select_kernel and
// beam_select_at_kernel; called by the whole workgroup, `bv` is the score thread 0 reports.
__device__ __forceinline__ void beam_trace_gather(const int* __restrict__ tok_in, const int* __restrict__ prev_row, const int* __restrict__ fin_step,
                                                  const int* __restrict__ fin_row, const float* __restrict__ fin_score,
                                                  const float* __restrict__ alpha_hist, int B, int K, int S, int L, int pad_id, int b, int bi, float bv,
                                                  int* __restrict__ cap_tokens, int* __restrict__ cap_len, float* __restrict__ cap_score,
                                                  float* __restrict__ cap_raw, int* __restrict__ cap_step, float* __restrict__ cap_alpha, int* s_rows,
                                                  int* s_step) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        int step = 0, cur = 0; float raw = 0.f;
        if (bi >= 0) { step = clampi(fin_step[b * K + bi], 0, S); cur = clampi(fin_row[b * K + bi], 0, K - 1); raw = fin_score[b * K + bi]; }
        for (int s = step; s >= 0; --s) {
            s_rows[s] = cur;
            if (s > 0) cur = clampi(prev_row[((long)s * B + b) * K + cur], 0, K - 1);
        }
        *s_step = step;
        cap_len[b] = step; cap_step[b] = step; cap_score[b] = bv; cap_raw[b] = raw;
    }
    __syncthreads();
    const int step = *s_step, W = S + 1;
    // tokens fed at steps 1..step (top_preds[:, i][1:-1], model.py:412): without START and without the last prediction
    for (int j = tid; j < W; j += 256)
        cap_tokens[(long)b * W + j] = j < step ? tok_in[((long)(j + 1) * B + b) * K + s_rows[j + 1]] : pad_id;
    if (cap_alpha) {                                   // maps of steps 0..step-1 (alphas[:, i][1:-1], model.py:413), zero beyond
        for (int idx = tid; idx < S * L; idx += 256) {
            const int s = idx / L, l = idx - s * L;
            cap_alpha[(long)b * S * L + idx] = s < step ? alpha_hist[(((long)s * B + b) * K + s_rows[s]) * L + l] : 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void beam_select_kernel(const int* __restrict__ tok_in, const int* __restrict__ prev_row, const int* __restrict__ fin_count,
                                                          const int* __restrict__ fin_step, const int* __restrict__ fin_row,
                                                          const float* __restrict__ fin_score, const float* __restrict__ fin_mean,
                                                          const float* __restrict__ alpha_hist, int B, int K, int S, int L, int method, float reward,
                                                          int pad_id, int* __restrict__ cap_tokens, int* __restrict__ cap_len, float* __restrict__ cap_score,
                                                          float* __restrict__ cap_raw, int* __restrict__ cap_step, float* __restrict__ cap_alpha) {
    __shared__ int s_rows[kCaptionMaxLen];
    __shared__ int s_step;
    const int b = blockIdx.x, tid = threadIdx.x;
    float bv = 0.f; int bi = -1;
    if (tid < 64) {
        const int fc = clampi(fin_count[b], 0, K);
        for (int f = tid; f < fc; f += 64) {
            const float s = fin_score[b * K + f];
            const float stepf = (float)fin_step[b * K + f];
            float v = s;
            if (method == 1) v = s / stepf;
            else if (method == 2) v = s + reward * stepf;
            else if (method == 3) v = s + reward * (-fin_mean[b * K + f]);
            if (bi < 0 || v > bv) { bv = v; bi = f; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
            if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
        }
        if (bi < 0) bv = -INFINITY;                    // no finished hypothesis (cannot happen for max_gen_length >= 1): an empty caption
    }
    beam_trace_gather(tok_in, prev_row, fin_step, fin_row, fin_score, alpha_hist, B, K, S, L, pad_id, b, bi, bv, cap_tokens, cap_len, cap_score, cap_raw,
                      cap_step, cap_alpha, s_rows, &s_step);
}

// sat_beam_select with the winner given: pick[b] clamped into the finished hypotheses of image b
__global__ __launch_bounds__(256) void beam_select_at_kernel(const int* __restrict__ tok_in, const int* __restrict__ prev_row, const int* __restrict__ fin_count,
                                                             const int* __restrict__ fin_step, const int* __restrict__ fin_row,
                                                             const float* __restrict__ fin_score, const float* __restrict__ alpha_hist,
                                                             const int* __restrict__ pick, const double* __restrict__ pick_score, int B, int K, int S, int L,
                                                             int pad_id, int* __restrict__ cap_tokens, int* __restrict__ cap_len, float* __restrict__ cap_score,
                                                             float* __restrict__ cap_raw, int* __restrict__ cap_step, float* __restrict__ cap_alpha) {
    __shared__ int s_rows[kCaptionMaxLen];
    __shared__ int s_step;
    const int b = blockIdx.x;
    float bv = 0.f; int bi = -1;
    if (threadIdx.x == 0) {
        const int fc = clampi(fin_count[b], 0, K);
        const int p = clampi(pick[b], 0, fc > 0 ? fc - 1 : 0);
        if (fc > 0) bi = p;
        if (pick_score) bv = (float)pick_score[b * K + p];
        else bv = bi >= 0 ? fin_score[b * K + bi] : -INFINITY;         // no finished hypothesis: as beam_select_kernel
    }
    beam_trace_gather(tok_in, prev_row, fin_step, fin_row, fin_score, alpha_hist, B, K, S, L, pad_id, b, bi, bv, cap_tokens, cap_len, cap_score, cap_raw,
                      cap_step, cap_alpha, s_rows, &s_step);
}

// every finished hypothesis of every image: one thread per (image, finished slot) walks the parent rows from the step the hypothesis
// ended at down to step 1, as beam_trace_gather does for the winner, and writes the token of every step on the way
__global__ __launch_bounds__(256) void beam_hypotheses_kernel(const int* __restrict__ tok_in, const int* __restrict__ prev_row, const int* __restrict__ fin_count,
                                                              const int* __restrict__ fin_step, const int* __restrict__ fin_row, int B, int K, int S,
                                                              int pad_id, int* __restrict__ hyp_tokens, int* __restrict__ hyp_len) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * K) return;
    const int b = (int)(idx / K), f = (int)(idx - (long)b * K), W = S + 1;
    int step = 0, cur = 0;
    if (f < clampi(fin_count[b], 0, K)) { step = clampi(fin_step[idx], 0, S); cur = clampi(fin_row[idx], 0, K - 1); }
    int* out = hyp_tokens + idx * W;
    for (int j = W - 1; j >= step; --j) out[j] = pad_id;
    for (int s = step; s >= 1; --s) {
        out[s - 1] = tok_in[((long)s * B + b) * K + cur];
        cur = clampi(prev_row[((long)s * B + b) * K + cur], 0, K - 1);
    }
    hyp_len[idx] = step;
}

__device__ __forceinline__ bool same_ngram(const int* a, const int* b, int n) {
    bool eq = true;
    for (int q = 0; q < n; ++q) eq = eq && (a[q] == b[q]);
    return eq;
}

// stage the hypothesis and the references (c[1:l]) of image b in LDS; returns the hypothesis length
__device__ __forceinline__ int stage_tokens(const int* __restrict__ cap_tokens, const int* __restrict__ cap_len, int W, const int* __restrict__ refs,
                                            const int* __restrict__ ref_len, int b, int R, int T, int* s_hyp, int* s_ref, int* s_rl) {
    const int tid = threadIdx.x;
    const int H = clampi(cap_len[b], 0, W);
    for (int j = tid; j < H; j += 256) s_hyp[j] = cap_tokens[(long)b * W + j];
    for (int r = 0; r < R; ++r) {
        const int rl = clampi(ref_len[b * R + r], 1, T) - 1;
        if (tid == 0) s_rl[r] = rl;
        for (int j = tid; j < rl; j += 256) s_ref[r * T + j] = refs[((long)b * R + r) * T + 1 + j];
    }
    return H;
}

__global__ __launch_bounds__(256) void caption_stats_kernel(const int* __restrict__ cap_tokens, const int* __restrict__ cap_len, int W,
                                                            const int* __restrict__ refs, const int* __restrict__ ref_len, int R, int T,
                                                            int* __restrict__ stats) {
    __shared__ int s_hyp[kCaptionMaxLen];
    __shared__ int s_ref[kCaptionMaxRefs * kCaptionMaxLen];
    __shared__ int s_rl[kCaptionMaxRefs];
    __shared__ int s_clip[4];
    __shared__ int s_tp[kCaptionMaxRefs];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int H = stage_tokens(cap_tokens, cap_len, W, refs, ref_len, b, R, T, s_hyp, s_ref, s_rl);
    if (tid < 4) s_clip[tid] = 0;
    if (tid < kCaptionMaxRefs) s_tp[tid] = 0;
    __syncthreads();
    for (int it = tid; it < 4 * H; it += 256) {
        const int n = it / H + 1, i = it - (n - 1) * H;
        if (i + n > H) continue;
        const int* g = s_hyp + i;
        bool first = true;
        for (int j = 0; j < i && first; ++j) first = !same_ngram(s_hyp + j, g, n);
        if (!first) continue;                          // a distinct n-gram is counted once, at its first position
        int c = 1;
        for (int j = i + 1; j + n <= H; ++j) c += same_ngram(s_hyp + j, g, n) ? 1 : 0;
        int mx = 0;
        for (int r = 0; r < R; ++r) {
            const int rl = s_rl[r];
            int cr = 0;
            for (int j = 0; j + n <= rl; ++j) cr += same_ngram(s_ref + r * T + j, g, n) ? 1 : 0;
            mx = cr > mx ? cr : mx;
            const int tp = c < cr ? c : cr;
            if (tp) atomicAdd(&s_tp[r], tp);
        }
        const int cl = c < mx ? c : mx;
        if (cl) atomicAdd(&s_clip[n - 1], cl);
    }
    __syncthreads();
    if (tid == 0) {
        int* o = stats + (long)b * 12;
        int tpfp = 0;
        for (int n = 1; n <= 4; ++n) {
            const int cnt = H - n + 1;
            o[n - 1] = s_clip[n - 1];
            o[4 + n - 1] = cnt > 1 ? cnt : 1;          // max(1, .) per segment, as modified_precision
            tpfp += cnt > 0 ? cnt : 0;
        }
        int close = s_rl[0];
        long best_tp = 0, best_total = 0;
        for (int r = 0; r < R; ++r) {
            const int rl = s_rl[r];
            const int d = rl > H ? rl - H : H - rl, dc = close > H ? close - H : H - close;
            if (d < dc || (d == dc && rl < close)) close = rl;          // the tie goes to the shorter reference
            int tpfn = 0;
            for (int n = 1; n <= 4; ++n) tpfn += rl - n + 1 > 0 ? rl - n + 1 : 0;
            const long total = tpfp > tpfn ? tpfp : tpfn, tp = s_tp[r];
            if (total > 0 && (best_total == 0 || tp * best_total > best_tp * total)) { best_tp = tp; best_total = total; }      // strictly better only
        }
        o[8] = H; o[9] = close; o[10] = (int)best_tp; o[11] = (int)best_total;
    }
}

// sum over the workgroup (4 waves) in a fixed order; every thread gets the result
__device__ __forceinline__ float block_sum(float v, float* s_red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
    __syncthreads();
    return r;
}

constexpr int kEmbedPerThread = kCaptionMaxEmbed / 256;

// mean over `len` tokens of the embedding rows, components tid, tid + 256, ... of this thread
__device__ __forceinline__ void mean_embedding(const int* toks, int len, const float* __restrict__ E, int V, int m, float (&out)[kEmbedPerThread]) {
#pragma unroll
    for (int q = 0; q < kEmbedPerThread; ++q) out[q] = 0.f;
    for (int j = 0; j < len; ++j) {
        const int tok = toks[j];
        const bool ok = tok >= 0 && tok < V;
        const float* row = E + (long)(ok ? tok : 0) * m;
#pragma unroll
        for (int q = 0; q < kEmbedPerThread; ++q) {
            const int d = threadIdx.x + 256 * q;
            if (d < m) out[q] += ok ? row[d] : NAN;
        }
    }
    const float cnt = (float)len;                      // len = 0: 0 / 0 = NaN, as torch's mean of an empty tensor
#pragma unroll
    for (int q = 0; q < kEmbedPerThread; ++q) out[q] = out[q] / cnt;
}

__global__ __launch_bounds__(256) void caption_cosine_kernel(const int* __restrict__ cap_tokens, const int* __restrict__ cap_len, int W,
                                                             const int* __restrict__ refs, const int* __restrict__ ref_len, int R, int T,
                                                             const float* __restrict__ E, int V, int m, float* __restrict__ best) {
    __shared__ int s_hyp[kCaptionMaxLen];
    __shared__ int s_ref[kCaptionMaxRefs * kCaptionMaxLen];
    __shared__ int s_rl[kCaptionMaxRefs];
    __shared__ float s_red[4];
    const int b = blockIdx.x;
    const int H = stage_tokens(cap_tokens, cap_len, W, refs, ref_len, b, R, T, s_hyp, s_ref, s_rl);
    __syncthreads();
    const float eps = 1e-8f;
    float a[kEmbedPerThread], c[kEmbedPerThread];
    mean_embedding(s_hyp, H, E, V, m, a);
    float sq = 0.f;
#pragma unroll
    for (int q = 0; q < kEmbedPerThread; ++q) sq += (int)threadIdx.x + 256 * q < m ? a[q] * a[q] : 0.f;
    const float na = fmaxf(sqrtf(block_sum(sq, s_red)), eps);
    float bestv = -INFINITY;
    for (int r = 0; r < R; ++r) {
        mean_embedding(s_ref + r * T, s_rl[r], E, V, m, c);
        sq = 0.f;
#pragma unroll
        for (int q = 0; q < kEmbedPerThread; ++q) sq += (int)threadIdx.x + 256 * q < m ? c[q] * c[q] : 0.f;
        const float nc = fmaxf(sqrtf(block_sum(sq, s_red)), eps);
        float dot = 0.f;
#pragma unroll
        for (int q = 0; q < kEmbedPerThread; ++q) dot += (int)threadIdx.x + 256 * q < m ? (c[q] / nc) * (a[q] / na) : 0.f;
        const float cs = block_sum(dot, s_red);
        if (cs > bestv || cs != cs) bestv = cs;        // a NaN stays (bestv > NaN is never true again)
    }
    if (threadIdx.x == 0) best[b] = bestv;
}

}  // namespace

int beam_select(const int* tok_in, const int* prev_row, const int* fin_count, const int* fin_step, const int* fin_row, const float* fin_score,
                const float* fin_mean, const float* alpha_hist, int B, int K, int S, int L, int method, float reward, int pad_id, int* cap_tokens,
                int* cap_len, float* cap_score, float* cap_raw, int* cap_step, float* cap_alpha, hipStream_t st) {
    hipLaunchKernelGGL(beam_select_kernel, dim3(B), dim3(256), 0, st, tok_in, prev_row, fin_count, fin_step, fin_row, fin_score, fin_mean, alpha_hist, B, K, S,
                       L, method, reward, pad_id, cap_tokens, cap_len, cap_score, cap_raw, cap_step, cap_alpha);
    return launch_ok("beam_select");
}

int beam_select_at(const int* tok_in, const int* prev_row, const int* fin_count, const int* fin_step, const int* fin_row, const float* fin_score,
                   const float* alpha_hist, const int* pick, const double* pick_score, int B, int K, int S, int L, int pad_id, int* cap_tokens, int* cap_len,
                   float* cap_score, float* cap_raw, int* cap_step, float* cap_alpha, hipStream_t st) {
    hipLaunchKernelGGL(beam_select_at_kernel, dim3(B), dim3(256), 0, st, tok_in, prev_row, fin_count, fin_step, fin_row, fin_score, alpha_hist, pick,
                       pick_score, B, K, S, L, pad_id, cap_tokens, cap_len, cap_score, cap_raw, cap_step, cap_alpha);
    return launch_ok("beam_select_at");
}

int beam_hypotheses(const int* tok_in, const int* prev_row, const int* fin_count, const int* fin_step, const int* fin_row, int B, int K, int S, int pad_id,
                    int* hyp_tokens, int* hyp_len, hipStream_t st) {
    const long n = (long)B * K;
    hipLaunchKernelGGL(beam_hypotheses_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, tok_in, prev_row, fin_count, fin_step, fin_row, B, K, S,
                       pad_id, hyp_tokens, hyp_len);
    return launch_ok("beam_hypotheses");
}

int caption_stats(const int* cap_tokens, const int* cap_len, int W, const int* refs, const int* ref_len, int B, int R, int T, int* stats, hipStream_t st) {
    hipLaunchKernelGGL(caption_stats_kernel, dim3(B), dim3(256), 0, st, cap_tokens, cap_len, W, refs, ref_len, R, T, stats);
    return launch_ok("caption_stats");
}

int caption_cosine(const int* cap_tokens, const int* cap_len, int W, const int* refs, const int* ref_len, int B, int R, int T, const float* embedding,
                   int V, int m, float* best, hipStream_t st) {
    hipLaunchKernelGGL(caption_cosine_kernel, dim3(B), dim3(256), 0, st, cap_tokens, cap_len, W, refs, ref_len, R, T, embedding, V, m, best);
    return launch_ok("caption_cosine");
}

}  // namespace sat
