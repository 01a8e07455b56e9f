// Device kernels of the caption searches: the scores, keys and selections of one search step, the bookkeeping between steps, and the
// initial states of the beams (model.py:255-448).  Included by decoder_search.hip only; the kernels of the decode step itself are
// in decoder_kernels.h and are reached through the launchers of decoder_step.h.
#pragma once
#include "common.h"
#include "row_reduce.h"

namespace sat {

// ------------------------------------------------------------------ small utilities
// clears and constants as kernels: a search enqueues nothing but kernel launches, so that a captured stream (hipGraph) is one linear
// chain of kernel nodes (memset / memcpy nodes were seen to run out of order inside a replayed graph)
__global__ void set4_int_kernel(int* p, int a, int b, int c, int d) { p[0] = a; p[1] = b; p[2] = c; p[3] = d; }
__global__ void fill_int_kernel(int* p, long n, int v) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// ------------------------------------------------------------------ inference (beam search, model.py:329-343, 351-359)
// scores[r, v] = log_softmax(logits[r, :] / T)[v] (+ parent[r]); masked token ids become -inf.  One block per beam row.
// The row's arithmetic (shared by the constrained kernel below, so that a word has the same float in both searches).
// x and o may be the same row (beam_history_scores_kernel normalises its penalised copy in place): every element is read in the
// first pass, and the last pass reads and writes element v from the same thread.
// A -inf logit gives a -inf score and leaves the other scores as they are without it; a row of nothing but -inf gives NaN
// (torch.log_softmax does both).
__device__ __forceinline__ void beam_scores_row(const float* x, int V, float inv_temp, float add, float* o, int tid) {
    __shared__ float s_m[4], s_s[4];
    float mx = -INFINITY, sum = 0.f;
    for (int v = tid; v < V; v += 256) lse_word(x[v] * inv_temp, mx, sum);
    lse_wave_put<true>(mx, sum, s_m, s_s, tid);
    __syncthreads();
    const float lse = lse_block(s_m, s_s);
    for (int v = tid; v < V; v += 256) o[v] = x[v] * inv_temp - lse + add;
    __syncthreads();
}
__global__ __launch_bounds__(256) void beam_scores_kernel(const float* __restrict__ logits, int V, float inv_temp,
                                                          const int* __restrict__ masked, int n_masked,
                                                          const float* __restrict__ parent, float* __restrict__ scores) {
    const int r = blockIdx.x, tid = threadIdx.x;
    float* o = scores + (long)r * V;
    beam_scores_row(logits + (long)r * V, V, inv_temp, parent ? parent[r] : 0.f, o, tid);
    for (int k = tid; k < n_masked; k += 256) { int id = masked[k]; if (id >= 0 && id < V) o[id] = -INFINITY; }
}

// Ensemble decoding ("Ensemble decoding"): combined[r, v] of M members' logits for the same hypothesis row, the logits of
// the model the shared search then runs on at temperature 1.  With l_i = log_softmax(z_i * inv_temp) of member i's row:
//   arithmetic (mixture)         c_v = log sum_i w_i exp(l_i,v), as mx + log sum_i exp(l_i,v + log w_i - mx), mx the largest term's exponent
//   geometric (product of experts) c_v = sum_i w_i l_i,v
// Members with w_i == 0 are skipped in both (their logw is unused).  One block per row: sweep 1 reads every member's value of a word
// and keeps M online (max, sum-exp) pairs, reduced over the wave by shuffles and over the four waves through LDS; sweep 2 reads the
// row again (L2-resident) and writes c.  Finite logits give finite c: every l_i,v is finite, the mixture's sum holds the term 1, and
// the product is a finite sum.  16-byte loads and stores where every member's row and the output row start 16-byte aligned; the
// words past the last whole float4, or every word of an unaligned row, go one by one.  No atomics: same input, same bits.
__global__ __launch_bounds__(256) void beam_ensemble_combine_kernel(EnsembleArgs a, int M, int geometric, int V, float inv_temp, float* __restrict__ combined) {
    __shared__ float s_m[SAT_ENSEMBLE_MAX][4], s_s[SAT_ENSEMBLE_MAX][4];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float* z[SAT_ENSEMBLE_MAX];
    float* o = combined + (long)r * V;
    unsigned long long low = (unsigned long long)o;
#pragma unroll
    for (int i = 0; i < SAT_ENSEMBLE_MAX; ++i) { z[i] = i < M ? a.z[i] + (long)r * V : nullptr; if (i < M) low |= (unsigned long long)z[i]; }
    const int n4 = (low & 15) == 0 ? V >> 2 : 0;       // float4 of the row's body; the rest is the scalar tail
    float mx[SAT_ENSEMBLE_MAX], sum[SAT_ENSEMBLE_MAX];
#pragma unroll
    for (int i = 0; i < SAT_ENSEMBLE_MAX; ++i) { mx[i] = -INFINITY; sum[i] = 0.f; }
    for (int q = tid; q < n4; q += 256) {
#pragma unroll
        for (int i = 0; i < SAT_ENSEMBLE_MAX; ++i) if (i < M) {
            const float4 v = reinterpret_cast<const float4*>(z[i])[q];
            lse_word(v.x * inv_temp, mx[i], sum[i]); lse_word(v.y * inv_temp, mx[i], sum[i]);
            lse_word(v.z * inv_temp, mx[i], sum[i]); lse_word(v.w * inv_temp, mx[i], sum[i]);
        }
    }
    for (int v = 4 * n4 + tid; v < V; v += 256) {
#pragma unroll
        for (int i = 0; i < SAT_ENSEMBLE_MAX; ++i) if (i < M) lse_word(z[i][v] * inv_temp, mx[i], sum[i]);
    }
    float lse[SAT_ENSEMBLE_MAX];
#pragma unroll
    for (int i = 0; i < SAT_ENSEMBLE_MAX; ++i) if (i < M)
        lse_wave_put(mx[i], sum[i], s_m[i], s_s[i], tid);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < SAT_ENSEMBLE_MAX; ++i) lse[i] = i < M ? lse_block(s_m[i], s_s[i]) : 0.f;
    float x[SAT_ENSEMBLE_MAX];
    for (int q = tid; q < n4; q += 256) {
        float4 v[SAT_ENSEMBLE_MAX], c;
#pragma unroll
        for (int i = 0; i < SAT_ENSEMBLE_MAX; ++i) v[i] = i < M ? reinterpret_cast<const float4*>(z[i])[q] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < SAT_ENSEMBLE_MAX; ++i) x[i] = v[i].x;
        c.x = ensemble_word<SAT_ENSEMBLE_MAX>(x, lse, a, M, geometric, inv_temp);
#pragma unroll
        for (int i = 0; i < SAT_ENSEMBLE_MAX; ++i) x[i] = v[i].y;
        c.y = ensemble_word<SAT_ENSEMBLE_MAX>(x, lse, a, M, geometric, inv_temp);
#pragma unroll
        for (int i = 0; i < SAT_ENSEMBLE_MAX; ++i) x[i] = v[i].z;
        c.z = ensemble_word<SAT_ENSEMBLE_MAX>(x, lse, a, M, geometric, inv_temp);
#pragma unroll
        for (int i = 0; i < SAT_ENSEMBLE_MAX; ++i) x[i] = v[i].w;
        c.w = ensemble_word<SAT_ENSEMBLE_MAX>(x, lse, a, M, geometric, inv_temp);
        reinterpret_cast<float4*>(o)[q] = c;
    }
    for (int v = 4 * n4 + tid; v < V; v += 256) {
#pragma unroll
        for (int i = 0; i < SAT_ENSEMBLE_MAX; ++i) x[i] = i < M ? z[i][v] : 0.f;
        o[v] = ensemble_word<SAT_ENSEMBLE_MAX>(x, lse, a, M, geometric, inv_temp);
    }
}

// top-k of a flat array of n >= k floats by a single block of 1024 threads: descending, ties to the lowest index, every index at
// most once.  wk is a scratch copy of x in which a winner is marked as taken with NaN, which the scan skips -- apart from the -inf
// of masked, banned and out-of-nucleus entries, so once fewer than k entries above -inf are left the rest of the result is the
// -inf entries in increasing index order (a stable descending sort).  NaN in x is not supported.
__device__ __forceinline__ void beam_block_topk(const float* __restrict__ x, float* __restrict__ wk, long n, int k, float* __restrict__ values,
                                                int* __restrict__ indices, int tid) {
    for (long i = tid; i < n; i += 1024) wk[i] = x[i];
    __syncthreads();
    block_picks_marking(wk, n, k, [&](int it, float bv, long bi) { values[it] = bv; indices[it] = (int)bi; }, tid);
}
// torch.topk on the flattened beam scores of one image (model.py:359), with the tie rule above.  Single block.
__global__ __launch_bounds__(1024) void topk_kernel(const float* __restrict__ x, float* __restrict__ work, long n, int k,
                                                    float* __restrict__ values, int* __restrict__ indices) {
    beam_block_topk(x, work, n, k, values, indices, threadIdx.x);
}


// ------------------------------------------------------------------ batched beam search (all images of a batch at once)
// Rows are laid out (B, K): image b owns rows b*K .. b*K + K - 1, its klive[b] live hypotheses first.
// InitLSTM over the expanded copies of ONE image's annotation (model.py:265-269), for every beam: an image has G beams of Kg rows
// (G = 1 without groups), and the raw reshape of F3 acts on each beam's own (Kg, 2*layers*n) buffer, so that a group starts exactly
// like a plain search at beamk = Kg.  Beam p = b * G + g reads image b.  h, c: (layers, B*G*Kg, n).
__global__ void init_expand_beams_kernel(const float* __restrict__ init_img, float* __restrict__ h0, float* __restrict__ c0, int B, int G, int Kg, int n,
                                         int layers) {
    const long per = 2L * layers * Kg * n;                     // flat elements of one beam
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= per * B * G) return;
    const int p = (int)(e / per); const long f = e - (long)p * per;
    const long w2 = 2L * layers * n, slab_sz = (long)Kg * n;
    const float v = init_img[(long)(p / G) * w2 + f % w2];     // every one of the Kg rows is the image's init vector
    const long slab = f / slab_sz, within = f - slab * slab_sz;
    const long row = within / n, col = within - row * n;
    const long N = (long)B * G * Kg;
    if (slab < layers) h0[(slab * N + (long)p * Kg + row) * n + col] = v;
    else c0[((slab - layers) * N + (long)p * Kg + row) * n + col] = v;
}
// live[i] = 1 for the first klive[b] rows of image b (the kernels' `lengths[i] > step` predicate with step = 0)
__global__ void beam_live_kernel(const int* __restrict__ klive, int* __restrict__ live, int B, int K) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B * K) live[i] = (i % K) < klive[i / K] ? 1 : 0;
}
// torch.topk of the flattened live scores of every image (model.py:343 at step 0: row 0 only; model.py:359 afterwards):
// beam_block_topk, one block per image; `work` (B, K*V) is scratch.
__global__ __launch_bounds__(1024) void beam_topk_kernel(const float* __restrict__ scores, float* __restrict__ work, const int* __restrict__ klive,
                                                         int K, int V, int first_step, float* __restrict__ values, int* __restrict__ indices) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int k = klive[b];
    if (k <= 0) return;
    const long n = first_step ? V : (long)k * V;
    beam_block_topk(scores + (long)b * K * V, work + (long)b * K * V, n, k, values + b * K, indices + b * K, tid);
}
// ---- sampled continuation of the beams (model.py:360-379) for all images at once.
// torch.multinomial(p, k) without replacement draws an ordered sample from the Plackett-Luce distribution of p; so does
// "top-k of log p + Gumbel noise" (Gumbel-top-k), which needs no sequential renormalisation and reuses the per-image top-k
// kernel.  The draws are therefore not torch's: they come from a counter-based hash of (seed, step, row, candidate), or from a
// caller-supplied table of Gumbel variates (tests).
__device__ __forceinline__ float hash_uniform(unsigned long long seed, unsigned long long stream, unsigned long long idx) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (stream + 1) + idx * 0xD1342543DE82EF95ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return ((float)(z >> 40) + 0.5f) * (1.0f / 16777216.0f);       // 24 bits -> (0, 1)
}
__device__ __forceinline__ float gumbel_of(float u) { return -__logf(-__logf(u)); }
// keys[i, :] for live row i = (b, j):  method 1 ("multinomial", model.py:360-364): log softmax_v(20 * s / step) + G
//                                      method 2 ("topk", model.py:365-379): s / step + G for the row's sample_topk best
//                                      candidates (torch.topk order; the Gumbel variate belongs to the candidate's RANK t), else -inf
// gumbel: optional table (B*K rows, gstride floats per row) of this step: method 1 reads [v], method 2 reads [t].
__global__ __launch_bounds__(256) void beam_sample_keys_kernel(const float* __restrict__ scores, const int* __restrict__ klive, int K, int V, int method,
                                                               int sample_topk, float step, unsigned long long seed, unsigned long long stream,
                                                               const float* __restrict__ gumbel, int gstride, float* __restrict__ keys) {
    const int i = blockIdx.x, b = i / K, j = i - b * K, tid = threadIdx.x;
    if (j >= klive[b]) return;
    const float* s = scores + (long)i * V; float* key = keys + (long)i * V;
    __shared__ float s_v[4];
    if (method == 1) {
        const float sc = 20.0f / step;
        float mx = -INFINITY;
        for (int v = tid; v < V; v += 256) mx = fmaxf(mx, s[v] * sc);
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        if ((tid & 63) == 0) s_v[tid >> 6] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(s_v[0], s_v[1]), fmaxf(s_v[2], s_v[3]));
        __syncthreads();
        float sum = 0.f;
        for (int v = tid; v < V; v += 256) sum += __expf(s[v] * sc - mx);
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if ((tid & 63) == 0) s_v[tid >> 6] = sum;
        __syncthreads();
        const float lse = mx + __logf(s_v[0] + s_v[1] + s_v[2] + s_v[3]);
        for (int v = tid; v < V; v += 256) {
            const float g = gumbel ? gumbel[(long)i * gstride + v] : gumbel_of(hash_uniform(seed, stream, (unsigned long long)i * V + v));
            key[v] = s[v] * sc - lse + g;                 // -inf scores (masked tokens) stay -inf: probability zero
        }
    } else {
        for (int v = tid; v < V; v += 256) key[v] = -INFINITY;
        __syncthreads();
        // the row's best sample_topk candidates, one per pass: descending value, ties to the lowest index; stops once none is left
        block_picks_in_order<4>(V, sample_topk, true, [&](int v, float& x, int& id) { x = s[v]; id = v; }, [&](int t, float bv, int bi) {
            if (bi < V) {
                const float g = gumbel ? gumbel[(long)i * gstride + t] : gumbel_of(hash_uniform(seed, stream, (unsigned long long)i * V + t));
                key[bi] = bv / step + g;
            }
        }, tid);
    }
}
// ---- method 4 ("ancestral", DESIGN.md 5 "Self-critical training"): keys[i, v] = s[v] + G[v] for live row i, every step: the arg-max
// key is one draw from the row's own distribution over its unmasked words (-inf stays -inf).  Table layout and hash indexing of method 1.
__global__ __launch_bounds__(256) void beam_ancestral_keys_kernel(const float* __restrict__ scores, const int* __restrict__ klive, int K, int V,
                                                                  unsigned long long seed, unsigned long long stream, const float* __restrict__ gumbel,
                                                                  float* __restrict__ keys) {
    const int i = blockIdx.x, b = i / K, j = i - b * K;
    if (j >= klive[b]) return;
    const float* s = scores + (long)i * V; float* key = keys + (long)i * V;
    for (int v = threadIdx.x; v < V; v += 256) {
        const float g = gumbel ? gumbel[(long)i * V + v] : gumbel_of(hash_uniform(seed, stream, (unsigned long long)i * V + v));
        key[v] = s[v] + g;
    }
}
// ---- method 3 ("nucleus", DESIGN.md 5 "Sampled decoding"): "topk"'s rule s / step + G on another candidate set, the fewest words of
// the row (score descending, ties to the lower id) whose weights w = exp(s - max) sum to topp * W.  The cut is searched on the
// score itself: the order-preserving unsigned image of the float is bisected bit by bit, every pass one block reduction of
// sum{ w : s >= t }.  Sums of non-negative floats taken in one fixed order are monotone in the set summed, so the bisection is
// well defined in fp32, and a pass that includes every finite entry reproduces W bit for bit.
__device__ __forceinline__ unsigned ordered_bits(float x) {
    const unsigned u = x == 0.f ? 0u : __float_as_uint(x);  // -0 and +0 are one score
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_float(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }
// fixed-order block reductions for 256 threads: xor butterfly inside each wave (every lane ends with the same value), then
// (wave0 + wave1) + (wave2 + wave3).  `slot` holds 4 words; callers alternate between two slots, so one barrier a call is enough.
__device__ __forceinline__ float block_sum_f(float x, float* slot, int tid) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if ((tid & 63) == 0) slot[tid >> 6] = x;
    __syncthreads();
    return (slot[0] + slot[1]) + (slot[2] + slot[3]);
}
__device__ __forceinline__ int block_sum_i(int x, int* slot, int tid) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if ((tid & 63) == 0) slot[tid >> 6] = x;
    __syncthreads();
    return (slot[0] + slot[1]) + (slot[2] + slot[3]);
}
#define NUCLEUS_REGS 32                                     // entries a thread keeps in registers: rows up to 256 * 32 = 8192 words
// keys[i, v] = s[v] / step + G[v] for the words of row i's nucleus, else -inf; nucleus_size[i] (optional) = the member count.
// klive NULL: every row is live (sat_nucleus_keys).  gumbel: optional (rows, V) table of this step, else the hash at (i * V + v).
__global__ __launch_bounds__(256) void beam_nucleus_keys_kernel(const float* __restrict__ scores, const int* __restrict__ klive, int K, int V, float topp,
                                                                float step, unsigned long long seed, unsigned long long stream,
                                                                const float* __restrict__ gumbel, float* __restrict__ keys, int* __restrict__ nucleus_size) {
    const int i = blockIdx.x, tid = threadIdx.x;
    if (klive) { const int b = i / K; if (i - b * K >= klive[b]) return; }
    const float* s = scores + (long)i * V; float* key = keys + (long)i * V;
    __shared__ float s_f[2][4]; __shared__ int s_n[2][4]; __shared__ int s_c[2][4]; __shared__ int s_scan[4];
    const bool cached = V <= 256 * NUCLEUS_REGS;
    const int nk = (V + 255) >> 8;                           // strided passes a thread makes over the row
    // the largest finite score.  Non-finite entries (masked and banned words at -inf) are no candidates.
    float mx = -INFINITY;
    for (int v = tid; v < V; v += 256) { const float x = s[v]; if (x < INFINITY) mx = fmaxf(mx, x); }
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if ((tid & 63) == 0) s_f[1][tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(s_f[1][0], s_f[1][1]), fmaxf(s_f[1][2], s_f[1][3]));
    if (!(mx > -INFINITY)) {                                 // no finite entry: an empty nucleus
        for (int v = tid; v < V; v += 256) key[v] = -INFINITY;
        if (nucleus_size && tid == 0) nucleus_size[i] = 0;
        return;
    }
    // w and the ordered image in registers where the row fits; image 0 marks "not a candidate" (no finite float maps to 0)
    float rw[NUCLEUS_REGS]; unsigned ru[NUCLEUS_REGS];
    auto weight = [&](float x) { return __expf(x - mx); };
    auto finite = [](float x) { return x > -INFINITY && x < INFINITY; };
    if (cached) {
#pragma unroll
        for (int k = 0; k < NUCLEUS_REGS; ++k) {
            const int v = tid + (k << 8);
            rw[k] = 0.f; ru[k] = 0u;
            if (v < V) { const float x = s[v]; if (finite(x)) { rw[k] = weight(x); ru[k] = ordered_bits(x); } }
        }
    }
    // mass_ge(t) = sum{ w[v] : image[v] >= t } over the candidates, t >= 1
    int pass = 0;
    auto mass_ge = [&](unsigned t) {
        float acc = 0.f;
        if (cached) {
#pragma unroll
            for (int k = 0; k < NUCLEUS_REGS; ++k) { if (k < nk && ru[k] >= t) acc += rw[k]; }
        } else {
            for (int v = tid; v < V; v += 256) { const float x = s[v]; if (finite(x) && ordered_bits(x) >= t) acc += weight(x); }
        }
        return block_sum_f(acc, s_f[(pass++) & 1], tid);
    };
    const float W = mass_ge(1u);
    const float target = topp * W;
    unsigned t = 1u;                                         // every candidate: topp >= 1, or a target the sums never reach
    if (topp < 1.f) {
        t = 0u;
        for (int bit = 31; bit >= 0; --bit) {                // the largest t with mass_ge(t) >= target: the image of a score of the row
            const unsigned cand = t | (1u << bit);
            if (mass_ge(cand) >= target) t = cand;
        }
        if (t == 0u) t = 1u;
    }
    // the entries above the threshold are in; of the cnt entries AT it (equal scores, equal weights c) the m lowest ids are
    float above = 0.f; int n_above = 0, cnt = 0;
    if (cached) {
#pragma unroll
        for (int k = 0; k < NUCLEUS_REGS; ++k) {
            if (k < nk) { if (ru[k] > t) { above += rw[k]; ++n_above; } else if (ru[k] == t) ++cnt; }
        }
    } else {
        for (int v = tid; v < V; v += 256) {
            const float x = s[v];
            if (finite(x)) { const unsigned u = ordered_bits(x); if (u > t) { above += weight(x); ++n_above; } else if (u == t) ++cnt; }
        }
    }
    const int p = (pass++) & 1;
    above = block_sum_f(above, s_f[p], tid);
    n_above = block_sum_i(n_above, s_n[p], tid);
    cnt = block_sum_i(cnt, s_c[p], tid);
    int m = cnt;                                             // t == 1 lies below every candidate: all of them are "above", cnt = 0
    if (t > 1u) {
        const float c = weight(ordered_float(t));
        const float need = ceilf((target - above) / c);
        m = need >= (float)cnt ? cnt : (need >= 1.f ? (int)need : 1);
    }
    if (nucleus_size && tid == 0) nucleus_size[i] = n_above + m;
    const bool split = m < cnt;                              // the cut falls inside the run of equal scores
    const float tv = ordered_float(t);
    auto draw = [&](int v) {
        return gumbel ? gumbel[(long)i * V + v] : gumbel_of(hash_uniform(seed, stream, (unsigned long long)i * V + v));
    };
    // strided pass: everything but a split run, whose entries the blocked pass below writes
    for (int v = tid; v < V; v += 256) {
        const float x = s[v];
        const unsigned u = finite(x) ? ordered_bits(x) : 0u;
        if (split && u == t) continue;
        key[v] = (u >= t) ? x / step + draw(v) : -INFINITY;
    }
    if (!split) return;
    // ranks of the tied entries by id: thread tid owns the ids [tid * chunk, tid * chunk + chunk), a block prefix count orders them
    const int chunk = (V + 255) >> 8, lo = tid * chunk, hi = min(V, lo + chunk);
    int mine = 0;
    for (int v = lo; v < hi; ++v) mine += (s[v] == tv) ? 1 : 0;
    int incl = mine;
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(incl, o, 64); if ((tid & 63) >= o) incl += y; }
    if ((tid & 63) == 63) s_scan[tid >> 6] = incl;
    __syncthreads();
    int rank = incl - mine;
    for (int w = 0; w < (tid >> 6); ++w) rank += s_scan[w];
    for (int v = lo; v < hi; ++v) {
        if (s[v] == tv) { key[v] = rank < m ? tv / step + draw(v) : -INFINITY; ++rank; }
    }
}
// after the top-k over the keys: the kept hypotheses carry their SCORES (model.py:382 top_scores = seq_scores.reshape(-1)[pred_idx])
__global__ void beam_take_scores_kernel(const float* __restrict__ scores, const int* __restrict__ inds, const int* __restrict__ klive, int B, int K, int V,
                                        float* __restrict__ values) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * K) return;
    const int b = i / K, j = i - b * K;
    if (j < klive[b]) { const int ind = inds[i]; if (ind >= 0 && ind < K * V) values[i] = scores[(long)b * K * V + ind]; }
}
// ---- constrained search: forced prefix, banned ids, top-g clipping ("Constrained search").
// Image b has a forced prefix of P_b words.  Step s < P_b: every row keeps its parent and takes prefix[b][s].  s == P_b: the
// first free step, the top k of row 0 (model.py:343).  s > P_b: the free search.  P_b = 0 is the unconstrained search.
__device__ __forceinline__ int beam_prefix_len(const int* __restrict__ prefix_len, int b, int max_prefix) {
    if (!prefix_len) return 0;
    const int p = prefix_len[b];
    return p < 0 ? 0 : (p > max_prefix ? max_prefix : p);
}
// beam_scores_kernel with the mask chosen per image (the first-step mask only where step 0 is the image's first free step)
// and the banned ids on top.
__global__ __launch_bounds__(256) void beam_scores_constrained_kernel(const float* __restrict__ logits, int K, int V, float inv_temp,
                                                                      const int* __restrict__ mask_first, const int* __restrict__ mask_rest, int step,
                                                                      const int* __restrict__ prefix_len, int max_prefix,
                                                                      const int* __restrict__ banned, int n_banned,
                                                                      const float* __restrict__ parent, float* __restrict__ scores) {
    const int r = blockIdx.x, tid = threadIdx.x;
    float* o = scores + (long)r * V;
    beam_scores_row(logits + (long)r * V, V, inv_temp, parent ? parent[r] : 0.f, o, tid);
    const bool first = step == 0 && beam_prefix_len(prefix_len, r / K, max_prefix) == 0;
    const int* masked = first ? mask_first : mask_rest; const int n_masked = first ? 4 : 2;
    for (int k = tid; k < n_masked; k += 256) { int id = masked[k]; if (id >= 0 && id < V) o[id] = -INFINITY; }
    for (int k = tid; k < n_banned; k += 256) { int id = banned[k]; if (id >= 0 && id < V) o[id] = -INFINITY; }
}
// top-g clipping, stage 1: the g best entries of every live row in its free steps (value descending, ties to the lower id), as
// (value, flat index j * V + v) in cand_*[(b * K + j) * g + t].  One block per row; no scratch, every pass looks for the best
// entry strictly after the previous pick.
__global__ __launch_bounds__(256) void beam_row_topg_kernel(const float* __restrict__ scores, const int* __restrict__ klive, int K, int V, int g, int step,
                                                            const int* __restrict__ prefix_len, int max_prefix, float* __restrict__ cand_val,
                                                            int* __restrict__ cand_idx) {
    const int i = blockIdx.x, b = i / K, j = i - b * K, tid = threadIdx.x;
    if (j >= klive[b] || step <= beam_prefix_len(prefix_len, b, max_prefix)) return;
    const float* s = scores + (long)i * V;
    block_picks_in_order<4>(V, g, false, [&](int v, float& x, int& id) { x = s[v]; id = v; }, [&](int t, float bv, int bi) {
        cand_val[(long)i * g + t] = bv; cand_idx[(long)i * g + t] = bi < V ? j * V + bi : 0x7fffffff;   // g <= V: the row never runs out
    }, tid);
}
// The selection of one step with the per-image branch; one block per image, writes what beam_topk_kernel writes (values and
// flat indices parent * V + word of the k kept hypotheses).  keys: the sampled search's keys (free steps draw from them) or
// NULL; g > 0: stage 2 of top-g clipping, the top k of the image's k * g candidates (value descending, ties to the lower flat
// index).  A pure function of the scores: no atomics, no dependence on arrival order.
__global__ __launch_bounds__(1024) void beam_select_kernel(const float* __restrict__ scores, const float* __restrict__ keys, const float* __restrict__ cand_val,
                                                           const int* __restrict__ cand_idx, int g, float* __restrict__ work, const int* __restrict__ klive,
                                                           int K, int V, int step, const int* __restrict__ prefix, const int* __restrict__ prefix_len,
                                                           int max_prefix, float* __restrict__ values, int* __restrict__ indices) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int k = klive[b];
    if (k <= 0) return;
    const int P = beam_prefix_len(prefix_len, b, max_prefix);
    if (step < P) {                                        // forced: row j -> (j, prefix[b][step]) with the word's own score
        if (tid < k) {
            int w = prefix[(long)b * max_prefix + step];
            w = w < 0 ? 0 : (w >= V ? V - 1 : w);
            values[b * K + tid] = scores[((long)b * K + tid) * V + w]; indices[b * K + tid] = tid * V + w;
        }
        return;
    }
    if (step == P || g <= 0) {
        const float* src = (step > P && keys) ? keys : scores;
        beam_block_topk(src + (long)b * K * V, work + (long)b * K * V, step == P ? (long)V : (long)k * V, k, values + b * K, indices + b * K, tid);
        return;
    }
    const float* cv = cand_val + (long)b * K * g; const int* ci = cand_idx + (long)b * K * g;
    block_picks_in_order<16>(k * g, k, false, [&](int i, float& x, int& id) { x = cv[i]; id = ci[i]; }, [&](int it, float bv, int bi) {
        values[b * K + it] = bv; indices[b * K + it] = bi < K * V ? bi : 0;
    }, tid);
}
// decoder noise (model.py:322-324): out = N(0, 1) * scale for every layer and live row (0 for dead rows); normals from the table
// or the hash (Box-Muller).  The noise joins h after attention and the gate were taken from the clean state, so it reaches the
// step through the recurrent products only: the caller adds out * W_hh^T to the gate pre-activations.
__global__ void beam_state_noise_kernel(float* __restrict__ out, const int* __restrict__ live, long N, int n, int layers, float scale,
                                        unsigned long long seed, unsigned long long stream, const float* __restrict__ normals) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)layers * N * n) return;
    const long i = (e / n) % N;
    float z = 0.f;
    if (live[i]) {
        if (normals) z = normals[e];
        else {
            const float u1 = hash_uniform(seed, stream, 2ull * e), u2 = hash_uniform(seed, stream, 2ull * e + 1);
            z = sqrtf(-2.0f * __logf(u1)) * __cosf(6.28318530718f * u2);
        }
    }
    out[e] = z * scale;
}
// Beam bookkeeping of one step for every image (model.py:343-447), one thread per image, in the reference's order:
// extend each kept hypothesis (parent row, word), record the completed ones (word == END) in index order, drop them from the
// beam, and at the last step record whatever is left.  Writes the next step's inputs: token, parent row (for the back-trace
// and the state gather), parent score; the finished list keeps (step, parent row, raw score, mean of the beam's scores at
// that moment -- what the BAR rescoring needs).
__global__ void beam_update_kernel(const float* __restrict__ values, const int* __restrict__ indices, int* __restrict__ klive, int B, int K, int V,
                                   int step, int last_step, int end_id, const int* __restrict__ prefix_len, int max_prefix,
                                   int* __restrict__ tok_next, int* __restrict__ prev_next,
                                   float* __restrict__ top_scores, int* __restrict__ gmap, int* __restrict__ fin_count, int* __restrict__ fin_step,
                                   int* __restrict__ fin_row, float* __restrict__ fin_score, float* __restrict__ fin_mean) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int k = klive[b];
    int nk = 0;
    if (k > 0) {
        const bool own = step <= beam_prefix_len(prefix_len, b, max_prefix);     // up to its first free step a row is its own parent
        float mean_all = 0.f;
        for (int j = 0; j < k; ++j) mean_all += values[b * K + j];
        mean_all /= (float)k;
        int fc = fin_count[b];
        // completed hypotheses first, in index order (torch.nonzero(complete))
        for (int j = 0; j < k; ++j) {
            const int ind = indices[b * K + j];
            const int parent = own ? j : ind / V, tok = ind - (ind / V) * V;
            if (tok == end_id) {
                fin_step[b * K + fc] = step; fin_row[b * K + fc] = parent; fin_score[b * K + fc] = values[b * K + j]; fin_mean[b * K + fc] = mean_all; ++fc;
            }
        }
        // the incomplete ones continue, order kept
        float rest = 0.f;
        for (int j = 0; j < k; ++j) {
            const int ind = indices[b * K + j];
            const int parent = own ? j : ind / V, tok = ind - (ind / V) * V;
            if (tok != end_id) {
                tok_next[b * K + nk] = tok; prev_next[b * K + nk] = parent; top_scores[b * K + nk] = values[b * K + j]; gmap[b * K + nk] = parent;
                rest += values[b * K + j]; ++nk;
            }
        }
        if (step >= last_step && nk > 0) {           // model.py:438-447: cut at max_gen_length
            const float mean_rest = rest / (float)nk;
            for (int j = 0; j < nk; ++j) {
                fin_step[b * K + fc] = step; fin_row[b * K + fc] = prev_next[b * K + j]; fin_score[b * K + fc] = top_scores[b * K + j]; fin_mean[b * K + fc] = mean_rest; ++fc;
            }
            nk = 0;
        }
        fin_count[b] = fc;
    }
    klive[b] = nk;
}
// state of the next step's row j' = this step's new state of its parent row (model.py:366: h, c = h[:, keep], c[:, keep])
__global__ void beam_gather_state_kernel(const float* __restrict__ src, float* __restrict__ dst, const int* __restrict__ gmap, const int* __restrict__ klive,
                                         int B, int K, int n, int layers) {
    const long N = (long)B * K;
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)layers * N * n) return;
    const long l = e / (N * n); const long rem = e - l * N * n; const long i = rem / n; const int col = (int)(rem - i * n);
    const int b = (int)(i / K), j = (int)(i - (long)b * K);
    if (j < klive[b]) dst[e] = src[(l * N + (long)b * K + gmap[i]) * n + col];
}

// ---- history rules: repetition penalty, minimum length, no-repeat n-gram ("History rules").
// A live row of step s has said w_1 .. w_s (the words fed at steps 1..s, prefix words included); the search keeps them as a
// materialised (B * K, stride) table, double-buffered, so that the score kernel reads one short row instead of walking prev_row.
#define SAT_BEAM_HIST_MAX SAT_CAPTION_MAX_LEN
// beam_scores_constrained_kernel for rows with a history.  In order: the penalty on the raw logits of the distinct history words
// (x > 0 ? x / theta : x * theta, a copy in the row's own output so that logits stay untouched), beam_scores_row's arithmetic,
// today's masks and banned ids, END below min_length, the words that would complete an n-gram the row already holds.  Rules 3
// and 4 wait for the image's first free step.  hist_len == NULL: every row holds `step` words (the search).  No atomics; every
// id and length read from memory is clamped or skipped before it addresses anything; the same input gives the same bits.
__global__ __launch_bounds__(256) void beam_history_scores_kernel(const float* __restrict__ logits, int K, int V, float inv_temp,
                                                                  const int* __restrict__ mask_first, int n_first, const int* __restrict__ mask_rest,
                                                                  int n_rest, int step, const int* __restrict__ prefix_len, int max_prefix,
                                                                  const int* __restrict__ banned, int n_banned, const float* __restrict__ parent,
                                                                  const int* __restrict__ hist, const int* __restrict__ hist_len, int hist_stride,
                                                                  int ngram, int min_length, float theta, int end_id, float* __restrict__ scores) {
    __shared__ int s_hist[SAT_BEAM_HIST_MAX];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int cap = hist_stride < SAT_BEAM_HIST_MAX ? hist_stride : SAT_BEAM_HIST_MAX;
    int len = hist_len ? hist_len[r] : step;
    len = len < 0 ? 0 : (len > cap ? cap : len);
    if (tid < len) s_hist[tid] = hist[(long)r * hist_stride + tid];
    __syncthreads();
    const float* x = logits + (long)r * V;
    float* o = scores + (long)r * V;
    const float add = parent ? parent[r] : 0.f;
    if (theta != 1.0f && len > 0) {
        for (int v = tid; v < V; v += 256) o[v] = x[v];
        __syncthreads();
        if (tid < len) {                                   // one thread per position; the first occurrence of a word applies the penalty, once
            const int w = s_hist[tid];
            bool first = w >= 0 && w < V;
            for (int q = 0; q < tid && first; ++q) first = s_hist[q] != w;
            if (first) { const float xv = x[w]; o[w] = xv > 0.f ? xv / theta : xv * theta; }
        }
        __syncthreads();
        beam_scores_row(o, V, inv_temp, add, o, tid);
    } else {
        beam_scores_row(x, V, inv_temp, add, o, tid);
    }
    const int P = beam_prefix_len(prefix_len, r / K, max_prefix);
    const bool first_step = step == 0 && P == 0;
    const int* masked = first_step ? mask_first : mask_rest; const int n_masked = first_step ? n_first : n_rest;
    for (int k = tid; k < n_masked; k += 256) { int id = masked[k]; if (id >= 0 && id < V) o[id] = -INFINITY; }
    for (int k = tid; k < n_banned; k += 256) { int id = banned[k]; if (id >= 0 && id < V) o[id] = -INFINITY; }
    if (step < P) return;                                  // a forced word is obeyed even if it repeats or ends too early
    if (tid == 0 && step < min_length && end_id >= 0 && end_id < V) o[end_id] = -INFINITY;
    // thread p: does hist[p : p + n - 1] equal the last n - 1 words?  Then hist[p + n - 1] would repeat that n-gram.
    if (ngram >= 1 && len >= ngram - 1 && tid <= len - ngram) {
        const int u = len - (ngram - 1);
        bool eq = true;
        for (int i = 0; i < ngram - 1 && eq; ++i) eq = s_hist[tid + i] == s_hist[u + i];
        const int w = s_hist[tid + ngram - 1];
        if (eq && w >= 0 && w < V) o[w] = -INFINITY;
    }
}
// next[i, :step] = cur[parent(i), :step]; next[i, step] = the word row i was just given.  After beam_update_kernel of `step`, for
// the rows that stay live; one thread per (row, position).
__global__ void beam_history_advance_kernel(const int* __restrict__ cur, int* __restrict__ next, const int* __restrict__ tok_next,
                                            const int* __restrict__ prev_next, const int* __restrict__ klive, int B, int K, int stride, int step) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (step < 0 || step >= stride || e >= (long)B * K * (step + 1)) return;
    const int i = (int)(e / (step + 1)), p = (int)(e - (long)i * (step + 1));
    const int b = i / K, j = i - b * K;
    if (j >= klive[b]) return;
    if (p == step) { next[(long)i * stride + p] = tok_next[i]; return; }
    int parent = prev_next[i];
    parent = parent < 0 ? 0 : (parent >= K ? K - 1 : parent);
    next[(long)i * stride + p] = cur[((long)b * K + parent) * stride + p];
}

// ---- diverse (group) beam search: Hamming diversity between the groups of a beam ("Diverse beam search").
// The K rows of an image are G groups of Kg = K / G rows, each a beam of its own; everything but this selection and the final merge
// treats (image, group) as an image of Kg rows.
#define SAT_BEAM_GROUP_MAX_K 1024
// (the groups' initial states: init_expand_beams_kernel, above)
// The selection of one step, one block per image, its groups one after the other.  Group g ranks its candidates (row j of the group,
// word v) by pen = s[j, v] - lambda * c[v], c[v] = how many hypotheses the groups before it kept with word v at this step (s_word, at
// most K entries, so c is a count over that short list); two roundings, multiply then subtract, so c == 0 or lambda == 0 leaves s as
// it is.  beam_block_topk's loop (block_picks_marking) on the penalised copy in `work` (descending, ties to the lower flat index, -inf entries last in index
// order); values is the UNPENALISED s at the winner, indices the group-local parent * V + word, both where beam_update_kernel reads
// them with (B * G, Kg).  klive (B, G) is clamped to 0..Kg.  No atomics, no dependence on arrival order.
__global__ __launch_bounds__(1024) void beam_group_select_kernel(const float* __restrict__ scores, float* __restrict__ work, const int* __restrict__ klive,
                                                                 int K, int G, int V, int first_step, float lambda, float* __restrict__ values,
                                                                 int* __restrict__ indices) {
    __shared__ int s_word[SAT_BEAM_GROUP_MAX_K];
    const int b = blockIdx.x, tid = threadIdx.x, Kg = K / G;
    int kept = 0;                                          // the same in every thread: klive is read by all
    for (int g = 0; g < G; ++g) {
        int k = klive[b * G + g];
        k = k < 0 ? 0 : (k > Kg ? Kg : k);
        if (k <= 0) continue;
        const long base = ((long)b * K + (long)g * Kg) * V;
        const float* x = scores + base; float* wk = work + base;
        const long n = first_step ? (long)V : (long)k * V;
        if (kept > 0 && lambda != 0.f) {
            for (long i = tid; i < n; i += 1024) {
                const int v = (int)(i % V);
                int c = 0;
                for (int q = 0; q < kept; ++q) c += s_word[q] == v ? 1 : 0;
                wk[i] = __fsub_rn(x[i], __fmul_rn(lambda, (float)c));
            }
        } else {
            for (long i = tid; i < n; i += 1024) wk[i] = x[i];
        }
        __syncthreads();
        block_picks_marking(wk, n, k, [&](int it, float, long bi) {
            const bool found = bi < n;                     // k <= n: only a group asked for more picks than it has candidates misses
            const int o = b * K + g * Kg + it;
            values[o] = found ? x[bi] : -INFINITY; indices[o] = found ? (int)bi : 0;
            s_word[kept + it] = found ? (int)(bi % V) : -1;
        }, tid);
        kept += k;
    }
}
// After the last step: prev_row of steps 1 .. S + 1 from group-local to image-level rows (row j of an image belongs to group j / Kg),
// and the finished lists of the (image, group) pairs, g_* (B * G, Kg), compacted into the caller's (B, K) arrays: group ascending,
// inside a group the append order; fin_row image-level.  Thread e translates one prev_row entry; threads e < B * G copy one list.
__global__ void beam_group_merge_kernel(int* __restrict__ prev_row, long n_prev, int B, int K, int G, const int* __restrict__ g_count,
                                        const int* __restrict__ g_step, const int* __restrict__ g_row, const float* __restrict__ g_score,
                                        const float* __restrict__ g_mean, int* __restrict__ fin_count, int* __restrict__ fin_step,
                                        int* __restrict__ fin_row, float* __restrict__ fin_score, float* __restrict__ fin_mean) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int Kg = K / G;
    if (e < n_prev) {
        const int j = (int)(e % K);
        int p = prev_row[e];
        p = p < 0 ? 0 : (p >= Kg ? Kg - 1 : p);
        prev_row[e] = (j / Kg) * Kg + p;
    }
    if (e < (long)B * G) {
        const int b = (int)(e / G), g = (int)(e - (long)b * G);
        int off = 0;
        for (int q = 0; q < g; ++q) { int c = g_count[b * G + q]; off += c < 0 ? 0 : (c > Kg ? Kg : c); }
        int cnt = g_count[b * G + g];
        cnt = cnt < 0 ? 0 : (cnt > Kg ? Kg : cnt);
        for (int f = 0; f < cnt; ++f) {
            const long s = (long)e * Kg + f, d = (long)b * K + off + f;
            int r = g_row[s];
            r = r < 0 ? 0 : (r >= Kg ? Kg - 1 : r);
            fin_step[d] = g_step[s]; fin_row[d] = g * Kg + r; fin_score[d] = g_score[s]; fin_mean[d] = g_mean[s];
        }
        if (g == G - 1) fin_count[b] = off + cnt;
    }
}

// ---- required words: a caption must contain the words of its image ("Required words"; Anderson et al. 2017, Post & Vilar
// 2018).  Everything but this selection and the kernel after the loop is the search with the history tables on.
#define SAT_BEAM_REQUIRED_CAND (SAT_BEAM_REQUIRED_MAX_K * (SAT_BEAM_REQUIRED_MAX + 2))
// image b's required words that can be said at all (ids inside [0, V)), in their order, in s_q; thread 0, the caller syncs.  Returns nothing:
// *s_nq is their number.
__device__ __forceinline__ void beam_required_words(const int* __restrict__ words, const int* __restrict__ n_words, int C, int b, int V, int* s_q, int* s_nq) {
    int nq = 0;
    if (C > 0) {
        int cb = n_words[b];
        cb = cb < 0 ? 0 : (cb > C ? C : cb);
        cb = cb > SAT_BEAM_REQUIRED_MAX ? SAT_BEAM_REQUIRED_MAX : cb;
        for (int c = 0; c < cb; ++c) { const int w = words[(long)b * C + c]; if (w >= 0 && w < V) s_q[nq++] = w; }
    }
    *s_nq = nq;
}
// The selection of one step, one block per image (include/sat_hip.h, sat_beam_search_required).  met(j): which of the image's words row j
// has said, a scan of its history slice.  END is held back (-inf in the working copy) in the rows that miss a word.  The candidates are
// the union by flat index of A, the k picks of beam_block_topk over that copy, R, every row's unmet words, and M, every row's best word;
// a wave per row finds M while it writes the working copy, so the only other pass over k * V floats is the block top-k.  The candidates
// sit in LDS at fixed slots (A: t; R: k + j * C_b + c; M: k + rows * C_b + j), a slot that holds nothing (a -inf score, or a candidate an
// earlier slot already holds: A marks its picks with NaN in the working copy) has no bank.  bank = how many words the extended
// hypothesis has met; at the last step (first_step & 2) the picked word is dropped from the caption (<END>, or the cut), so the bank is
// |met(j)| and a complete row keeps slot 0.  first_step & 1: row 0 alone.  Then k picks round robin from the fullest bank: a block arg-max over the slots of the chosen bank, value
// descending, ties to the lower flat index; nothing left: -inf / index 0.  values is the score at the pick, unchanged.  An image
// without words takes beam_block_topk's picks.  No atomics; counts and ids read from memory are clamped or skipped.
__global__ __launch_bounds__(1024) void beam_required_select_kernel(const float* __restrict__ scores, float* __restrict__ work, const int* __restrict__ klive,
                                                                    const int* __restrict__ hist, int hist_stride, int hist_len,
                                                                    const int* __restrict__ words, const int* __restrict__ n_words, int C, int K, int V,
                                                                    int first_step, int end_id, float* __restrict__ values, int* __restrict__ indices) {
    __shared__ float s_val[SAT_BEAM_REQUIRED_CAND]; __shared__ int s_idx[SAT_BEAM_REQUIRED_CAND]; __shared__ unsigned char s_bank[SAT_BEAM_REQUIRED_CAND];
    __shared__ int s_q[SAT_BEAM_REQUIRED_MAX]; __shared__ int s_nq;
    __shared__ unsigned s_met[SAT_BEAM_REQUIRED_MAX_K]; __shared__ float s_mv[SAT_BEAM_REQUIRED_MAX_K]; __shared__ int s_mi[SAT_BEAM_REQUIRED_MAX_K];
    __shared__ int s_cnt[SAT_BEAM_REQUIRED_MAX + 1]; __shared__ int s_p;
    __shared__ float s_bv[16]; __shared__ long s_bi[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    int k = klive[b];
    k = k < 0 ? 0 : (k > K ? K : k);
    if (k <= 0) return;
    const float* x = scores + (long)b * K * V; float* wk = work + (long)b * K * V;
    if (tid == 0) beam_required_words(words, n_words, C, b, V, s_q, &s_nq);
    __syncthreads();
    const int nq = s_nq, rows = (first_step & 1) ? 1 : k;
    const bool last = (first_step & 2) != 0;              // the word picked now is not part of the caption: the banks count met(j) alone
    const long n = (long)rows * V;
    if (nq == 0) {                                         // nothing required of this image: today's picks
        beam_block_topk(x, wk, n, k, values + b * K, indices + b * K, tid);
        return;
    }
    const unsigned full = (1u << nq) - 1u;
    if (tid < rows) {
        const int len = hist_len < 0 ? 0 : (hist_len > hist_stride ? hist_stride : hist_len);
        const int* hrow = hist + ((long)b * K + tid) * hist_stride;
        unsigned m = 0;
        for (int p = 0; p < len; ++p) { const int w = hrow[p]; for (int c = 0; c < nq; ++c) m |= (w == s_q[c]) ? (1u << c) : 0u; }
        s_met[tid] = m;
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int j = wave; j < rows; j += 16) {                // the working copy with END held back, and M on the way
        const bool hold = s_met[j] != full;
        float bv = -INFINITY; int bi = 0x7fffffff;
        for (int v = lane; v < V; v += 64) {
            float s = x[(long)j * V + v];
            if (hold && v == end_id) s = -INFINITY;
            wk[(long)j * V + v] = s;
            if (s == s && arg_before(s, v, bv, bi)) { bv = s; bi = v; }
        }
        wave_argbest(bv, bi);
        if (lane == 0) { s_mv[j] = bv; s_mi[j] = bi; }
    }
    __syncthreads();
    block_picks_marking(wk, n, k, [&](int it, float bv, long bi) { s_val[it] = bv; s_idx[it] = (bi < n && bv > -INFINITY) ? (int)bi : -1; }, tid);   // A
    const int nR = rows * nq, nC = k + nR + rows;
    for (int i = tid; i < nC; i += 1024) {
        int flat = -1; float val = -INFINITY;
        if (i < k) { flat = s_idx[i]; val = s_val[i]; }
        else if (i < k + nR) {                             // R: (row j, its unmet word c), the first of equal words only
            const int e = i - k, j = e / nq, c = e - j * nq, q = s_q[c];
            bool take = ((s_met[j] >> c) & 1u) == 0u;
            for (int c2 = 0; c2 < c; ++c2) take = take && s_q[c2] != q;
            if (take) { const float s = wk[(long)j * V + q]; if (s == s && s > -INFINITY) { flat = j * V + q; val = s; } }
        } else {                                           // M: (row j, its best word) unless A or R holds it
            const int j = i - k - nR, v = s_mi[j];
            const float s = s_mv[j];
            if (s > -INFINITY && v < V) {
                const float m = wk[(long)j * V + v];
                bool take = m == m;
                for (int c = 0; c < nq; ++c) take = take && !(s_q[c] == v && ((s_met[j] >> c) & 1u) == 0u);
                if (take) { flat = j * V + v; val = s; }
            }
        }
        int bank = 0xff;
        if (flat >= 0) {
            const int j = flat / V, v = flat - j * V;
            unsigned m = s_met[j];
            if (!last) for (int c = 0; c < nq; ++c) m |= (s_q[c] == v) ? (1u << c) : 0u;
            bank = __popc(m);
        }
        s_idx[i] = flat; s_val[i] = val; s_bank[i] = (unsigned char)bank;
    }
    __syncthreads();
    if (wave <= nq) {                                      // wave w counts bank w
        int c = 0;
        for (int i = lane; i < nC; i += 64) c += s_bank[i] == wave ? 1 : 0;
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) s_cnt[wave] = c;
    }
    if (tid == 0) s_p = nq;
    __syncthreads();
    for (int t = 0; t < k; ++t) {
        const int p = s_p;
        int beta = -1;
        for (int u = 0; u <= nq && beta < 0; ++u) { const int bk = p - u < 0 ? p - u + nq + 1 : p - u; if (s_cnt[bk] > 0) beta = bk; }
        float bv = -INFINITY; long bi = 0x7fffffffffffffffL;
        if (beta >= 0)
            for (int i = tid; i < nC; i += 1024)
                if (s_bank[i] == beta) { const long key = (long)s_idx[i] * 4096 + i; if (arg_before(s_val[i], key, bv, bi)) { bv = s_val[i]; bi = key; } }
        block_argbest<16>(bv, bi, s_bv, s_bi, tid);
        if (tid == 0) {
            const bool found = beta >= 0 && bi != 0x7fffffffffffffffL;
            values[b * K + t] = found ? bv : -INFINITY; indices[b * K + t] = found ? (int)(bi >> 12) : 0;
            if (found) { s_bank[(int)(bi & 4095)] = 0xff; s_cnt[beta] -= 1; s_p = beta == 0 ? nq : beta - 1; }
        }
        __syncthreads();
    }
}
// After the last step, one block per image, thread f its f-th finished hypothesis: the back-trace of beam_hypotheses_kernel counts the
// required words the hypothesis contains; req_met[b] is the largest count, and the fin_* lists are compacted in place to the hypotheses
// that reach it, order kept (every thread reads its entry before the barrier and writes it after).  K <= 256 = the block.
__global__ __launch_bounds__(256) void beam_required_finish_kernel(const int* __restrict__ tok_in, const int* __restrict__ prev_row, int* __restrict__ fin_count,
                                                                   int* __restrict__ fin_step, int* __restrict__ fin_row, float* __restrict__ fin_score,
                                                                   float* __restrict__ fin_mean, const int* __restrict__ words, const int* __restrict__ n_words,
                                                                   int C, int B, int K, int S, int V, int* __restrict__ req_met) {
    __shared__ int s_q[SAT_BEAM_REQUIRED_MAX]; __shared__ int s_nq; __shared__ int s_c[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) beam_required_words(words, n_words, C, b, V, s_q, &s_nq);
    __syncthreads();
    const int nq = s_nq;
    int fc = fin_count[b];
    fc = fc < 0 ? 0 : (fc > K ? K : fc);
    fc = fc > 256 ? 256 : fc;
    int cnt = -1, st = 0, row = 0; float sc = 0.f, mn = 0.f;
    if (tid < fc) {
        const long idx = (long)b * K + tid;
        st = fin_step[idx]; row = fin_row[idx]; sc = fin_score[idx]; mn = fin_mean[idx];
        const int step = st < 0 ? 0 : (st > S ? S : st);
        int cur = row < 0 ? 0 : (row >= K ? K - 1 : row);
        unsigned m = 0;
        for (int s = step; s >= 1; --s) {
            const long at = ((long)s * B + b) * K + cur;
            const int w = tok_in[at];
            for (int c = 0; c < nq; ++c) m |= (w == s_q[c]) ? (1u << c) : 0u;
            cur = prev_row[at];
            cur = cur < 0 ? 0 : (cur >= K ? K - 1 : cur);
        }
        cnt = __popc(m);
    }
    s_c[tid] = cnt;
    __syncthreads();
    int best = 0, dst = 0, total = 0;
    for (int f = 0; f < fc; ++f) best = s_c[f] > best ? s_c[f] : best;
    for (int f = 0; f < fc; ++f) { const int keep = s_c[f] == best ? 1 : 0; total += keep; dst += f < tid ? keep : 0; }
    if (tid < fc && cnt == best) {
        const long o = (long)b * K + dst;
        fin_step[o] = st; fin_row[o] = row; fin_score[o] = sc; fin_mean[o] = mn;
    }
    if (tid == 0) { req_met[b] = best; if (fc > 0) fin_count[b] = total; }
}

}  // namespace sat
