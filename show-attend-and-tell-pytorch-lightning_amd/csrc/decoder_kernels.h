// Device kernels of the SAT attention-LSTM decoder (forward and backward).
// Reference semantics: model.py:76-81 (InitLSTM), 94-109 (SoftAttention),
// 125-131 (DeepOutput), 187-192 (beta), 510-548 (train_batch loop).
// The two losses (util.py:105-112, model.py:594) are in ce_loss.hip.
//
// Layout (all fp32, row-major):
//   ann    (B, L, D)   annotations, one row per location -- NHWC encoder output viewed flat.
//                      The R captions of an image share it (repeat_interleave is never materialised:
//                      caption row i belongs to image i / R).
//   U      (B, L, A)   att_enc = ann * W_e^T, hoisted out of the time loop.
//   HC[t]  (N, A+D+4n) per step: [ q = h W_d^T | beta = sigmoid(h W_b^T + b) | LSTM gates ]
//   time-major padded buffers (T1, N, .) for everything saved for backward.
#pragma once
#include "common.h"
#include "row_reduce.h"

namespace sat {

constexpr int ATT_RMAX = 8;      // caption rows of one image handled per pass
constexpr int ATT_THREADS = 256;

// ------------------------------------------------------------------ small utilities
__global__ void fill_kernel(float* p, long n, float v) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// fp32 -> bf16 copy, 4 elements per thread (n4 = elements / 4)
__global__ void cast_bf16_kernel(const float* __restrict__ src, __bf16* __restrict__ dst, long n4) {
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n4) return;
    const float4 v = reinterpret_cast<const float4*>(src)[e];
    typedef __bf16 b4 __attribute__((ext_vector_type(4)));
    b4 o; o[0] = (__bf16)v.x; o[1] = (__bf16)v.y; o[2] = (__bf16)v.z; o[3] = (__bf16)v.w;
    reinterpret_cast<b4*>(dst)[e] = o;
}

// rows x cols fp32 block with row stride ld -> compact bf16 (cols % 4 == 0)
__global__ void cast_block_bf16_kernel(const float* __restrict__ src, long ld, __bf16* __restrict__ dst, int rows, int cols) {
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c4 = cols / 4;
    if (e >= (long)rows * c4) return;
    const long r = e / c4; const int c = (int)(e - r * c4) * 4;
    const float4 v = *reinterpret_cast<const float4*>(src + r * ld + c);
    typedef __bf16 b4 __attribute__((ext_vector_type(4)));
    b4 o; o[0] = (__bf16)v.x; o[1] = (__bf16)v.y; o[2] = (__bf16)v.z; o[3] = (__bf16)v.w;
    *reinterpret_cast<b4*>(dst + r * cols + c) = o;
}

// ---- dropout (nn.Dropout in training mode: model.py:74/78, 117/130, 164/526).  The mask is a counter-based hash of
// (seed, stream, element index): no state, recomputed wherever it is needed (forward, backward), reproducible.
// streams: 0 = InitLSTM mean, 1 = embedding, 2 = DeepOutput, 3 = weight-drop on the hidden-to-hidden matrices.  keep-probability 1-p,
// kept values scaled by 1/(1-p).
__device__ __forceinline__ float dropout_scale(unsigned long long seed, unsigned stream, unsigned long long idx, float p) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(stream + 1) + idx * 0xD1342543DE82EF95ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const float u = (float)(z >> 40) * (1.0f / 16777216.0f);      // 24 bits -> [0,1)
    return (u >= p) ? 1.0f / (1.0f - p) : 0.f;
}

// Which row of a mask a buffer row reads.  Per-step dropout: its own, row0 + r.  Variational (locked) dropout keeps one mask row per
// caption for all of its time steps: `period` = N > 0 folds a time-major row t * N + i onto i, and `row_map` (the packing plan's src_row,
// t * N + i of every packed row) takes a packed row there first.
__device__ __forceinline__ long mask_row(long r, const int* __restrict__ row_map, int period) {
    if (row_map) r = row_map[r];
    return period > 0 ? r % period : r;
}
// dst[r, :] = table[tok[r], :] (embedding gather; tok outside [0, V) -> zeros, the ids the gradient skips), with embedding_dropout when p > 0
__global__ void gather_rows_kernel(const float* __restrict__ table, const int* __restrict__ tok, float* __restrict__ out, int rows, int width, int V,
                                   float p, unsigned long long seed, long row0, int period) {
    int r = blockIdx.x;
    if (r >= rows) return;
    int t = tok[r];
    const long mr = mask_row(row0 + r, nullptr, period);
    for (int c = threadIdx.x; c < width; c += blockDim.x) {
        float v = (t >= 0 && t < V) ? table[(long)t * width + c] : 0.f;
        if (p > 0.f) v *= dropout_scale(seed, 1, (unsigned long long)mr * width + c, p);
        out[(long)r * width + c] = v;
    }
}
// y[r, c] = x[r, c] * mask(stream, mask_row(row0 + r) * width + c)   (in place allowed)
__global__ void dropout_rows_kernel(const float* __restrict__ x, float* __restrict__ y, long total, int width, float p,
                                    unsigned long long seed, unsigned stream, long row0, const int* __restrict__ row_map, int period) {
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    unsigned long long idx = (unsigned long long)row0 * width + e;
    if (row_map || period > 0) {
        const long r = e / width;
        idx = (unsigned long long)mask_row(row0 + r, row_map, period) * width + (e - r * width);
    }
    y[e] = x[e] * dropout_scale(seed, stream, idx, p);
}
// InitLSTM with dropout: the mean of the REPEATED annotations is dropped per caption row (model.py:78 after 487)
__global__ void init_mean_rows_kernel(const float* __restrict__ mean, float* __restrict__ out, int N, int R, int D, float p, unsigned long long seed) {
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)N * D) return;
    long i = e / D; int d = (int)(e - i * D);
    out[e] = mean[(i / R) * D + d] * dropout_scale(seed, 0, (unsigned long long)e, p);
}
// dmean[b, d] = sum_r dmean_rows[b*R + r, d] * mask
__global__ void init_mean_rows_bwd_kernel(const float* __restrict__ drows, float* __restrict__ dmean, int B, int R, int D, float p, unsigned long long seed) {
    long o = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= (long)B * D) return;
    long b = o / D; int d = (int)(o - b * D);
    float s = 0.f;
    for (int r = 0; r < R; ++r) { long e = (b * R + r) * D + d; s += drows[e] * dropout_scale(seed, 0, (unsigned long long)e, p); }
    dmean[o] = s;
}

// Packed per-step parameters in one launch: Wcat = [W_d ; W_beta ; W_hh] (A + D + 4n rows of n), its bf16 copy when the per-step GEMMs read
// bf16 operands, and bcat = [0 ; b_beta ; b_ih + b_hh].  wd_p > 0: weight-drop, the W_hh rows (and only they) are written as W_hh * s with
// s = dropout_scale(seed, 3, index inside W_hh = layer 0 of the (layers, 4n, n) mask, wd_p).
__global__ void pack_wcat_kernel(const float* __restrict__ att_dec, const float* __restrict__ beta_w, const float* __restrict__ w_hh,
                                 const float* __restrict__ beta_b, const float* __restrict__ b_ih, const float* __restrict__ b_hh, float* __restrict__ Wcat,
                                 __bf16* __restrict__ Wcat_b, float* __restrict__ bcat, int A, int D, int n, float wd_p, unsigned long long seed) {
    const long HCW = (long)A + D + 4L * n, nw = HCW * n, e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nw) {
        const long r = e / n;
        float v;
        if (r < A) v = att_dec[e];
        else if (r < A + D) v = beta_w[e - (long)A * n];
        else {
            const long k = e - (long)(A + D) * n;
            v = w_hh[k];
            if (wd_p > 0.f) v *= dropout_scale(seed, 3, (unsigned long long)k, wd_p);
        }
        Wcat[e] = v;
        if (Wcat_b) Wcat_b[e] = (__bf16)v;
    } else if (e < nw + HCW) {
        const long r = e - nw;
        bcat[r] = r < A ? 0.f : (r < A + D ? beta_b[r - A] : b_ih[r - A - D] + b_hh[r - A - D]);
    }
}

// Weight-drop (DropConnect on the hidden-to-hidden matrices) outside the pack: dst[l] = src[l] * s[layer0 + l] for `layers` matrices of
// `per` elements each, s[L][k] = dropout_scale(seed, 3, L * per + k, p).  dst[l] may be src[l] (the weight gradients are masked in
// place); dstb[l], when given, gets the bf16 copy of the same product.
struct WeightDropLayers {
    const float* src[SAT_MAX_LSTM_LAYERS]; float* dst[SAT_MAX_LSTM_LAYERS]; __bf16* dstb[SAT_MAX_LSTM_LAYERS];
};
__global__ void weight_drop_kernel(WeightDropLayers w, int layers, long per, int layer0, float p, unsigned long long seed) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= layers * per) return;
    const int l = (int)(e / per); const long k = e - l * per;
    const float* src = w.src[0]; float* dst = w.dst[0]; __bf16* dstb = w.dstb[0];
#pragma unroll
    for (int j = 1; j < SAT_MAX_LSTM_LAYERS; ++j)
        if (l == j) { src = w.src[j]; dst = w.dst[j]; dstb = w.dstb[j]; }
    const float v = src[k] * dropout_scale(seed, 3, (unsigned long long)(layer0 + l) * per + k, p);
    dst[k] = v;
    if (dstb) dstb[k] = (__bf16)v;
}

// token ids of step `step` for every caption row (teacher forcing): tok[i] = caps[i*T + step]
// (grid.y > 1: steps step .. step + grid.y - 1 in one launch, tok advancing by N per step)
__global__ void teacher_tokens_kernel(const int* __restrict__ caps, const int* __restrict__ lengths, int* __restrict__ tok, int N, int T, int step) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    step += blockIdx.y; tok += (long)blockIdx.y * N;
    if (i < N) tok[i] = (lengths[i] > step) ? caps[(long)i * T + step] : -1;     // finished captions feed nothing
}

// argmax feedback (model.py:523): tok[i] = argmax_v logits_packed[prow_prev[i], v] (first maximum), -1 for dead rows
__global__ void argmax_tokens_kernel(const float* __restrict__ logits, const int* __restrict__ prow_prev, const int* __restrict__ lengths,
                                     int* __restrict__ tok, int V, int step) {
    int i = blockIdx.x;
    __shared__ float sv[4];
    __shared__ int si[4];
    if (lengths[i] <= step) { if (threadIdx.x == 0) tok[i] = -1; return; }
    const float* row = logits + (long)prow_prev[i] * V;
    float best = -INFINITY; int bi = 0x7fffffff;
    for (int v = threadIdx.x; v < V; v += blockDim.x) {
        float x = row[v];
        if (x > best || (x == best && v < bi)) { best = x; bi = v; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        float ob = __shfl_xor(best, o, 64); int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sv[w] = best; si[w] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < (int)(blockDim.x >> 6); ++k)
            if (sv[k] > best || (sv[k] == best && si[k] < bi)) { best = sv[k]; bi = si[k]; }
        tok[i] = bi;
    }
}

// the same decision and the embedding row of the chosen token in ONE launch (scheduled sampling without max-norm renormalisation: model.py:521-526):
// token of caption i at `step` = first maximum of its previous logits row, y[i, :] = embedding[token] (zeros for finished captions)
__global__ __launch_bounds__(256) void argmax_gather_kernel(const float* __restrict__ logits, const int* __restrict__ prow_prev, const int* __restrict__ lengths,
                                                            int* __restrict__ tok, int V, int step, const float* __restrict__ table, float* __restrict__ out, int width,
                                                            float p, unsigned long long seed, long row0, int period) {
    const int i = blockIdx.x;
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ int s_tok;
    const bool live = lengths[i] > step;          // uniform over the block
    int bi = 0x7fffffff;
    if (live) {
        const float* row = logits + (long)prow_prev[i] * V;
        float best = -INFINITY;
        for (int v = threadIdx.x; v < V; v += 256) {
            const float x = row[v];
            if (x > best || (x == best && v < bi)) { best = x; bi = v; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        const int w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) { sv[w] = best; si[w] = bi; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 1; k < 4; ++k)
                if (sv[k] > best || (sv[k] == best && si[k] < bi)) { best = sv[k]; bi = si[k]; }
            s_tok = bi; tok[i] = bi;
        }
        __syncthreads();
    } else if (threadIdx.x == 0) tok[i] = -1;
    const int t = live ? s_tok : -1;
    for (int c = threadIdx.x; c < width; c += 256) {
        float v = (t >= 0 && t < V) ? table[(long)t * width + c] : 0.f;          // a row without a maximum (all NaN) leaves t = INT_MAX
        if (p > 0.f) v *= dropout_scale(seed, 1, (unsigned long long)mask_row(row0 + i, nullptr, period) * width + c, p);
        out[(long)i * width + c] = v;
    }
}

// mean over L of the annotations: mean[b, d]  (model.py:78)
__global__ void ann_mean_kernel(const float* __restrict__ ann, float* __restrict__ mean, int L, int D) {
    int b = blockIdx.x;
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        float s = 0.f;
        for (int l = 0; l < L; ++l) s += ann[((long)b * L + l) * D + d];
        mean[(long)b * D + d] = s / (float)L;
    }
}

// InitLSTM raw reshape (model.py:79-80): the (N, 2*layers*n) buffer whose row j is init[j / R]
// is reinterpreted as (2*layers, N, n): slabs [0, layers) are h0, the rest c0.  flat element e -> row e / (2*layers*n).
// Layer slab l of h0 / c0 is written at h0 + l * lstride (the time-major state buffers keep one run per layer).
__global__ void init_expand_kernel(const float* __restrict__ init_img, float* __restrict__ h0, float* __restrict__ c0, int N, int R, int n,
                                   int layers, long lstride) {
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long slab_sz = (long)N * n, w2 = 2L * layers * n;
    if (e >= 2 * layers * slab_sz) return;
    long row = e / w2, col = e % w2;
    float v = init_img[(row / R) * w2 + col];
    long slab = e / slab_sz, within = e - slab * slab_sz;
    if (slab < layers) h0[slab * lstride + within] = v; else c0[(slab - layers) * lstride + within] = v;
}
// backward of the above: dinit_img[b, col] = sum_r dflat[(b*R + r), col]
__global__ void init_expand_bwd_kernel(const float* __restrict__ dh0, const float* __restrict__ dc0, float* __restrict__ dinit_img, int B, int R, int n) {
    long o = (long)blockIdx.x * blockDim.x + threadIdx.x;
    int N = B * R; long half = (long)N * n;
    if (o >= (long)B * 2 * n) return;
    long b = o / (2 * n), col = o % (2 * n);
    float s = 0.f;
    for (int r = 0; r < R; ++r) {
        long e = (b * R + r) * (2 * n) + col;
        s += (e < half) ? dh0[e] : dc0[e - half];
    }
    dinit_img[o] = s;
}

// ------------------------------------------------------------------ attention forward (one decode step)
// grid = (B, D-chunks); block = 256.  Every block recomputes the (cheap) scores + softmax of its image's
// R caption rows, then accumulates its D-chunk of the context while reading the annotation tile ONCE
// for all R rows.  dyn LDS: [RMAX*L scores/alpha][RMAX*A q][A w][part: 4*RMAX*chunk]
constexpr int ATTF_WAVES = 16;                 // forward: 16 waves share the tanh-heavy score phase of one image
constexpr int ATTF_THREADS = ATTF_WAVES * 64;
// RN = caption rows handled per pass (compile-time: the row loops unroll without per-row guards -- a guard per FMA serialises
// every FMA behind its operand read; dead rows run on zeros instead and are masked at the stores).
template <int VW, int RN>
__global__ __launch_bounds__(ATTF_THREADS) void attention_fwd_kernel(
    const float* __restrict__ ann, const float* __restrict__ U, const float* __restrict__ hc, int hc_ld,
    const float* __restrict__ wf, const int* __restrict__ lengths, int step,
    float* __restrict__ alphas, int T1, float* __restrict__ Z, float* __restrict__ XZ,
    int R, int L, int D, int A, int dchunk) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* s_sc = sm;                        // [RMAX][L]
    float* s_q = s_sc + ATT_RMAX * L;        // [RMAX][A]
    float* s_w = s_q + ATT_RMAX * A;         // [A]
    float* s_part = s_w + A;                 // [4 groups][RMAX][dchunk]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d0 = blockIdx.y * dchunk, dn = min(dchunk, D - d0);
    const float scale = 1.0f / sqrtf((float)L);
    for (int k = tid; k < A; k += ATTF_THREADS) s_w[k] = wf[k];

    for (int r0 = 0; r0 < R; r0 += RN) {
        const int rn = min(RN, R - r0);
        const int i0 = b * R + r0;
        unsigned lmask = 0;
        for (int r = 0; r < rn; ++r) if (lengths[i0 + r] > step) lmask |= 1u << r;
        const bool any = lmask != 0;
        __syncthreads();
        if (any) {
            for (int e = tid; e < RN * A; e += ATTF_THREADS) { int r = e / A, k = e - r * A; s_q[r * A + k] = (r < rn) ? hc[(long)(i0 + r) * hc_ld + k] : 0.f; }
            __syncthreads();
            // ---- scores: wave per location, lanes over the attention dim
            for (int l = wave; l < L; l += ATTF_WAVES) {
                float part[RN];
#pragma unroll
                for (int r = 0; r < RN; ++r) part[r] = 0.f;
                const float* u = U + ((long)b * L + l) * A;
                for (int k = lane; k < A; k += 64) {
                    float uv = u[k], w = s_w[k];
#pragma unroll
                    for (int r = 0; r < RN; ++r) part[r] = fmaf(w, fast_tanh(uv + s_q[r * A + k]), part[r]);
                }
#pragma unroll
                for (int r = 0; r < RN; ++r) { float s = wave_sum(part[r]); if (lane == 0) s_sc[r * L + l] = s * scale; }
            }
            __syncthreads();
            // ---- softmax over L: wave per row
            for (int r = wave; r < rn; r += ATTF_WAVES) {
                if (!((lmask >> r) & 1u)) continue;       // wave-uniform
                float mx = -INFINITY;
                for (int l = lane; l < L; l += 64) mx = fmaxf(mx, s_sc[r * L + l]);
                mx = wave_max(mx);
                float sum = 0.f;
                for (int l = lane; l < L; l += 64) { float e = __expf(s_sc[r * L + l] - mx); s_sc[r * L + l] = e; sum += e; }
                sum = wave_sum(sum);
                float inv = 1.0f / sum;
                for (int l = lane; l < L; l += 64) s_sc[r * L + l] *= inv;
            }
            __syncthreads();
            // dead rows (finished captions, rows past R) take zero attention weights: the context loop below runs unguarded
            for (int e = tid; e < RN * L; e += ATTF_THREADS) { int r = e / L; if (!((lmask >> r) & 1u)) s_sc[e] = 0.f; }
            __syncthreads();
        }
        // ---- alphas out (only the first D-chunk block writes); dead rows are written as zeros
        if (blockIdx.y == 0) {
            for (int e = tid; e < rn * L; e += ATTF_THREADS) {
                int r = e / L, l = e - r * L;
                alphas[((long)(i0 + r) * T1 + step) * L + l] = ((lmask >> r) & 1u) ? s_sc[r * L + l] : 0.f;
            }
        }
        // ---- context: z[r][d] = sum_l alpha[r][l] * ann[b,l,d] for d in this chunk
        const int nv = dn / VW;                         // vectors in the chunk
        const int groups = max(1, min(4, ATT_THREADS / max(nv, 1)));
        const int gsz = ATT_THREADS / groups;           // threads per group
        const bool ctx_thread = tid < ATT_THREADS;       // the context phase runs on the first 4 waves; all waves do the scores
        const int g = ctx_thread ? tid / gsz : groups, tv = tid - (ctx_thread ? g : 0) * gsz;
        float acc[RN][VW];
        if (any) {
            for (int v0 = 0; v0 < nv; v0 += gsz) {
                const int v = v0 + tv;
#pragma unroll
                for (int r = 0; r < RN; ++r)
#pragma unroll
                    for (int c = 0; c < VW; ++c) acc[r][c] = 0.f;
                if (v < nv && g < groups) {
                    const float* base = ann + (long)b * L * D + d0 + v * VW;
                    for (int l = g; l < L; l += groups) {
                        float x[VW];
                        if (VW == 4) { float4 t4 = *reinterpret_cast<const float4*>(base + (long)l * D); x[0] = t4.x; x[1 % VW] = t4.y; x[2 % VW] = t4.z; x[3 % VW] = t4.w; }
                        else x[0] = base[(long)l * D];
#pragma unroll
                        for (int r = 0; r < RN; ++r) { const float al = s_sc[r * L + l];
#pragma unroll
                            for (int c = 0; c < VW; ++c) acc[r][c] = fmaf(al, x[c], acc[r][c]); }
                    }
                }
                // combine the l-groups through LDS in a fixed order
                __syncthreads();
                if (v < nv && g < groups)
#pragma unroll
                    for (int r = 0; r < RN; ++r)
#pragma unroll
                        for (int c = 0; c < VW; ++c) s_part[((g * ATT_RMAX + r) * gsz + tv) * VW + c] = acc[r][c];
                __syncthreads();
                if (g == 0 && v < nv) {
#pragma unroll
                    for (int r = 0; r < RN; ++r) {
                        if (r >= rn) continue;
                        const long orow = (long)(i0 + r);
#pragma unroll
                        for (int c = 0; c < VW; ++c) {
                            float z = 0.f;
                            if (((lmask >> r) & 1u)) for (int gg = 0; gg < groups; ++gg) z += s_part[((gg * ATT_RMAX + r) * gsz + tv) * VW + c];
                            const int d = d0 + v * VW + c;
                            const float beta = ((lmask >> r) & 1u) ? hc[orow * hc_ld + A + d] : 0.f;
                            Z[orow * D + d] = z;
                            XZ[orow * D + d] = beta * z;
                        }
                    }
                }
            }
        } else {
            for (int e = tid; e < rn * dn; e += ATTF_THREADS) { int r = e / dn, d = d0 + e - r * dn; Z[(long)(i0 + r) * D + d] = 0.f; XZ[(long)(i0 + r) * D + d] = 0.f; }
        }
    }
}

// ------------------------------------------------------------------ attention forward, split over the chip
// The fused kernel above runs one workgroup per (image, 256-wide slice of D): 256 workgroups, each recomputing the image's
// scores, and a context phase on 4 waves.  The two kernels below spread the step over ~1000 workgroups:
//   scores : grid (B, ceil(L / 16)), wave per location -> raw scaled scores (N, L) in scratch
//   context: grid (B, D / 64): softmax of the image's RN rows (cheap, redundant per slice), then 16 location groups x 16
//            float4 vectors accumulate the slice of the context; fixed combination order.
constexpr int ATTS_WAVES = 16;
template <int RN>
__global__ __launch_bounds__(ATTS_WAVES * 64) void attention_scores_kernel(const float* __restrict__ U, const float* __restrict__ hc, int hc_ld,
                                                                           const float* __restrict__ wf, float* __restrict__ sc, int R, int L, int A) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* s_q = sm;                 // [RN][A]
    float* s_w = s_q + RN * A;       // [A]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l = blockIdx.y * ATTS_WAVES + wave;
    const float scale = 1.0f / sqrtf((float)L);
    for (int k = tid; k < A; k += ATTS_WAVES * 64) s_w[k] = wf[k];
    for (int r0 = 0; r0 < R; r0 += RN) {
        const int rn = min(RN, R - r0), i0 = b * R + r0;
        __syncthreads();
        for (int e = tid; e < RN * A; e += ATTS_WAVES * 64) { int r = e / A, k = e - r * A; s_q[e] = (r < rn) ? hc[(long)(i0 + r) * hc_ld + k] : 0.f; }
        __syncthreads();
        if (l < L) {
            float part[RN];
#pragma unroll
            for (int r = 0; r < RN; ++r) part[r] = 0.f;
            const float* u = U + ((long)b * L + l) * A;
            for (int k = lane; k < A; k += 64) {
                const float uv = u[k], w = s_w[k];
#pragma unroll
                for (int r = 0; r < RN; ++r) part[r] = fmaf(w, fast_tanh(uv + s_q[r * A + k]), part[r]);
            }
#pragma unroll
            for (int r = 0; r < RN; ++r) { const float s = wave_sum(part[r]); if (lane == 0 && r < rn) sc[(long)(i0 + r) * L + l] = s * scale; }
        }
    }
}

constexpr int ATTC_DCH = 64;          // context slice: 64 features = 16 float4 vectors x 16 location groups per 256 threads
// TA = float, or __bf16: the bf16 copy of the annotations that bf16 mode keeps for the two kernels that stream them every time step
// (context here, dalpha in the backward pass): half the bytes of the decoder's largest per-step stream; products and sums stay fp32.
template <typename TA> __device__ __forceinline__ float4 ld_ann4(const TA* p);
template <> __device__ __forceinline__ float4 ld_ann4<float>(const float* p) { return *reinterpret_cast<const float4*>(p); }
template <> __device__ __forceinline__ float4 ld_ann4<__bf16>(const __bf16* p) {
    typedef __bf16 b4 __attribute__((ext_vector_type(4)));
    const b4 q = *reinterpret_cast<const b4*>(p);
    return make_float4((float)q[0], (float)q[1], (float)q[2], (float)q[3]);
}
template <int RN, typename TA>
__global__ __launch_bounds__(256) void attention_context_kernel(const TA* __restrict__ ann, const float* __restrict__ sc, const float* __restrict__ hc,
                                                                int hc_ld, const int* __restrict__ lengths, int step, float* __restrict__ alphas, int T1,
                                                                float* __restrict__ Z, float* __restrict__ XZ, int R, int L, int D, int A,
                                                                __bf16* __restrict__ xzb) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* s_al = sm;                          // [RN][L]
    float4* s_part = reinterpret_cast<float4*>(sm + ((RN * L + 3) & ~3));   // [16 groups][RN][16 vectors]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d0 = blockIdx.y * ATTC_DCH;
    const int v = tid & 15, g = tid >> 4;
    for (int r0 = 0; r0 < R; r0 += RN) {
        const int rn = min(RN, R - r0), i0 = b * R + r0;
        unsigned lmask = 0;
        for (int r = 0; r < rn; ++r) if (lengths[i0 + r] > step) lmask |= 1u << r;
        __syncthreads();
        // softmax over L of the live rows (wave per row); dead rows and rows past R get zero weights
        for (int r = wave; r < RN; r += 4) {
            const bool livr = (lmask >> r) & 1u;
            float mx = -INFINITY;
            if (livr) for (int l = lane; l < L; l += 64) mx = fmaxf(mx, sc[(long)(i0 + r) * L + l]);
            mx = wave_max(mx);
            float sum = 0.f;
            if (livr) for (int l = lane; l < L; l += 64) { const float e = __expf(sc[(long)(i0 + r) * L + l] - mx); s_al[r * L + l] = e; sum += e; }
            sum = wave_sum(sum);
            const float inv = livr ? 1.0f / sum : 0.f;
            for (int l = lane; l < L; l += 64) s_al[r * L + l] = livr ? s_al[r * L + l] * inv : 0.f;
        }
        __syncthreads();
        if (blockIdx.y == 0)
            for (int e = tid; e < rn * L; e += 256) { int r = e / L, l = e - r * L; alphas[((long)(i0 + r) * T1 + step) * L + l] = s_al[r * L + l]; }
        // context slice
        float4 acc[RN];
#pragma unroll
        for (int r = 0; r < RN; ++r) acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
        const int d = d0 + 4 * v;
        if (d < D && lmask) {
            const TA* base = ann + (long)b * L * D + d;
            for (int l0 = g; l0 < L; l0 += 64) {          // four locations per trip, their loads issued together (L = 196: 4 trips instead of 13)
                float4 x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { const int l = l0 + 16 * u; x[u] = l < L ? ld_ann4<TA>(base + (long)l * D) : make_float4(0.f, 0.f, 0.f, 0.f); }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int l = l0 + 16 * u;
                    if (l >= L) continue;
#pragma unroll
                    for (int r = 0; r < RN; ++r) {
                        const float al = s_al[r * L + l];
                        acc[r].x = fmaf(al, x[u].x, acc[r].x); acc[r].y = fmaf(al, x[u].y, acc[r].y); acc[r].z = fmaf(al, x[u].z, acc[r].z); acc[r].w = fmaf(al, x[u].w, acc[r].w);
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RN; ++r) s_part[(g * RN + r) * 16 + v] = acc[r];
        __syncthreads();
        // thread (r = tid / 16 .., v): sums the 16 location groups in order and writes z and beta * z
        for (int e = tid; e < rn * 16; e += 256) {
            const int r = e >> 4, vv = e & 15, dd = d0 + 4 * vv;
            if (dd >= D) continue;
            float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int gg = 0; gg < 16; ++gg) { const float4 t = s_part[(gg * RN + r) * 16 + vv]; z.x += t.x; z.y += t.y; z.z += t.z; z.w += t.w; }
            const long orow = i0 + r;
            float4 be = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((lmask >> r) & 1u) be = *reinterpret_cast<const float4*>(hc + orow * hc_ld + A + dd);
            *reinterpret_cast<float4*>(Z + orow * D + dd) = z;
            *reinterpret_cast<float4*>(XZ + orow * D + dd) = make_float4(be.x * z.x, be.y * z.y, be.z * z.z, be.w * z.w);
            if (xzb) {
                typedef __bf16 b4 __attribute__((ext_vector_type(4)));
                b4 o; o[0] = (__bf16)(be.x * z.x); o[1] = (__bf16)(be.y * z.y); o[2] = (__bf16)(be.z * z.z); o[3] = (__bf16)(be.w * z.w);
                *reinterpret_cast<b4*>(xzb + orow * D + dd) = o;
            }
        }
    }
}

// ------------------------------------------------------------------ LSTM cell (pointwise part)
// gates (N,4n) pre-activation = h W_hh^T + xz W_ih_z^T + biases (already in HC) + GY (embedding part).
// Gate order i,f,g,o.  Activated gates are written back in place for backward.
__global__ void lstm_cell_fwd_kernel(float* __restrict__ gates, int g_ld, const float* __restrict__ gy,
                                     const float* __restrict__ c_prev, const float* __restrict__ h_prev,
                                     float* __restrict__ c_new, float* __restrict__ h_new,
                                     const int* __restrict__ lengths, int step, int N, int n, __bf16* __restrict__ hb_new = nullptr) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)N * n) return;
    int i = (int)(idx / n), j = (int)(idx - (long)i * n);
    if (lengths && lengths[i] <= step) {       // finished caption: state is carried unchanged (model.py:544 updates live rows only); lengths NULL: every row live
        const float hp = h_prev[idx];
        c_new[idx] = c_prev[idx]; h_new[idx] = hp;
        if (hb_new) hb_new[idx] = (__bf16)hp;
        float* g = gates + (long)i * g_ld;
        g[j] = 0.f; g[n + j] = 0.f; g[2 * n + j] = 0.f; g[3 * n + j] = 0.f;
        return;
    }
    float* g = gates + (long)i * g_ld;
    const float* y = gy ? gy + (long)i * 4 * n : nullptr;
    float gi = fast_sigmoid(g[j] + (y ? y[j] : 0.f));
    float gf = fast_sigmoid(g[n + j] + (y ? y[n + j] : 0.f));
    float gg = fast_tanh(g[2 * n + j] + (y ? y[2 * n + j] : 0.f));
    float go = fast_sigmoid(g[3 * n + j] + (y ? y[3 * n + j] : 0.f));
    float c = gf * c_prev[idx] + gi * gg;
    c_new[idx] = c;
    const float hn = go * fast_tanh(c);
    h_new[idx] = hn;
    if (hb_new) hb_new[idx] = (__bf16)hn;          // bf16 copy: operand of the next step's GEMM (bf16 mode)
    g[j] = gi; g[n + j] = gf; g[2 * n + j] = gg; g[3 * n + j] = go;
}

// backward of the cell.  dh_carry/dc_carry are the running gradients w.r.t. h_t / c_t from later steps;
// dh_out is the gradient arriving from the output layer of this step.  Writes dG (pre-activation gate
// grads) and leaves dh_carry = 0 for live rows (the h_{t-1} gradient is accumulated by the GEMM after).
__global__ void lstm_cell_bwd_kernel(const float* __restrict__ gates, int g_ld, const float* __restrict__ c_prev,
                                     const float* __restrict__ c_new, const float* __restrict__ dh_out,
                                     float* __restrict__ dh_carry, float* __restrict__ dc_carry,
                                     float* __restrict__ dgates, int dg_ld,
                                     const int* __restrict__ lengths, int step, int N, int n, __bf16* __restrict__ dgb = nullptr) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)N * n) return;
    int i = (int)(idx / n), j = (int)(idx - (long)i * n);
    float* dg = dgates + (long)i * dg_ld;
    __bf16* db = dgb ? dgb + (long)i * dg_ld : nullptr;            // bf16 copy with the same row stride (operand of this step's GEMMs)
    if (lengths && lengths[i] <= step) {
        dg[j] = 0.f; dg[n + j] = 0.f; dg[2 * n + j] = 0.f; dg[3 * n + j] = 0.f;
        if (db) { db[j] = (__bf16)0.f; db[n + j] = (__bf16)0.f; db[2 * n + j] = (__bf16)0.f; db[3 * n + j] = (__bf16)0.f; }
        return;
    }
    const float* g = gates + (long)i * g_ld;
    float gi = g[j], gf = g[n + j], gg = g[2 * n + j], go = g[3 * n + j];
    float dh = dh_carry[idx] + (dh_out ? dh_out[idx] : 0.f);
    float tc = fast_tanh(c_new[idx]);
    float dc = dc_carry[idx] + dh * go * (1.f - tc * tc);
    const float d0 = dc * gg * gi * (1.f - gi), d1 = dc * c_prev[idx] * gf * (1.f - gf), d2 = dc * gi * (1.f - gg * gg), d3 = dh * tc * go * (1.f - go);
    dg[j] = d0; dg[n + j] = d1; dg[2 * n + j] = d2; dg[3 * n + j] = d3;
    if (db) { db[j] = (__bf16)d0; db[n + j] = (__bf16)d1; db[2 * n + j] = (__bf16)d2; db[3 * n + j] = (__bf16)d3; }
    dc_carry[idx] = dc * gf;
    dh_carry[idx] = 0.f;
}

// ------------------------------------------------------------------ layer-normalised LSTM cell (Ba et al. 2016)
//   x^_k = (a_k - mean_k) * rstd_k, k in {i,f,g,o} over the n units of each gate;  i,f,o = sigmoid, g = tanh of gamma_k x^_k + beta_k
//   c_t = f c_{t-1} + i g (carried un-normalised);  c^ = (c_t - mean_c) * rstd_c;  h_t = o tanh(gamma_c c^ + beta_c)
// biased variance, eps = LN_EPS; mean first, then the squared deviations (two passes over the row in LDS).
// One block walks rows blockIdx.x, blockIdx.x + gridDim.x, ...; a thread owns the units tid, tid + blockDim.x, ... of its row in every
// pass, so everything it reads back from LDS or from an in-place buffer (c_new == c_prev, h_new == h_prev) it wrote or read itself.
// dyn LDS: [LN_RED floats: cross-wave partials][5n floats: the row]
constexpr float LN_EPS = 1e-5f;
constexpr int LN_RED = 32;                     // 8 sums x 4 waves
constexpr int LN_MAX_SLOTS = 1024;             // blocks (= partial-sum slots of the backward kernel): one row a block up to here (C2: 640 rows)

// the K sums of a block, the same bits in every thread: lanes by shuffle, waves in index order through LDS
template <int K>
__device__ __forceinline__ void ln_block_sum(float (&v)[K], float* s_red) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    const int nw = blockDim.x >> 6;
    if (nw == 1) return;
    __syncthreads();                           // the previous sums have been read
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) s_red[(threadIdx.x >> 6) * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) { float s = 0.f; for (int w = 0; w < nw; ++w) s += s_red[w * K + k]; v[k] = s; }
}

// Same contract as lstm_cell_fwd_kernel (gates in place, gy addend, lengths / step mask, bf16 copy of h).  xhat (N, 5n) = [x^_i x^_f x^_g
// x^_o c^] and rstd (N, 5) are saved for the backward pass when xhat is not NULL (dead rows: not written).
__global__ void lstm_ln_cell_fwd_kernel(float* gates, int g_ld, const float* __restrict__ gy, const float* c_prev, const float* h_prev,
                                        float* c_new, float* h_new, const int* __restrict__ lengths, int step, int N, int n, __bf16* hb_new,
                                        const float* __restrict__ gam_g, const float* __restrict__ bet_g, const float* __restrict__ gam_c,
                                        const float* __restrict__ bet_c, float* __restrict__ xhat, float* __restrict__ rstd) {
    extern __shared__ __attribute__((aligned(16))) float ln_sm[];
    float* s_red = ln_sm; float* s_row = ln_sm + LN_RED;
    const int tid = threadIdx.x, bd = blockDim.x;
    const float inv_n = 1.f / (float)n;
    for (int row = blockIdx.x; row < N; row += gridDim.x) {
        float* g = gates + (long)row * g_ld;
        const long r0 = (long)row * n;
        if (lengths && lengths[row] <= step) {           // finished caption: state carried, zero gates (block-uniform branch)
            for (int j = tid; j < n; j += bd) {
                const float hp = h_prev[r0 + j];
                c_new[r0 + j] = c_prev[r0 + j]; h_new[r0 + j] = hp;
                if (hb_new) hb_new[r0 + j] = (__bf16)hp;
                g[j] = 0.f; g[n + j] = 0.f; g[2 * n + j] = 0.f; g[3 * n + j] = 0.f;
            }
            continue;
        }
        const float* y = gy ? gy + (long)row * 4 * n : nullptr;
        float mu[4] = {0.f, 0.f, 0.f, 0.f};
        for (int j = tid; j < n; j += bd) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { const float a = g[k * n + j] + (y ? y[k * n + j] : 0.f); s_row[k * n + j] = a; mu[k] += a; }
        }
        ln_block_sum<4>(mu, s_red);
        float rs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) mu[k] *= inv_n;
        for (int j = tid; j < n; j += bd) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { const float dlt = s_row[k * n + j] - mu[k]; rs[k] = fmaf(dlt, dlt, rs[k]); }
        }
        ln_block_sum<4>(rs, s_red);
#pragma unroll
        for (int k = 0; k < 4; ++k) rs[k] = 1.f / sqrtf(rs[k] * inv_n + LN_EPS);
        float* xh = xhat ? xhat + (long)row * 5 * n : nullptr;
        float mc[1] = {0.f};
        for (int j = tid; j < n; j += bd) {
            float act[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float x = (s_row[k * n + j] - mu[k]) * rs[k];
                if (xh) xh[k * n + j] = x;
                act[k] = fmaf(x, gam_g[k * n + j], bet_g[k * n + j]);
            }
            const float gi = fast_sigmoid(act[0]), gf = fast_sigmoid(act[1]), gg = fast_tanh(act[2]), go = fast_sigmoid(act[3]);
            const float c = gf * c_prev[r0 + j] + gi * gg;
            c_new[r0 + j] = c;
            g[j] = gi; g[n + j] = gf; g[2 * n + j] = gg; g[3 * n + j] = go;
            s_row[3 * n + j] = go; s_row[4 * n + j] = c;
            mc[0] += c;
        }
        ln_block_sum<1>(mc, s_red);
        const float mean_c = mc[0] * inv_n;
        float qc[1] = {0.f};
        for (int j = tid; j < n; j += bd) { const float dlt = s_row[4 * n + j] - mean_c; qc[0] = fmaf(dlt, dlt, qc[0]); }
        ln_block_sum<1>(qc, s_red);
        const float rs_c = 1.f / sqrtf(qc[0] * inv_n + LN_EPS);
        for (int j = tid; j < n; j += bd) {
            const float ch = (s_row[4 * n + j] - mean_c) * rs_c;
            if (xh) xh[4 * n + j] = ch;
            const float hn = s_row[3 * n + j] * fast_tanh(fmaf(ch, gam_c[j], bet_c[j]));
            h_new[r0 + j] = hn;
            if (hb_new) hb_new[r0 + j] = (__bf16)hn;
        }
        if (rstd && tid == 0) { float* r = rstd + (long)row * 5; r[0] = rs[0]; r[1] = rs[1]; r[2] = rs[2]; r[3] = rs[3]; r[4] = rs_c; }
    }
}

// Same contract as lstm_cell_bwd_kernel (dh_carry / dc_carry, dead rows: zero dgates, bf16 copy of dgates); dgates is the gradient of the
// PRE-NORM sum a.  Per live row:
//   dh = dh_carry + dh_out;  tc = tanh(gamma_c c^ + beta_c);  du = dh o (1 - tc^2);  d a^_o = dh tc o (1 - o)
//   d c^ = du gamma_c;  dc = dc_carry + rstd_c (d c^ - mean(d c^) - c^ mean(d c^ c^))                            two row sums
//   d a^_i = dc g i (1 - i), d a^_f = dc c_{t-1} f (1 - f), d a^_g = dc i (1 - g^2);  d x^_k = d a^_k gamma_k
//   d a_k = rstd_k (d x^_k - mean(d x^_k) - x^_k mean(d x^_k x^_k))                                              eight row sums
// Parameter gradients: block b ADDS its rows' d a^_k x^_k, d a^_k, du c^, du into slot b of part (gridDim.x, 10n) =
// [dgamma_g 4n | dbeta_g 4n | dgamma_c n | dbeta_c n] with a plain read-modify-write; a slot has one writer per launch, the launches of a
// backward pass follow each other on one stream, and the sum over slots comes after the loop: fixed order, no atomics.  part NULL: skipped.
__global__ void lstm_ln_cell_bwd_kernel(const float* __restrict__ gates, int g_ld, const float* __restrict__ c_prev, const float* __restrict__ xhat,
                                        const float* __restrict__ rstd, const float* __restrict__ dh_out, float* __restrict__ dh_carry,
                                        float* __restrict__ dc_carry, float* __restrict__ dgates, int dg_ld, const int* __restrict__ lengths, int step,
                                        int N, int n, __bf16* __restrict__ dgb, const float* __restrict__ gam_g, const float* __restrict__ gam_c,
                                        const float* __restrict__ bet_c, float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float ln_sm[];
    float* s_red = ln_sm; float* s_row = ln_sm + LN_RED;
    const int tid = threadIdx.x, bd = blockDim.x;
    const float inv_n = 1.f / (float)n;
    float* slot = part ? part + (long)blockIdx.x * 10 * n : nullptr;
    for (int row = blockIdx.x; row < N; row += gridDim.x) {
        float* dg = dgates + (long)row * dg_ld;
        __bf16* db = dgb ? dgb + (long)row * dg_ld : nullptr;
        if (lengths && lengths[row] <= step) {
            for (int j = tid; j < n; j += bd) {
                dg[j] = 0.f; dg[n + j] = 0.f; dg[2 * n + j] = 0.f; dg[3 * n + j] = 0.f;
                if (db) { db[j] = (__bf16)0.f; db[n + j] = (__bf16)0.f; db[2 * n + j] = (__bf16)0.f; db[3 * n + j] = (__bf16)0.f; }
            }
            continue;
        }
        const float* g = gates + (long)row * g_ld;
        const float* xh = xhat + (long)row * 5 * n;
        const float* rr = rstd + (long)row * 5;
        const float rs[4] = {rr[0], rr[1], rr[2], rr[3]};
        const float rs_c = rr[4];
        const long r0 = (long)row * n;
        float sc[2] = {0.f, 0.f};
        for (int j = tid; j < n; j += bd) {
            const float go = g[3 * n + j], ch = xh[4 * n + j], gc = gam_c[j];
            const float tc = fast_tanh(fmaf(ch, gc, bet_c[j]));
            const float dh = dh_carry[r0 + j] + (dh_out ? dh_out[r0 + j] : 0.f);
            const float du = dh * go * (1.f - tc * tc);
            if (slot) { slot[8 * n + j] += du * ch; slot[9 * n + j] += du; }
            const float dch = du * gc;
            s_row[3 * n + j] = dh * tc * go * (1.f - go);
            s_row[4 * n + j] = dch;
            sc[0] += dch; sc[1] = fmaf(dch, ch, sc[1]);
        }
        ln_block_sum<2>(sc, s_red);
        const float m1 = sc[0] * inv_n, m2 = sc[1] * inv_n;
        float sg[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int j = tid; j < n; j += bd) {
            const float ch = xh[4 * n + j];
            const float dc = dc_carry[r0 + j] + rs_c * (s_row[4 * n + j] - m1 - ch * m2);
            const float gi = g[j], gf = g[n + j], gg = g[2 * n + j];
            const float da[4] = {dc * gg * gi * (1.f - gi), dc * c_prev[r0 + j] * gf * (1.f - gf), dc * gi * (1.f - gg * gg), s_row[3 * n + j]};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float x = xh[k * n + j];
                if (slot) { slot[k * n + j] += da[k] * x; slot[4 * n + k * n + j] += da[k]; }
                const float dx = da[k] * gam_g[k * n + j];
                s_row[k * n + j] = dx;
                sg[k] += dx; sg[4 + k] = fmaf(dx, x, sg[4 + k]);
            }
            dc_carry[r0 + j] = dc * gf;
            dh_carry[r0 + j] = 0.f;
        }
        ln_block_sum<8>(sg, s_red);
#pragma unroll
        for (int k = 0; k < 8; ++k) sg[k] *= inv_n;
        for (int j = tid; j < n; j += bd) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = rs[k] * (s_row[k * n + j] - sg[k] - xh[k * n + j] * sg[4 + k]);
                dg[k * n + j] = d;
                if (db) db[k * n + j] = (__bf16)d;
            }
        }
    }
}

// ------------------------------------------------------------------ attention backward (one decode step)
// grid = B; block = 256.  Per live caption row i of image b:
//   dz = dZ_out + dXZ*beta ; dbeta_pre = dXZ * z * beta(1-beta)
//   dalpha_l = dz . ann[b,l,:] + dalpha_ext ; ds = alpha (dalpha - sum alpha dalpha)
//   dpre_lk = ds_l L^-1/2 w_k (1 - tanh^2(U_lk + q_k)) ; dq_k = sum_l dpre ; dU += sum_r dpre ; dw_k += sum ds L^-1/2 tanh
// dyn LDS: [RMAX*L alpha][RMAX*L dalpha/ds][RMAX*A q][A w][RMAX*D dz][4*RMAX*A dq partial][4*A dw partial]
constexpr int ATTB_WAVES = 16;                 // 1024 threads: one block per image, so hide latency with waves
constexpr int ATTB_THREADS = ATTB_WAVES * 64;
template <int RN>
__global__ __launch_bounds__(ATTB_THREADS) void attention_bwd_kernel(
    const float* __restrict__ ann, const float* __restrict__ U, const float* __restrict__ hc, int hc_ld,
    const float* __restrict__ wf, const int* __restrict__ lengths, int step,
    const float* __restrict__ alphas, const float* __restrict__ dalphas_ext, int T1,
    const float* __restrict__ Zs, const float* __restrict__ dZ_out, const float* __restrict__ dXZ,
    float* __restrict__ DZ, float* __restrict__ dhc, int dhc_ld, float* __restrict__ dU, float* __restrict__ dwf_part,
    int R, int L, int D, int A) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* s_al = sm;                         // [RMAX][L]
    float* s_da = s_al + ATT_RMAX * L;        // [RMAX][L]
    float* s_q = s_da + ATT_RMAX * L;         // [RMAX][A]
    float* s_w = s_q + ATT_RMAX * A;          // [A]
    float* s_dz = s_w + A;                    // [RMAX][D]
    float* s_dq = s_dz + ATT_RMAX * D;        // [waves][RMAX][A]
    float* s_dw = s_dq + ATTB_WAVES * ATT_RMAX * A;    // [waves][A]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float scale = 1.0f / sqrtf((float)L);
    for (int k = tid; k < A; k += ATTB_THREADS) s_w[k] = wf[k];
    for (int e = tid; e < ATTB_WAVES * A; e += ATTB_THREADS) s_dw[e] = 0.f;

    for (int r0 = 0; r0 < R; r0 += RN) {
        const int rn = min(RN, R - r0);
        const int i0 = b * R + r0;
        unsigned lmask = 0;
        for (int r = 0; r < rn; ++r) if (lengths[i0 + r] > step) lmask |= 1u << r;
        const bool any = lmask != 0;
        __syncthreads();
        // gate backward + dz for every row of the pass (dead rows and rows past R: zeros, so the loops below run unguarded)
        for (int e = tid; e < RN * D; e += ATTB_THREADS) {
            int r = e / D, d = e - r * D; long row = i0 + r;
            float dz = 0.f, dbp = 0.f;
            if (((lmask >> r) & 1u)) {
                float beta = hc[row * hc_ld + A + d], z = Zs[row * D + d], dx = dXZ[row * D + d];
                dz = dZ_out[row * D + d] + dx * beta;
                dbp = dx * z * beta * (1.f - beta);
            }
            s_dz[r * D + d] = dz;
            if (r < rn) { DZ[row * D + d] = dz; dhc[row * dhc_ld + A + d] = dbp; }
        }
        if (!any) {
            for (int e = tid; e < rn * A; e += ATTB_THREADS) { int r = e / A, k = e - r * A; dhc[(long)(i0 + r) * dhc_ld + k] = 0.f; }
            continue;
        }
        // dead rows run on q = 0: their ds is 0, but 0 * (1 - tanh^2) is only 0 for a finite tanh, and nothing promises that a finished row of hc is finite
        for (int e = tid; e < RN * A; e += ATTB_THREADS) { int r = e / A, k = e - r * A; s_q[r * A + k] = ((lmask >> r) & 1u) ? hc[(long)(i0 + r) * hc_ld + k] : 0.f; }
        for (int e = tid; e < RN * L; e += ATTB_THREADS) { int r = e / L, l = e - r * L; s_al[r * L + l] = ((lmask >> r) & 1u) ? alphas[((long)(i0 + r) * T1 + step) * L + l] : 0.f; }
        __syncthreads();
        // ---- dalpha[r][l] = dz[r] . ann[b,l,:]  (wave per location)
        for (int l = wave; l < L; l += ATTB_WAVES) {
            float part[RN];
#pragma unroll
            for (int r = 0; r < RN; ++r) part[r] = 0.f;
            const float* a = ann + ((long)b * L + l) * D;
            for (int d = lane; d < D; d += 64) {
                float av = a[d];
#pragma unroll
                for (int r = 0; r < RN; ++r) part[r] = fmaf(av, s_dz[r * D + d], part[r]);
            }
#pragma unroll
            for (int r = 0; r < RN; ++r) {
                float s = wave_sum(part[r]);
                if (lane == 0) s_da[r * L + l] = ((lmask >> r) & 1u) ? s + (dalphas_ext ? dalphas_ext[((long)(i0 + r) * T1 + step) * L + l] : 0.f) : 0.f;
            }
        }
        __syncthreads();
        // ---- softmax backward, wave per row: ds = alpha * (dalpha - sum alpha*dalpha)
        for (int r = wave; r < rn; r += ATTB_WAVES) {
            if (!((lmask >> r) & 1u)) continue;
            float dot = 0.f;
            for (int l = lane; l < L; l += 64) dot += s_al[r * L + l] * s_da[r * L + l];
            dot = wave_sum(dot);
            for (int l = lane; l < L; l += 64) s_da[r * L + l] = s_al[r * L + l] * (s_da[r * L + l] - dot) * scale;
        }
        __syncthreads();
        // ---- through tanh: wave per location, lanes over the attention dim (2 per lane at A=128)
        for (int k0 = 0; k0 < A; k0 += 64) {
            const int k = k0 + lane;
            float dq[RN]; float dw = 0.f;
#pragma unroll
            for (int r = 0; r < RN; ++r) dq[r] = 0.f;
            if (k < A) {
                const float w = s_w[k];
                for (int l = wave; l < L; l += ATTB_WAVES) {
                    const long uo = ((long)b * L + l) * A + k;
                    const float uv = U[uo];
                    float du = 0.f;
#pragma unroll
                    for (int r = 0; r < RN; ++r) {             // dead rows: ds = 0
                        float th = fast_tanh(uv + s_q[r * A + k]);
                        float ds = s_da[r * L + l];
                        float dp = ds * w * (1.f - th * th);
                        dq[r] += dp; du += dp; dw = fmaf(ds, th, dw);
                    }
                    dU[uo] += du;                   // this block owns image b: plain read-modify-write, fixed order
                }
#pragma unroll
                for (int r = 0; r < RN; ++r) s_dq[(wave * ATT_RMAX + r) * A + k] = dq[r];
                s_dw[wave * A + k] += dw;
            }
        }
        __syncthreads();
        for (int e = tid; e < rn * A; e += ATTB_THREADS) {
            int r = e / A, k = e - r * A;
            float s = 0.f;
            if (((lmask >> r) & 1u)) for (int w = 0; w < ATTB_WAVES; ++w) s += s_dq[(w * ATT_RMAX + r) * A + k];
            dhc[(long)(i0 + r) * dhc_ld + k] = s;
        }
    }
    __syncthreads();
    for (int k = tid; k < A; k += ATTB_THREADS) { float sw = 0.f; for (int w = 0; w < ATTB_WAVES; ++w) sw += s_dw[w * A + k]; dwf_part[(long)b * A + k] += sw; }
}

// ------------------------------------------------------------------ attention backward, split over the chip (see the forward split)
//   dalpha : grid (B, ceil(L / 16)): dz rows of the image in LDS (block 0 of an image also writes DZ and the gate gradient),
//            wave per location: dalpha[r][l] = dz[r] . ann[b, l, :] (+ external gradient) -> scratch (N, L)
//   tanh   : grid (B, ceil(A / 32)): softmax backward of the image's rows (redundant per slice), then 32 attention units x 32
//            location lanes go through the tanh; the block owns dU[b, :, its units], dq and dw of its units.
template <int RN, typename TA>
__global__ __launch_bounds__(1024) void attention_bwd_dalpha_kernel(const TA* __restrict__ ann, const float* __restrict__ hc, int hc_ld,
        const int* __restrict__ lengths, int step, const float* __restrict__ dalphas_ext, int T1, const float* __restrict__ Zs,
        const float* __restrict__ dZ_out, const float* __restrict__ dXZ, float* __restrict__ DZ, float* __restrict__ dhc, int dhc_ld,
        float* __restrict__ da, int R, int L, int D, int A, __bf16* __restrict__ dhcb) {
    extern __shared__ __attribute__((aligned(16))) float s_dz[];          // [RN][D]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l = blockIdx.y * 16 + wave;
    for (int r0 = 0; r0 < R; r0 += RN) {
        const int rn = min(RN, R - r0), i0 = b * R + r0;
        unsigned lmask = 0;
        for (int r = 0; r < rn; ++r) if (lengths[i0 + r] > step) lmask |= 1u << r;
        __syncthreads();
        for (int e = tid; e < RN * D; e += 1024) {
            const int r = e / D, d = e - r * D; const long row = i0 + r;
            float dz = 0.f, dbp = 0.f;
            if ((lmask >> r) & 1u) {
                const float beta = hc[row * hc_ld + A + d], z = Zs[row * D + d], dx = dXZ[row * D + d];
                dz = dZ_out[row * D + d] + dx * beta;
                dbp = dx * z * beta * (1.f - beta);
            }
            s_dz[e] = dz;
            if (blockIdx.y == 0 && r < rn) { DZ[row * D + d] = dz; dhc[row * dhc_ld + A + d] = dbp; if (dhcb) dhcb[row * dhc_ld + A + d] = (__bf16)dbp; }
        }
        __syncthreads();
        if (l < L) {
            float part[RN];
#pragma unroll
            for (int r = 0; r < RN; ++r) part[r] = 0.f;
            const TA* a = ann + ((long)b * L + l) * D;
            // 16 (fp32) / 8 (bf16) bytes per lane, two loads in flight (D % 4 == 0: the split kernels' launch condition); the 4-byte form
            // walked D / 64 dependent trips: 27.7 us for C4's 65 MB
            for (int d0 = lane * 4; d0 < D; d0 += 512) {
                const int d1 = d0 + 256;
                const float4 av0 = ld_ann4<TA>(a + d0);
                const float4 av1 = d1 < D ? ld_ann4<TA>(a + d1) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int r = 0; r < RN; ++r) {
                    const float4 z0 = *reinterpret_cast<const float4*>(s_dz + r * D + d0);
                    float p = part[r];
                    p = fmaf(av0.x, z0.x, p); p = fmaf(av0.y, z0.y, p); p = fmaf(av0.z, z0.z, p); p = fmaf(av0.w, z0.w, p);
                    if (d1 < D) {
                        const float4 z1 = *reinterpret_cast<const float4*>(s_dz + r * D + d1);
                        p = fmaf(av1.x, z1.x, p); p = fmaf(av1.y, z1.y, p); p = fmaf(av1.z, z1.z, p); p = fmaf(av1.w, z1.w, p);
                    }
                    part[r] = p;
                }
            }
#pragma unroll
            for (int r = 0; r < RN; ++r) {
                const float sdot = wave_sum(part[r]);
                if (lane == 0 && r < rn)
                    da[(long)(i0 + r) * L + l] = ((lmask >> r) & 1u) ? sdot + (dalphas_ext ? dalphas_ext[((long)(i0 + r) * T1 + step) * L + l] : 0.f) : 0.f;
            }
        }
    }
}

constexpr int ATTB_KCH = 32;
template <int RN>
__global__ __launch_bounds__(1024) void attention_bwd_tanh_kernel(const float* __restrict__ U, const float* __restrict__ hc, int hc_ld, const float* __restrict__ wf,
        const int* __restrict__ lengths, int step, const float* __restrict__ alphas, int T1, const float* __restrict__ da, float* __restrict__ dhc,
        int dhc_ld, float* __restrict__ dU, float* __restrict__ dwf_part, int R, int L, int A, __bf16* __restrict__ dhcb) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* s_ds = sm;                               // [RN][L]
    float* s_q = s_ds + RN * L;                     // [RN][KCH]
    float* s_red = s_q + RN * ATTB_KCH;             // [32 lanes][RN + 1][KCH]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kk = tid & 31, lg = tid >> 5, k = blockIdx.y * ATTB_KCH + kk;
    const float scale = 1.0f / sqrtf((float)L);
    const float w = k < A ? wf[k] : 0.f;
    float dw_total = 0.f;
    for (int r0 = 0; r0 < R; r0 += RN) {
        const int rn = min(RN, R - r0), i0 = b * R + r0;
        unsigned lmask = 0;
        for (int r = 0; r < rn; ++r) if (lengths[i0 + r] > step) lmask |= 1u << r;
        __syncthreads();
        // softmax backward: ds = alpha * (dalpha - sum alpha * dalpha) * L^-1/2, wave per row; dead rows: 0
        for (int r = wave; r < RN; r += 16) {
            const bool livr = (lmask >> r) & 1u;
            float dot = 0.f;
            if (livr) for (int l = lane; l < L; l += 64) dot += alphas[((long)(i0 + r) * T1 + step) * L + l] * da[(long)(i0 + r) * L + l];
            dot = wave_sum(dot);
            for (int l = lane; l < L; l += 64)
                s_ds[r * L + l] = livr ? alphas[((long)(i0 + r) * T1 + step) * L + l] * (da[(long)(i0 + r) * L + l] - dot) * scale : 0.f;
        }
        for (int e = tid; e < RN * ATTB_KCH; e += 1024) {
            const int r = e / ATTB_KCH, k2 = blockIdx.y * ATTB_KCH + (e - r * ATTB_KCH);
            s_q[e] = (((lmask >> r) & 1u) && k2 < A) ? hc[(long)(i0 + r) * hc_ld + k2] : 0.f;          // dead rows: q = 0 (finite), ds = 0
        }
        __syncthreads();
        float dq[RN], dw = 0.f;
#pragma unroll
        for (int r = 0; r < RN; ++r) dq[r] = 0.f;
        if (k < A && lmask) {
            for (int l = lg; l < L; l += 32) {
                const long uo = ((long)b * L + l) * A + k;
                const float uv = U[uo];
                float du = 0.f;
#pragma unroll
                for (int r = 0; r < RN; ++r) {
                    const float th = fast_tanh(uv + s_q[r * ATTB_KCH + kk]);
                    const float ds = s_ds[r * L + l];
                    const float dp = ds * w * (1.f - th * th);
                    dq[r] += dp; du += dp; dw = fmaf(ds, th, dw);
                }
                dU[uo] += du;                        // (b, k) belongs to this block alone: plain read-modify-write, fixed order
            }
        }
#pragma unroll
        for (int r = 0; r < RN; ++r) s_red[(lg * (RN + 1) + r) * ATTB_KCH + kk] = dq[r];
        s_red[(lg * (RN + 1) + RN) * ATTB_KCH + kk] = dw;
        __syncthreads();
        for (int e = tid; e < (RN + 1) * ATTB_KCH; e += 1024) {
            const int r = e / ATTB_KCH, k2 = e - r * ATTB_KCH, kg = blockIdx.y * ATTB_KCH + k2;
            float sacc = 0.f;
            for (int g2 = 0; g2 < 32; ++g2) sacc += s_red[(g2 * (RN + 1) + r) * ATTB_KCH + k2];
            if (kg < A) {
                if (r < RN) { if (r < rn) { dhc[(long)(i0 + r) * dhc_ld + kg] = sacc; if (dhcb) dhcb[(long)(i0 + r) * dhc_ld + kg] = (__bf16)sacc; } }
                else s_q[k2] = sacc;                 // dw of this pass (s_q is free until the next pass reloads it)
            }
        }
        __syncthreads();
        if (tid < ATTB_KCH) dw_total += s_q[tid];
    }
    if (tid < ATTB_KCH && k < A) dwf_part[(long)b * A + k] += dw_total;
}

// d ann[b, l, :] += sum over the image's captions r and steps t of alpha[i, t, l] * DZ[t, i, :]  (i = b*R + r):
// the context path of the attention backward, summed over time.  One block per (image, 256-wide slice of D).  The
// image's alphas are staged in LDS once, rows zero-padded to a multiple of 4 floats so that a location slab is NQ
// 16-byte LDS reads with a compile-time trip count (a guard per location serialised every FMA behind its own LDS
// read: 390 us); the (r, t) loop has no barrier and keeps 8 DZ loads in flight.  Fixed order: deterministic.
template <int NQ>
__global__ __launch_bounds__(256) void dann_from_context_kernel(const float* __restrict__ alphas, const float* __restrict__ DZ, const int* __restrict__ lengths,
                                         float* __restrict__ dann, int accumulate, int R, int N, int T1, int L, int D) {
    extern __shared__ float4 s_a4[];  // [R*T1][Lq] float4: alphas of this image, rows padded with zeros
    const int b = blockIdx.x, d = blockIdx.y * blockDim.x + threadIdx.x;
    const int Lq = ((L + 3) / 4 + NQ - 1) / NQ * NQ, Lp = Lq * 4;          // padded row: whole slabs
    float* s_a = reinterpret_cast<float*>(s_a4);
    for (int idx = threadIdx.x; idx < R * T1 * Lp; idx += blockDim.x) {
        const int row = idx / Lp, l = idx - row * Lp;
        s_a[idx] = l < L ? alphas[((long)b * R * T1 + row) * L + l] : 0.f;
    }
    __syncthreads();
    if (d >= D) return;
    for (int q0 = 0; q0 < Lq; q0 += NQ) {
        float acc[NQ * 4];
#pragma unroll
        for (int j = 0; j < NQ * 4; ++j) acc[j] = 0.f;
        for (int r = 0; r < R; ++r) {
            const int i = b * R + r; const int len = min(lengths[i], T1);
            const float4* sa = s_a4 + (long)r * T1 * Lq + q0;
            for (int t0 = 0; t0 < len; t0 += 8) {             // 8 independent DZ loads in flight, then 8 x NQ*4 FMAs
                float dz[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) dz[u] = (t0 + u < len) ? DZ[((long)(t0 + u) * N + i) * D + d] : 0.f;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int tt = (t0 + u < T1) ? t0 + u : T1 - 1;          // stay inside the staged rows; dz is 0 past len
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        const float4 a4 = sa[tt * Lq + q];
                        acc[4 * q] = fmaf(a4.x, dz[u], acc[4 * q]); acc[4 * q + 1] = fmaf(a4.y, dz[u], acc[4 * q + 1]);
                        acc[4 * q + 2] = fmaf(a4.z, dz[u], acc[4 * q + 2]); acc[4 * q + 3] = fmaf(a4.w, dz[u], acc[4 * q + 3]);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NQ * 4; ++j) {
            const int l = q0 * 4 + j;
            if (l < L) {
                float* p = dann + ((long)b * L + l) * D + d;
                *p = accumulate ? (*p + acc[j]) : acc[j];
            }
        }
    }
}

// dann[b,l,d] += dmean[b,d] / L  (backward of the spatial mean in InitLSTM)
__global__ void dann_add_mean_kernel(float* __restrict__ dann, const float* __restrict__ dmean, int L, int D, long total) {
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    long b = e / ((long)L * D); int d = (int)(e % D);
    dann[e] += dmean[b * D + d] / (float)L;
}

// ------------------------------------------------------------------ reductions for bias grads
// out[c] (+)= sum_r x[r*ld + c], rows split over grid.y into fixed chunks, partials reduced in order.
__global__ void colsum_part_kernel(const float* __restrict__ x, long ld, int rows, int cols, int rows_per, float* __restrict__ part) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cols) return;
    int r0 = blockIdx.y * rows_per, r1 = min(rows, r0 + rows_per);
    float s = 0.f;
    for (int r = r0; r < r1; ++r) s += x[(long)r * ld + c];
    part[(long)blockIdx.y * cols + c] = s;
}
// the same, four columns per thread (16-byte loads; x 16-byte aligned, ld % 4 == 0, cols % 4 == 0) and four independent row
// accumulators so that four loads are in flight per thread; combined in a fixed order
__global__ void colsum_part4_kernel(const float* __restrict__ x, long ld, int rows, int cols4, int rows_per, float* __restrict__ part) {
    const int c4 = blockIdx.x * blockDim.x + threadIdx.x;
    if (c4 >= cols4) return;
    const int r0 = blockIdx.y * rows_per, r1 = min(rows, r0 + rows_per);
    float4 a[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    int r = r0;
    for (; r + 3 < r1; r += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float4 v = *reinterpret_cast<const float4*>(x + (long)(r + u) * ld + 4 * c4);
            a[u].x += v.x; a[u].y += v.y; a[u].z += v.z; a[u].w += v.w;
        }
    }
    for (; r < r1; ++r) { const float4 v = *reinterpret_cast<const float4*>(x + (long)r * ld + 4 * c4); a[0].x += v.x; a[0].y += v.y; a[0].z += v.z; a[0].w += v.w; }
    float4 s;
    s.x = (a[0].x + a[1].x) + (a[2].x + a[3].x); s.y = (a[0].y + a[1].y) + (a[2].y + a[3].y);
    s.z = (a[0].z + a[1].z) + (a[2].z + a[3].z); s.w = (a[0].w + a[1].w) + (a[2].w + a[3].w);
    *reinterpret_cast<float4*>(part + (long)blockIdx.y * cols4 * 4 + 4 * c4) = s;
}
__global__ void colsum_finish_kernel(const float* __restrict__ part, int nparts, int cols, float* __restrict__ out, int accumulate, float scale) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cols) return;
    float s = 0.f;
    for (int p = 0; p < nparts; ++p) s += part[(long)p * cols + c];
    s *= scale;
    out[c] = accumulate ? out[c] + s : s;
}

// embedding gradient, deterministic (no floating-point atomics: the result does not depend on scheduling).  The padding row
// and rows without a token (-1) get zeros.
constexpr int EMB_LIST = 1024;
// Four small launches:
// count tokens per vocabulary row (integer atomics: the counts do not depend on the order), exclusive scan, scatter the token
// positions into per-row segments (unordered), then one block per row SORTS its segment and adds the dY rows in increasing
// position -- the summation order is again fixed.  Rows with more than EMB_LIST tokens take the scanning kernel's path.
__global__ void embedding_count_kernel(const int* __restrict__ tok, int rows, int V, int padding_idx, int* __restrict__ count) {
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    int v = tok[r];
    if (v >= 0 && v < V && v != padding_idx) atomicAdd(&count[v], 1);
}
__global__ __launch_bounds__(1024) void embedding_scan_kernel(const int* __restrict__ count, int V, int* __restrict__ offset, int* __restrict__ cursor) {
    __shared__ int s_part[1024];
    const int tid = threadIdx.x, per = (V + 1023) / 1024, b0 = tid * per, b1 = min(V, b0 + per);
    int s = 0;
    for (int v = b0; v < b1; ++v) s += count[v];
    s_part[tid] = s;
    __syncthreads();
    if (tid == 0) { int run = 0; for (int i = 0; i < 1024; ++i) { int t = s_part[i]; s_part[i] = run; run += t; } offset[V] = run; }
    __syncthreads();
    int run = s_part[tid];
    for (int v = b0; v < b1; ++v) { offset[v] = run; cursor[v] = 0; run += count[v]; }
}
__global__ void embedding_place_kernel(const int* __restrict__ tok, int rows, int V, int padding_idx, const int* __restrict__ offset, int* __restrict__ cursor,
                                       int* __restrict__ list) {
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    int v = tok[r];
    if (v >= 0 && v < V && v != padding_idx) list[offset[v] + atomicAdd(&cursor[v], 1)] = r;
}
__global__ __launch_bounds__(256) void embedding_sum_kernel(const float* __restrict__ dY, const int* __restrict__ tok, const int* __restrict__ offset,
                                                            const int* __restrict__ list, float* __restrict__ dE, int rows, int width, int padding_idx) {
    __shared__ int s_list[EMB_LIST];
    const int v = blockIdx.x, tid = threadIdx.x;
    float* out = dE + (long)v * width;
    const int o0 = offset[v], n = offset[v + 1] - o0;
    if (n == 0 || v == padding_idx) { for (int c = tid; c < width; c += 256) out[c] = 0.f; return; }
    if (n > EMB_LIST) {          // very frequent token: ordered compaction by scanning the token array, flushed whenever the
                                 // next 256-token chunk might not fit the list any more
        __shared__ int s_wcnt[4]; __shared__ int s_total;
        const int lane = tid & 63, wave = tid >> 6;
        for (int c = tid; c < width; c += 256) out[c] = 0.f;
        if (tid == 0) s_total = 0;
        __syncthreads();
        for (int base = 0;; base += 256) {           // one extra pass after the last chunk flushes what is left
            const bool last = base >= rows;
            if (last || s_total + 256 > EMB_LIST) {
                const int cnt = s_total;
                for (int c = tid; c < width; c += 256) { float acc = out[c]; for (int i = 0; i < cnt; ++i) acc += dY[(long)s_list[i] * width + c]; out[c] = acc; }
                __syncthreads();
                if (tid == 0) s_total = 0;
                __syncthreads();
                if (last) break;
            }
            const int r = base + tid;
            const bool hit = (r < rows) && (tok[r] == v);
            const unsigned long long mk = __ballot(hit);
            if (lane == 0) s_wcnt[wave] = __popcll(mk);
            __syncthreads();
            int off = s_total;
            for (int w = 0; w < wave; ++w) off += s_wcnt[w];
            const int pos = off + __popcll(mk & ((1ull << lane) - 1ull));
            if (hit) s_list[pos] = r;
            __syncthreads();
            if (tid == 0) s_total += s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
            __syncthreads();
        }
        return;
    }
    // bitonic sort of the segment (padded with INT_MAX to a power of two) in LDS
    int np2 = 1; while (np2 < n) np2 <<= 1;
    for (int i = tid; i < np2; i += 256) s_list[i] = i < n ? list[o0 + i] : 0x7fffffff;
    __syncthreads();
    for (int k = 2; k <= np2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < np2; i += 256) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const int a = s_list[i], b = s_list[ixj];
                    if (((i & k) == 0) ? (a > b) : (a < b)) { s_list[i] = b; s_list[ixj] = a; }
                }
            }
            __syncthreads();
        }
    for (int c = tid; c < width; c += 256) {
        float acc = 0.f;
        for (int i = 0; i < n; ++i) acc += dY[(long)s_list[i] * width + c];
        out[c] = acc;
    }
}

// nn.Embedding(max_norm=...) (model.py:161): rows that are looked up and whose L2 norm exceeds max_norm are rescaled
// in place by max_norm / (norm + 1e-7), as torch.embedding_renorm_ does.  flags marks the looked-up rows first so
// that a row used by several tokens is rescaled exactly once.
__global__ void embedding_mark_kernel(const int* __restrict__ tok, int n, int* __restrict__ flags, int V) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { int t = tok[i]; if (t >= 0 && t < V) flags[t] = 1; }
}
__global__ __launch_bounds__(64) void embedding_renorm_kernel(float* __restrict__ table, int* __restrict__ flags, int width, float max_norm) {
    const int v = blockIdx.x, lane = threadIdx.x;
    if (!flags[v]) return;
    float* row = table + (long)v * width;
    float s = 0.f;
    for (int c = lane; c < width; c += 64) s += row[c] * row[c];
    s = wave_sum(s);
    const float norm = sqrtf(s);
    if (norm > max_norm) { const float sc = max_norm / (norm + 1e-7f); for (int c = lane; c < width; c += 64) row[c] *= sc; }
    if (lane == 0) flags[v] = 0;
}

// out[i] = a[i] + b[i]
__global__ void sigmoid_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dpre, long n) {
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) { const float v = y[e]; dpre[e] = dy[e] * v * (1.f - v); }
}
// g[e] *= 1 - u[e]^2 : backward of tanh from its output
__global__ void mul_dtanh_kernel(float* __restrict__ g, const float* __restrict__ u, long n) {
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) { const float t = u[e]; g[e] *= 1.f - t * t; }
}
__global__ void add_kernel(float* __restrict__ out, const float* __restrict__ a, const float* __restrict__ b, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = a[i] + b[i];
}
// y[r, :] (+)= x[map[r], :]   (map < 0 -> zero contribution)
__global__ void scatter_rows_kernel(const float* __restrict__ src, const int* __restrict__ prow, float* __restrict__ dst, int rows, int width) {
    int r = blockIdx.x;
    if (r >= rows) return;
    int p = prow[r];
    for (int c = threadIdx.x; c < width; c += blockDim.x) dst[(long)r * width + c] = (p >= 0) ? src[(long)p * width + c] : 0.f;
}

}  // namespace sat
