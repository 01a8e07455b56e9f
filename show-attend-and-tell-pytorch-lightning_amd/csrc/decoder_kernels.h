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
__global__ void set4_int_kernel(int* p, int a, int b, int c, int d) { p[0] = a; p[1] = b; p[2] = c; p[3] = d; }
// plain copies / clears as kernels: the batched beam search enqueues nothing but kernel launches, so that a captured stream
// (hipGraph) is one linear chain of kernel nodes (memset / memcpy nodes were seen to run out of order inside a replayed graph)
__global__ void copy_words_kernel(unsigned* __restrict__ dst, const unsigned* __restrict__ src, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}
__global__ void fill_int_kernel(int* p, long n, int v) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---- dropout (nn.Dropout in training mode: model.py:74/78, 117/130, 164/526).  The mask is a counter-based hash of
// (seed, stream, element index): no state, recomputed wherever it is needed (forward, backward), reproducible.
// streams: 0 = InitLSTM mean, 1 = embedding, 2 = DeepOutput.  keep-probability 1-p, kept values scaled by 1/(1-p).
__device__ __forceinline__ float dropout_scale(unsigned long long seed, unsigned stream, unsigned long long idx, float p) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(stream + 1) + idx * 0xD1342543DE82EF95ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const float u = (float)(z >> 40) * (1.0f / 16777216.0f);      // 24 bits -> [0,1)
    return (u >= p) ? 1.0f / (1.0f - p) : 0.f;
}

// dst[r, :] = table[tok[r], :] (embedding gather; tok outside [0, V) -> zeros, the ids the gradient skips), with embedding_dropout when p > 0
__global__ void gather_rows_kernel(const float* __restrict__ table, const int* __restrict__ tok, float* __restrict__ out, int rows, int width, int V,
                                   float p, unsigned long long seed, long row0) {
    int r = blockIdx.x;
    if (r >= rows) return;
    int t = tok[r];
    for (int c = threadIdx.x; c < width; c += blockDim.x) {
        float v = (t >= 0 && t < V) ? table[(long)t * width + c] : 0.f;
        if (p > 0.f) v *= dropout_scale(seed, 1, (unsigned long long)(row0 + r) * width + c, p);
        out[(long)r * width + c] = v;
    }
}
// y[r, c] = x[r, c] * mask(stream, (row0 + r) * width + c)   (in place allowed)
__global__ void dropout_rows_kernel(const float* __restrict__ x, float* __restrict__ y, long total, int width, float p,
                                    unsigned long long seed, unsigned stream, long row0) {
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < total) y[e] = x[e] * dropout_scale(seed, stream, (unsigned long long)row0 * width + e, p);
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
// bf16 operands, and bcat = [0 ; b_beta ; b_ih + b_hh].
__global__ void pack_wcat_kernel(const float* __restrict__ att_dec, const float* __restrict__ beta_w, const float* __restrict__ w_hh,
                                 const float* __restrict__ beta_b, const float* __restrict__ b_ih, const float* __restrict__ b_hh, float* __restrict__ Wcat,
                                 __bf16* __restrict__ Wcat_b, float* __restrict__ bcat, int A, int D, int n) {
    const long HCW = (long)A + D + 4L * n, nw = HCW * n, e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nw) {
        const long r = e / n;
        const float v = r < A ? att_dec[e] : (r < A + D ? beta_w[e - (long)A * n] : w_hh[e - (long)(A + D) * n]);
        Wcat[e] = v;
        if (Wcat_b) Wcat_b[e] = (__bf16)v;
    } else if (e < nw + HCW) {
        const long r = e - nw;
        bcat[r] = r < A ? 0.f : (r < A + D ? beta_b[r - A] : b_ih[r - A - D] + b_hh[r - A - D]);
    }
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
                                                            float p, unsigned long long seed, long row0) {
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
        if (p > 0.f) v *= dropout_scale(seed, 1, (unsigned long long)(row0 + i) * width + c, p);
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
// InitLSTM over the K expanded copies of ONE image's annotation (model.py:265-269), for every image: the raw reshape of
// F3 acts on each image's own (K, 2*layers*n) buffer.  h, c: (layers, B*K, n).
__global__ void init_expand_images_kernel(const float* __restrict__ init_img, float* __restrict__ h0, float* __restrict__ c0, int B, int K, int n,
                                          int layers) {
    const long per = 2L * layers * K * n;                      // flat elements of one image
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= per * B) return;
    const int b = (int)(e / per); const long f = e - (long)b * per;
    const long w2 = 2L * layers * n, slab_sz = (long)K * n;
    const float v = init_img[(long)b * w2 + f % w2];           // every one of the K rows is the image's init vector
    const long slab = f / slab_sz, within = f - slab * slab_sz;
    const long row = within / n, col = within - row * n;
    const long N = (long)B * K;
    if (slab < layers) h0[(slab * N + (long)b * K + row) * n + col] = v;
    else c0[((slab - layers) * N + (long)b * K + row) * n + col] = v;
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
// init_expand_images_kernel for groups: the raw reshape of F3 acts on the (Kg, 2*layers*n) buffer of every (image, group) pair, as it
// does for a beam of Kg rows, so that a group starts exactly like the plain search at beamk = Kg.  Pair p = b * G + g reads image b.
__global__ void init_expand_groups_kernel(const float* __restrict__ init_img, float* __restrict__ h0, float* __restrict__ c0, int B, int G, int Kg, int n,
                                          int layers) {
    const long per = 2L * layers * Kg * n;                     // flat elements of one pair
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= per * B * G) return;
    const int p = (int)(e / per); const long f = e - (long)p * per;
    const long w2 = 2L * layers * n, slab_sz = (long)Kg * n;
    const float v = init_img[(long)(p / G) * w2 + f % w2];
    const long slab = f / slab_sz, within = f - slab * slab_sz;
    const long row = within / n, col = within - row * n;
    const long N = (long)B * G * Kg;
    if (slab < layers) h0[(slab * N + (long)p * Kg + row) * n + col] = v;
    else c0[((slab - layers) * N + (long)p * Kg + row) * n + col] = v;
}
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
