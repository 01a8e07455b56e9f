// The token losses of the train step beside the label-smoothed cross entropy ("Token losses"; include/sat_hip.h, "token
// losses"): focal loss (Lin et al. 2017) on the next-word distribution and token-level unlikelihood (Welleck et al. 2019) against the
// words the ground-truth caption has already said.
//   sat_token_loss_fwd   per packed row: the sweep of ce_rows_kernel (ce_row.h: log-sum-exp, sum of the logits, argmax), then the row's
//                        distinct negative candidates found in LDS and their logits gathered; the row terms ce, fl, ul, mass and the
//                        two numbers the gradient needs (w, R); a finish kernel sums the rows in double in a fixed order
//   sat_token_loss_bwd   one sweep writes the dense part (softmax times a per-row coefficient, plus the smoothing constant); behind a
//                        block barrier the target's entry and every candidate's are written whole, each by one thread, from x_v
// One 256-thread block per row, a candidate per thread (T - 1 <= 256).  The sweep never asks whether a word is a candidate.  With the
// cross entropy alone (ce_weight 1, the others 0) the forward is ce_row.h's core and nothing else, the backward is ce_grad_kernel.
#include <math.h>

#include "../../include/sat_hip.h"
#include "ce_row.h"
#include "common.h"
#include "decoder.h"
#include "row_reduce.h"

namespace sat {
namespace {

constexpr int kMaxContext = 256;                // ids of one row's context: one per thread
constexpr float kUlClamp = 1e-5f;               // log(max(1 - p_c, clamp)): fairseq's unlikelihood clamp

struct TokenLossParams {
    int V, N, T, pad_id;
    float smoothing, cw, fw, gamma, ua, inv_rows;
};

// The row's context and this thread's candidate.  Row p stands for step t of caption i (src = t * N + i): its context is
// context[i][1 .. t], the targets of the steps before it.  Thread k < t owns context id k: context_id loads it (the kernels call it in
// front of their sweep, so that the two dependent loads are behind them when the sweep ends) ...
struct ContextId { int t, id; };                // t: the number of context ids (-1: src outside [0, (T - 1) N), nothing was read)
__device__ __forceinline__ ContextId context_id(const int* __restrict__ context, const int* __restrict__ src_row, const TokenLossParams& k, int p, int tid) {
    const int src = src_row[p];
    if (src < 0 || src >= (k.T - 1) * k.N) return {-1, -1};
    const int t = src / k.N, i = src - t * k.N;
    return {t, tid < t ? context[(long)i * k.T + 1 + tid] : -1};
}
// ... and row_candidate keeps it when it is a word of the vocabulary, neither the target nor the pad word, and no earlier context id
// equals it (every distinct id is kept exactly once).  Returns the id, or -1.  One barrier; every thread of the block calls it.
__device__ __forceinline__ int row_candidate(const ContextId& c, const TokenLossParams& k, int y, int tid, int* s_id) {
    if (tid < c.t) s_id[tid] = c.id;
    __syncthreads();
    const int id = c.id;
    bool keep = tid < c.t && id >= 0 && id < k.V && id != y && id != k.pad_id;
    for (int j = 0; j < c.t; ++j) keep = keep && !(j < tid && s_id[j] == id);          // a block-uniform trip count: broadcast reads, no early exit to wait for
    return keep ? id : -1;
}

// a, b, c summed over the block in a fixed order (wave butterflies, then the four waves in order); every thread gets the sums
__device__ __forceinline__ void block_sum3(float& a, float& b, float& c, float (*s)[4], int tid) {
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); c += __shfl_xor(c, o, 64); }
    if ((tid & 63) == 0) { s[0][tid >> 6] = a; s[1][tid >> 6] = b; s[2][tid >> 6] = c; }
    __syncthreads();
    a = (s[0][0] + s[0][1]) + (s[0][2] + s[0][3]);
    b = (s[1][0] + s[1][1]) + (s[1][2] + s[1][3]);
    c = (s[2][0] + s[2][1]) + (s[2][2] + s[2][3]);
}

// Row p: lse_rows[p]; aux_rows[2p] = w (the focal rescale of softmax - onehot), [2p + 1] = R (the sum of p_c / (1 - p_c) over the
// candidates the clamp lets through); loss_rows[4p ..] = ce, fl, ul, mass; correct_rows[p].  A term whose weight is 0 is written as 0
// and nothing is read for it.
template <int VEC>
__global__ __launch_bounds__(256) void token_rows_kernel(const float* __restrict__ logits, const int* __restrict__ targets, const int* __restrict__ context,
                                                         const int* __restrict__ src_row, TokenLossParams k, float* __restrict__ lse_rows,
                                                         float* __restrict__ aux_rows, float* __restrict__ loss_rows, int* __restrict__ correct_rows) {
    const int p = blockIdx.x, tid = threadIdx.x, V = k.V;
    const float* x = logits + (long)p * V;
    __shared__ CeRowLds lds;
    __shared__ int s_id[kMaxContext];
    __shared__ float s_sum[3][4];
    float bv; int bi;
    const int y = targets[p];
    const bool y_ok = y >= 0 && y < V;
    ContextId ctx = {0, -1};
    if (k.ua != 0.f) ctx = context_id(context, src_row, k, p, tid);
    ce_row_sweep<VEC>(x, V, tid, lds, bv, bi);
    const float lse = ce_row_lse(lds);

    float ul = 0.f, mass = 0.f, R = 0.f;
    if (k.ua != 0.f) {
        if (ctx.t < 0) {
            ul = mass = R = NAN;
        } else if (ctx.t > 0) {
            const int c = row_candidate(ctx, k, y, tid, s_id);
            if (c >= 0) {
                const float d = x[c] - lse;
                const float pc = expf(d), om = -expm1f(d);                  // 1 - p_c without the cancellation of 1 - exp(d)
                mass = pc;
                ul = -logf(fmaxf(om, kUlClamp));
                R = om >= kUlClamp ? pc / om : 0.f;                         // the clamp passes no gradient
            }
            block_sum3(ul, mass, R, s_sum, tid);
        }
    }
    if (tid != 0) return;
    const float xy = y_ok ? x[y] : NAN;
    float ce = 0.f, fl = 0.f, w = 0.f;
    if (k.cw != 0.f) ce = y_ok ? ce_row_loss(lse, xy, ce_row_total(lds), V, k.smoothing) : NAN;
    if (k.fw != 0.f) {
        const float nll = lse - xy, logq = -nll;
        const float q = expf(logq), om = -expm1f(logq);                     // om = 1 - q
        if (k.gamma == 0.f) { fl = nll; w = 1.f; }
        else if (om <= 0.f) { fl = 0.f; w = 0.f; }                          // q == 1: (1 - q)^gamma and its slope times log q vanish together
        else {
            const float pw = powf(om, k.gamma);
            fl = pw * nll;
            w = pw - k.gamma * q * (pw / om) * logq;
        }
        if (!y_ok) fl = w = NAN;
    }
    lse_rows[p] = lse;
    aux_rows[2 * (long)p] = w; aux_rows[2 * (long)p + 1] = R;
    float* lr = loss_rows + 4 * (long)p;
    lr[0] = ce; lr[1] = fl; lr[2] = ul; lr[3] = mass;
    correct_rows[p] = (ce_row_argmax(lds, bv, bi) == y) ? 1 : 0;
}

// out[0] = ce_weight mean ce + focal_weight mean fl + ul_alpha mean ul (a weight of 0 skips its term), out[1] = #correct / P,
// out[2..5] = the means of ce, fl, ul, mass: double, one block, the fixed-order tree of ce_finish_kernel
__global__ __launch_bounds__(256) void token_finish_kernel(const float* __restrict__ loss_rows, const int* __restrict__ correct_rows, int P, float cw, float fw,
                                                           float ua, float* __restrict__ out) {
    __shared__ double s_a[256], s_c[256];
    double s[4] = {0.0, 0.0, 0.0, 0.0}; int c = 0;
    for (int p = threadIdx.x; p < P; p += 256) {
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] += (double)loss_rows[4 * (long)p + j];
        c += correct_rows[p];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { s[j] = block_tree_sum_d(s[j], s_a); __syncthreads(); }
    const int correct = (int)block_tree_sum_d((double)c, s_c);             // a count: exact in double in any order
    if (threadIdx.x == 0) {
        double total = 0.0;
        if (cw != 0.f) total += (double)cw * (s[0] / (double)P);
        if (fw != 0.f) total += (double)fw * (s[1] / (double)P);
        if (ua != 0.f) total += (double)ua * (s[2] / (double)P);
        out[0] = (float)total; out[1] = (float)correct / (float)P;
#pragma unroll
        for (int j = 0; j < 4; ++j) out[2 + j] = (float)(s[j] / (double)P);
    }
}

// dlogits[p][v] = sc * (p_v A - ce_weight smoothing/V - (ce_weight (1 - smoothing) + focal_weight w) [v == y] + ul_alpha r_v [v in C_p])
// with A = ce_weight + focal_weight w - ul_alpha R.  The sweep writes sc * (p_v A - B) everywhere; behind the barrier thread 0 writes the
// target's entry and each candidate's thread its own, every one computed whole from x_v.
template <int VEC>
__global__ __launch_bounds__(256) void token_grad_kernel(const float* __restrict__ logits, const int* __restrict__ targets, const int* __restrict__ context,
                                                         const int* __restrict__ src_row, TokenLossParams k, const float* __restrict__ lse_rows,
                                                         const float* __restrict__ aux_rows, const float* __restrict__ gscale, float* __restrict__ dlogits) {
    const int p = blockIdx.x, tid = threadIdx.x, V = k.V;
    const float* x = logits + (long)p * V; float* g = dlogits + (long)p * V;
    __shared__ int s_id[kMaxContext];
    const float lse = lse_rows[p], w = aux_rows[2 * (long)p], R = aux_rows[2 * (long)p + 1];
    const float sc = k.inv_rows * (gscale ? gscale[0] : 1.f);
    float A = 0.f, B = 0.f, hot = 0.f;
    if (k.cw != 0.f) { A += k.cw; B = k.cw * (k.smoothing / (float)V); hot += k.cw * (1.f - k.smoothing); }
    if (k.fw != 0.f) { A += k.fw * w; hot += k.fw * w; }
    if (k.ua != 0.f) A -= k.ua * R;
    const int y = targets[p];
    ContextId ctx = {0, -1};
    if (k.ua != 0.f) ctx = context_id(context, src_row, k, p, tid);
    row_sweep<VEC, kSweepDepth<VEC>, 256>(x, V / VEC, tid, [&](int u, const float (&e)[VEC]) {
        float o[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = (__expf(e[j] - lse) * A - B) * sc;
        store_unit<VEC>(g, u, o);
    });
    const int c = row_candidate(ctx, k, y, tid, s_id);                      // its barrier: the sweep's stores of this row are behind us
    if (tid == 0 && y >= 0 && y < V) g[y] = (__expf(x[y] - lse) * A - B - hot) * sc;
    if (c < 0) return;
    const float d = x[c] - lse;
    const float pc = expf(d), om = -expm1f(d);
    const float r = om >= kUlClamp ? pc / om : 0.f;
    g[c] = (__expf(d) * A - B + k.ua * r) * sc;
}

int token_check(const char* what, const float* logits, const int32_t* targets, int32_t P, int32_t V, float smoothing, float cw, float fw, float gamma, float ua,
                const int32_t* context, const int32_t* src_row, int32_t N, int32_t T, const void* lse_rows, const void* aux_rows) {
    if (!logits || !targets || !lse_rows || !aux_rows) return fail(SAT_EINVAL, "%s: null pointer", what);
    if (P < 1 || V < 1) return fail(SAT_EINVAL, "%s: empty input (P=%d V=%d)", what, P, V);
    if (!(smoothing >= 0.f && smoothing < 1.f)) return fail(SAT_EINVAL, "%s: smoothing %g outside [0, 1)", what, (double)smoothing);
    const float vals[4] = {cw, fw, gamma, ua};
    const char* names[4] = {"ce_weight", "focal_weight", "focal_gamma", "ul_alpha"};
    for (int i = 0; i < 4; ++i)
        if (!(vals[i] >= 0.f) || !(vals[i] < INFINITY)) return fail(SAT_EINVAL, "%s: %s %g is not a finite number >= 0", what, names[i], (double)vals[i]);
    if (cw == 0.f && fw == 0.f && ua == 0.f) return fail(SAT_EINVAL, "%s: ce_weight, focal_weight and ul_alpha are all zero", what);
    if (ua != 0.f) {
        if (!context || !src_row) return fail(SAT_EINVAL, "%s: null pointer (%s) with ul_alpha != 0", what, !context ? "context" : "src_row");
        if (N < 1 || T < 2) return fail(SAT_EINVAL, "%s: context of N=%d captions, T=%d words (N >= 1, T >= 2)", what, N, T);
        if (T - 1 > kMaxContext) return fail(SAT_EINVAL, "%s: T - 1 = %d context ids in a row (at most %d: one per thread)", what, T - 1, kMaxContext);
    }
    return SAT_OK;
}

}  // namespace
}  // namespace sat

using namespace sat;

extern "C" {

int sat_token_loss_fwd(const float* logits, const int32_t* targets, int32_t P, int32_t V, float smoothing, float ce_weight, float focal_weight,
                       float focal_gamma, float ul_alpha, const int32_t* context, const int32_t* src_row, int32_t N, int32_t T, int32_t pad_id, float* lse_rows,
                       float* aux_rows, float* loss_rows, int32_t* correct_rows, float* out, void* stream) {
    SAT_TRY(token_check("token_loss_fwd", logits, targets, P, V, smoothing, ce_weight, focal_weight, focal_gamma, ul_alpha, context, src_row, N, T, lse_rows,
                        aux_rows));
    if (!loss_rows || !correct_rows || !out) return fail(SAT_EINVAL, "token_loss_fwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const TokenLossParams k = {V, N, T, pad_id, smoothing, ce_weight, focal_weight, focal_gamma, ul_alpha, 1.0f / (float)P};
    with_width(rows_wide(V, logits), [&](auto vec) {
        hipLaunchKernelGGL(token_rows_kernel<decltype(vec)::value>, dim3(P), dim3(256), 0, st, logits, targets, context, src_row, k, lse_rows, aux_rows,
                           loss_rows, correct_rows);
    });
    SAT_TRY(launch_ok("token_rows"));
    hipLaunchKernelGGL(token_finish_kernel, dim3(1), dim3(256), 0, st, loss_rows, correct_rows, P, ce_weight, focal_weight, ul_alpha, out);
    return launch_ok("token_finish");
}

int sat_token_loss_bwd(const float* logits, const int32_t* targets, int32_t P, int32_t V, float smoothing, float ce_weight, float focal_weight,
                       float focal_gamma, float ul_alpha, const int32_t* context, const int32_t* src_row, int32_t N, int32_t T, int32_t pad_id,
                       const float* lse_rows, const float* aux_rows, const float* gscale, float* dlogits, void* stream) {
    SAT_TRY(token_check("token_loss_bwd", logits, targets, P, V, smoothing, ce_weight, focal_weight, focal_gamma, ul_alpha, context, src_row, N, T, lse_rows,
                        aux_rows));
    if (!dlogits) return fail(SAT_EINVAL, "token_loss_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (ce_weight == 1.f && focal_weight == 0.f && ul_alpha == 0.f)         // the cross entropy alone: its own gradient kernel
        return ce_bwd(logits, targets, lse_rows, P, V, smoothing, gscale, dlogits, st);
    const TokenLossParams k = {V, N, T, pad_id, smoothing, ce_weight, focal_weight, focal_gamma, ul_alpha, 1.0f / (float)P};
    with_width(rows_wide(V, logits, dlogits), [&](auto vec) {
        hipLaunchKernelGGL(token_grad_kernel<decltype(vec)::value>, dim3(P), dim3(256), 0, st, logits, targets, context, src_row, k, lse_rows, aux_rows, gscale,
                           dlogits);
    });
    return launch_ok("token_grad");
}

}  // extern "C"
