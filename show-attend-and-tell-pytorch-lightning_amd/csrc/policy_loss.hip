// Self-critical sequence training ("Self-critical training"; include/sat_hip.h, "policy-gradient loss"):
//   sat_policy_nll_fwd / _bwd   row-weighted negative log-likelihood over packed logits, of the distribution the search samples from
//                               (softmax over the unmasked words at the search's temperature)
//   sat_scst_prepare            scores of the sampled captions -> rewards, advantages and the train batch, one launch
#include <math.h>

#include "../../include/sat_hip.h"
#include "common.h"
#include "row_reduce.h"

namespace sat {
namespace {

// the masked ids of one packed row: all four {START, PAD, END, UNK} for the rows of the first decode step, the first two afterwards.
// An id that masks nothing is -1, which no column index equals.
struct RowMask {
    int m0, m1, m2, m3;
    __device__ __forceinline__ bool has(int v) const { return v == m0 || v == m1 || v == m2 || v == m3; }
};
__device__ __forceinline__ RowMask row_mask(const int* __restrict__ masked_ids, bool first) {
    RowMask m;
    m.m0 = masked_ids[0]; m.m1 = masked_ids[1];
    m.m2 = first ? masked_ids[2] : -1; m.m3 = first ? masked_ids[3] : -1;
    return m;
}

// lse_rows[p] = logsumexp over the unmasked v of x[v] = logits[p, v] * inv_temp; logq_rows[p] = x[target] - lse (NaN for a target
// that is out of range or masked).  One block per packed row, row_reduce.h's online log-sum-exp over its row sweep.
template <int VEC>
__global__ __launch_bounds__(256) void policy_rows_kernel(const float* __restrict__ logits, const int* __restrict__ target, int V, float inv_temp,
                                                          const int* __restrict__ masked_ids, int n_first_rows, float* __restrict__ lse_rows,
                                                          float* __restrict__ logq_rows) {
    const int p = blockIdx.x, tid = threadIdx.x;
    const float* x = logits + (long)p * V;
    const RowMask mk = row_mask(masked_ids, p < n_first_rows);
    __shared__ float s_m[4], s_s[4];
    float mx = -INFINITY, sum = 0.f;
    row_sweep<VEC, kSweepDepth<VEC>, 256>(x, V / VEC, tid, [&](int u, const float (&q)[VEC]) {
        float e[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) e[j] = mk.has(u * VEC + j) ? -INFINITY : q[j] * inv_temp;          // a -inf word carries no mass
        lse_unit<VEC>(e, mx, sum);
    });
    lse_wave_put(mx, sum, s_m, s_s, tid);
    __syncthreads();
    if (tid == 0) {
        const float lse = lse_block(s_m, s_s);
        const int t = target[p];
        lse_rows[p] = lse;
        logq_rows[p] = (t >= 0 && t < V && !mk.has(t)) ? x[t] * inv_temp - lse : NAN;
    }
}

// out[0] = -scale * sum_p row_weight[p] * logq_rows[p] over the rows of non-zero weight, in double, one block, fixed-order tree
__global__ __launch_bounds__(256) void policy_finish_kernel(const float* __restrict__ logq_rows, const float* __restrict__ row_weight, int P, float scale,
                                                            float* __restrict__ out) {
    __shared__ double s_l[256];
    double s = 0.0;
    for (int p = threadIdx.x; p < P; p += 256) { const float w = row_weight[p]; if (w != 0.f) s += (double)w * (double)logq_rows[p]; }
    s = block_tree_sum_d(s, s_l);
    if (threadIdx.x == 0) out[0] = (float)(-(double)scale * s);
}

// dlogits[p, v] = g * scale * w_p * inv_temp * (softmax_U(x)[v] - [v == target]) for the unmasked v, 0 for the masked ones; a row of
// weight zero is written as zeros without its logits being read
template <int VEC>
__global__ __launch_bounds__(256) void policy_grad_kernel(const float* __restrict__ logits, const int* __restrict__ target, const float* __restrict__ row_weight,
                                                          const float* __restrict__ lse_rows, int V, float inv_temp, const int* __restrict__ masked_ids,
                                                          int n_first_rows, float scale, const float* __restrict__ gscale, float* __restrict__ dlogits) {
    const int p = blockIdx.x, tid = threadIdx.x;
    const float* x = logits + (long)p * V; float* g = dlogits + (long)p * V;
    // every per-row word is loaded in front of the branch on the weight: one round trip, not one for the weight and one behind it
    const float w = row_weight[p];
    const RowMask mk = row_mask(masked_ids, p < n_first_rows);
    const float lse = lse_rows[p];
    const float sc = (gscale ? gscale[0] : 1.f) * scale * w * inv_temp;
    const int t = target[p];
    if (w == 0.f) {                            // nothing is read, so this is a plain strided loop of stores and no sweep
        const float zero[VEC] = {};
        for (int u = tid; u < V / VEC; u += 256) store_unit<VEC>(g, u, zero);
        return;
    }
    row_sweep<VEC, kSweepDepth<VEC>, 256>(x, V / VEC, tid, [&](int u, const float (&e)[VEC]) {
        float o[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int c = u * VEC + j;
            o[j] = mk.has(c) ? 0.f : (__expf(e[j] * inv_temp - lse) - ((c == t) ? 1.f : 0.f)) * sc;
        }
        store_unit<VEC>(g, u, o);
    });
}

// One block per image: the K sampled captions of image b are rows b * K .. b * K + K - 1.
__global__ __launch_bounds__(256) void scst_prepare_kernel(const int* __restrict__ cap_tokens, const int* __restrict__ cap_len, const double* __restrict__ scores,
                                                           const double* __restrict__ scores_greedy, int K, int S, double w_cider, double w_rouge, int mode,
                                                           int start_id, int pad_id, int end_id, float* __restrict__ reward, float* __restrict__ baseline,
                                                           float* __restrict__ advantage, int* __restrict__ caps, int* __restrict__ lengths,
                                                           float* __restrict__ step_weight, int* __restrict__ count) {
    __shared__ double s_r[SAT_SCST_MAX_SAMPLES];
    __shared__ float s_adv[SAT_SCST_MAX_SAMPLES];
    __shared__ int s_len[SAT_SCST_MAX_SAMPLES];
    const int b = blockIdx.x, tid = threadIdx.x, T = S + 2;
    for (int k = tid; k < K; k += 256) {
        const long n = (long)b * K + k;
        s_r[k] = w_cider * scores[2 * n] + w_rouge * scores[2 * n + 1];
        const int len = cap_len[n];
        s_len[k] = len < 1 ? 1 : (len > S ? S : len);
    }
    __syncthreads();
    for (int k = tid; k < K; k += 256) {
        const long n = (long)b * K + k;
        double base;
        if (mode == SAT_SCST_BASELINE_GREEDY) {
            base = w_cider * scores_greedy[2 * b] + w_rouge * scores_greedy[2 * b + 1];
        } else {                                                   // the other K - 1 samples, ascending
            double s = 0.0;
            for (int j = 0; j < K; ++j) if (j != k) s += s_r[j];
            base = s / (double)(K - 1);
        }
        const float adv = (float)(s_r[k] - base);
        s_adv[k] = adv;
        reward[n] = (float)s_r[k]; advantage[n] = adv;
        if (baseline) baseline[n] = (float)base;
        lengths[n] = s_len[k] + 1;
        count[n] = s_len[k] + (s_len[k] < S ? 1 : 0);
    }
    __syncthreads();
    for (int e = tid; e < K * T; e += 256) {
        const int k = e / T, j = e - k * T, len = s_len[k];
        const long n = (long)b * K + k;
        caps[n * T + j] = j == 0 ? start_id : (j <= len ? cap_tokens[n * (S + 1) + j - 1] : (j == len + 1 ? end_id : pad_id));
        if (j < T - 1)            // step j draws word j + 1; the END step of a cut caption (len == S) was never drawn: weight 0
            step_weight[n * (T - 1) + j] = (j < len || (j == len && len < S)) ? s_adv[k] : 0.f;
    }
}

}  // namespace
}  // namespace sat

using namespace sat;

static int policy_check(const char* what, const void* logits, const void* targets, const void* row_weight, const void* lse_rows, const void* masked_ids,
                        const void* out, int32_t P, int32_t V, float inv_temperature, int32_t n_first_rows, float scale) {
    if (!logits || !targets || !row_weight || !lse_rows || !masked_ids || !out) return fail(SAT_EINVAL, "%s: null pointer", what);
    if (P <= 0 || V <= 0) return fail(SAT_EINVAL, "%s: empty input (P=%d V=%d)", what, P, V);
    if (!(inv_temperature > 0.f) || !(inv_temperature < INFINITY))
        return fail(SAT_EINVAL, "%s: inv_temperature %g is not a positive finite number", what, (double)inv_temperature);
    if (n_first_rows < 0 || n_first_rows > P) return fail(SAT_EINVAL, "%s: n_first_rows %d outside [0, P=%d]", what, n_first_rows, P);
    if (!(fabsf(scale) < INFINITY)) return fail(SAT_EINVAL, "%s: scale %g is not finite", what, (double)scale);
    return SAT_OK;
}

extern "C" {

int sat_policy_nll_fwd(const float* logits, const int32_t* targets, const float* row_weight, int32_t P, int32_t V, float inv_temperature,
                       const int32_t* masked_ids, int32_t n_first_rows, float scale, float* lse_rows, float* logq_rows, float* out, void* stream) {
    SAT_TRY(policy_check("policy_nll_fwd", logits, targets, row_weight, lse_rows, masked_ids, out, P, V, inv_temperature, n_first_rows, scale));
    if (!logq_rows) return fail(SAT_EINVAL, "policy_nll_fwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    with_width(rows_wide(V, logits), [&](auto vec) {
        hipLaunchKernelGGL(policy_rows_kernel<decltype(vec)::value>, dim3(P), dim3(256), 0, st, logits, targets, V, inv_temperature, masked_ids, n_first_rows,
                           lse_rows, logq_rows);
    });
    SAT_TRY(launch_ok("policy_rows"));
    hipLaunchKernelGGL(policy_finish_kernel, dim3(1), dim3(256), 0, st, logq_rows, row_weight, P, scale, out);
    return launch_ok("policy_finish");
}

int sat_policy_nll_bwd(const float* logits, const int32_t* targets, const float* row_weight, const float* lse_rows, int32_t P, int32_t V,
                       float inv_temperature, const int32_t* masked_ids, int32_t n_first_rows, float scale, const float* gscale, float* dlogits,
                       void* stream) {
    SAT_TRY(policy_check("policy_nll_bwd", logits, targets, row_weight, lse_rows, masked_ids, dlogits, P, V, inv_temperature, n_first_rows, scale));
    hipStream_t st = (hipStream_t)stream;
    with_width(rows_wide(V, logits, dlogits), [&](auto vec) {
        hipLaunchKernelGGL(policy_grad_kernel<decltype(vec)::value>, dim3(P), dim3(256), 0, st, logits, targets, row_weight, lse_rows, V, inv_temperature, masked_ids,
                           n_first_rows, scale, gscale, dlogits);
    });
    return launch_ok("policy_grad");
}

int sat_scst_prepare(const int32_t* cap_tokens, const int32_t* cap_len, const double* scores, const double* scores_greedy, int32_t B, int32_t K, int32_t S,
                     double w_cider, double w_rouge, int32_t baseline_mode, const int32_t* special_ids_host, float* reward, float* baseline, float* advantage,
                     int32_t* caps, int32_t* lengths, float* step_weight, int32_t* count, void* stream) {
    if (!cap_tokens || !cap_len || !scores || !special_ids_host || !reward || !advantage || !caps || !lengths || !step_weight || !count)
        return fail(SAT_EINVAL, "scst_prepare: null pointer");
    if (B < 1 || K < 1 || S < 1) return fail(SAT_EINVAL, "scst_prepare: non-positive size (B=%d K=%d S=%d)", B, K, S);
    if (K > SAT_SCST_MAX_SAMPLES || S + 1 > SAT_CAPTION_MAX_LEN)
        return fail(SAT_EINVAL, "scst_prepare: over the limits (K=%d <= %d, S + 1=%d <= %d)", K, SAT_SCST_MAX_SAMPLES, S + 1, SAT_CAPTION_MAX_LEN);
    if (baseline_mode != SAT_SCST_BASELINE_GREEDY && baseline_mode != SAT_SCST_BASELINE_MEAN)
        return fail(SAT_EINVAL, "scst_prepare: baseline mode %d (0 = greedy, 1 = mean of the other samples)", baseline_mode);
    if (baseline_mode == SAT_SCST_BASELINE_GREEDY && !scores_greedy) return fail(SAT_EINVAL, "scst_prepare: the greedy baseline needs scores_greedy (null pointer)");
    if (baseline_mode == SAT_SCST_BASELINE_MEAN && K < 2) return fail(SAT_EINVAL, "scst_prepare: the mean baseline needs K >= 2 samples per image (K=%d)", K);
    if (!(fabs(w_cider) <= 1.79769313486231570815e308) || !(fabs(w_rouge) <= 1.79769313486231570815e308))
        return fail(SAT_EINVAL, "scst_prepare: reward weights (%g, %g) are not finite", w_cider, w_rouge);
    hipLaunchKernelGGL(scst_prepare_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, cap_tokens, cap_len, scores, scores_greedy, K, S, w_cider, w_rouge,
                       baseline_mode, special_ids_host[0], special_ids_host[1], special_ids_host[2], reward, baseline, advantage, caps, lengths, step_weight,
                       count);
    return launch_ok("scst_prepare");
}

}  // extern "C"
