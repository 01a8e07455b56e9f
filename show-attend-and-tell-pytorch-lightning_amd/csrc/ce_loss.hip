// The two losses of the train step (include/sat_hip.h: sat_ce_label_smooth_fwd / _bwd, sat_doubly_stochastic_fwd / _bwd):
//   ce_fwd / ce_bwd   label-smoothed cross entropy over packed logits rows (util.py:105-112) with the row argmax (accuracy, model.py:596-597)
//   ds_fwd / ds_bwd   the doubly-stochastic attention term (model.py:594)
// Nothing in the decoder's time loop calls them; api.hip does, through decoder.h.
#include <math.h>

#include "../../include/sat_hip.h"
#include "common.h"
#include "decoder.h"
#include "ce_row.h"
#include "row_reduce.h"

namespace sat {

// One block per packed token row, one sweep (ce_row.h, on row_reduce.h): online log-sum-exp, row argmax and the row loss; ce_finish_kernel
// reduces loss_rows in a fixed order.  The gradient is a second kernel so that autograd's grad_output scales it.
template <int VEC>
__global__ __launch_bounds__(256) void ce_rows_kernel(const float* __restrict__ logits, const int* __restrict__ target, int V,
                                                      float smoothing, float* __restrict__ lse_rows,
                                                      float* __restrict__ loss_rows, int* __restrict__ correct_rows) {
    const int p = blockIdx.x, tid = threadIdx.x;
    const float* x = logits + (long)p * V;
    __shared__ CeRowLds lds;
    float bv; int bi;
    ce_row_sweep<VEC>(x, V, tid, lds, bv, bi);
    if (tid == 0) {
        const float lse = ce_row_lse(lds);
        const int t = target[p];
        lse_rows[p] = lse;
        loss_rows[p] = ce_row_loss(lse, x[t], ce_row_total(lds), V, smoothing);
        correct_rows[p] = (ce_row_argmax(lds, bv, bi) == t) ? 1 : 0;
    }
}
// dlogits[p, v] = g/P * (softmax - smoothing/V - (1-smoothing)[v == target])
template <int VEC>
__global__ __launch_bounds__(256) void ce_grad_kernel(const float* __restrict__ logits, const int* __restrict__ target, const float* __restrict__ lse_rows,
                                                      int V, float smoothing, float inv_rows, const float* __restrict__ gscale, float* __restrict__ dlogits) {
    const int p = blockIdx.x;
    const float* x = logits + (long)p * V; float* g = dlogits + (long)p * V;
    const float lse = lse_rows[p], sv = smoothing / (float)V, conf = 1.f - smoothing;
    const float sc = inv_rows * (gscale ? gscale[0] : 1.f);
    const int t = target[p];
    row_sweep<VEC, kSweepDepth<VEC>, 256>(x, V / VEC, threadIdx.x, [&](int u, const float (&e)[VEC]) {
        float o[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = ce_grad_word(e[j], lse, sv, conf, u * VEC + j == t, sc);
        store_unit<VEC>(g, u, o);
    });
}

// out[0] = mean(loss_rows), out[1] = #correct / P   (single block, fixed-order tree)
__global__ void ce_finish_kernel(const float* __restrict__ loss_rows, const int* __restrict__ correct_rows, int P, float* __restrict__ out) {
    __shared__ double s_l[256], s_c[256];
    double s = 0.0; int c = 0;
    for (int p = threadIdx.x; p < P; p += 256) { s += (double)loss_rows[p]; c += correct_rows[p]; }
    s = block_tree_sum_d(s, s_l);
    const int correct = (int)block_tree_sum_d((double)c, s_c);             // a count: exact in double in any order
    if (threadIdx.x == 0) { out[0] = (float)(s / (double)P); out[1] = (float)correct / (float)P; }
}

// Doubly-stochastic term.  asum[i,l] = sum_t alphas[i,t,l]; part[block] = sum (1-asum)^2
__global__ void ds_rows_kernel(const float* __restrict__ alphas, float* __restrict__ asum, float* __restrict__ part, int N, int T1, int L) {
    __shared__ float s_p[256];
    long e = (long)blockIdx.x * 256 + threadIdx.x;
    float v = 0.f;
    if (e < (long)N * L) {
        long i = e / L; int l = (int)(e % L);
        float s = 0.f;
        for (int t = 0; t < T1; ++t) s += alphas[(i * T1 + t) * L + l];
        asum[e] = s;
        v = (1.f - s) * (1.f - s);
    }
    s_p[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) s_p[threadIdx.x] += s_p[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) part[blockIdx.x] = s_p[0];
}
__global__ void ds_finish_kernel(const float* __restrict__ part, int nparts, float gamma, long count, float* __restrict__ out) {
    __shared__ double s_p[256];
    double s = 0.0;
    for (int p = threadIdx.x; p < nparts; p += 256) s += (double)part[p];
    s = block_tree_sum_d(s, s_p);
    if (threadIdx.x == 0) out[0] = gamma * (float)(s / (double)count);
}
// dalphas[i,t,l] = gscale[0] * gamma * 2 (asum[i,l] - 1) / (N L)   for every t
__global__ void ds_grad_kernel(const float* __restrict__ asum, const float* __restrict__ gscale, float gamma, float* __restrict__ dalphas, int N, int T1, int L) {
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)N * T1 * L) return;
    long i = e / ((long)T1 * L); int l = (int)(e % L);
    float g = gscale ? gscale[0] : 1.f;
    dalphas[e] = g * gamma * 2.f * (asum[i * L + l] - 1.f) / (float)((long)N * L);
}

int ce_fwd(const float* logits, const int* targets, int P, int V, float smoothing, float* lse_rows, float* loss_rows, int* correct_rows, float* out, hipStream_t st) {
    SAT_REQUIRE(P > 0 && V > 0, "ce_fwd: empty input (P=%d V=%d)", P, V);
    SAT_REQUIRE(smoothing >= 0.f && smoothing < 1.f, "ce_fwd: smoothing %g out of range", smoothing);
    with_width(rows_wide(V, logits), [&](auto vec) {
        hipLaunchKernelGGL(ce_rows_kernel<decltype(vec)::value>, dim3(P), dim3(256), 0, st, logits, targets, V, smoothing, lse_rows, loss_rows, correct_rows);
    });
    SAT_TRY(launch_ok("ce_rows"));
    hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(256), 0, st, loss_rows, correct_rows, P, out);
    return launch_ok("ce_finish");
}
int ce_bwd(const float* logits, const int* targets, const float* lse_rows, int P, int V, float smoothing, const float* gscale, float* dlogits, hipStream_t st) {
    SAT_REQUIRE(P > 0 && V > 0, "ce_bwd: empty input");
    with_width(rows_wide(V, logits, dlogits), [&](auto vec) {
        hipLaunchKernelGGL(ce_grad_kernel<decltype(vec)::value>, dim3(P), dim3(256), 0, st, logits, targets, lse_rows, V, smoothing, 1.0f / (float)P, gscale, dlogits);
    });
    return launch_ok("ce_grad");
}
int ds_fwd(const float* alphas, int N, int T1, int L, float gamma, float* asum, float* part, float* out, hipStream_t st) {
    SAT_REQUIRE(N > 0 && T1 > 0 && L > 0, "ds_fwd: empty input");
    const int nb = cdiv((long)N * L, 256);
    hipLaunchKernelGGL(ds_rows_kernel, dim3(nb), dim3(256), 0, st, alphas, asum, part, N, T1, L);
    SAT_TRY(launch_ok("ds_rows"));
    hipLaunchKernelGGL(ds_finish_kernel, dim3(1), dim3(256), 0, st, part, nb, gamma, (long)N * L, out);
    return launch_ok("ds_finish");
}
int ds_bwd(const float* asum, const float* gscale, int N, int T1, int L, float gamma, float* dalphas, hipStream_t st) {
    hipLaunchKernelGGL(ds_grad_kernel, dim3(cdiv((long)N * T1 * L, 256)), dim3(256), 0, st, asum, gscale, gamma, dalphas, N, T1, L);
    return launch_ok("ds_grad");
}

}  // namespace sat
