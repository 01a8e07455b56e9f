// Knowledge distillation from an ensemble ("Distillation"; include/sat_hip.h, "distillation loss"):
//   sat_distill_fwd   per packed row: the student's two log-sum-exps (at temperature 1 and tau), every used teacher's log-sum-exp at tau,
//                     the combined teacher distribution q (the ensemble search's combine), KL(q || student at tau), the label-smoothed
//                     cross entropy and the correct-prediction flag; optionally the unscaled gradient in the same launch
//   sat_distill_bwd   the gradient from the logits and the row scratch, or the in-place scale of the gradient the forward wrote
// One 256-thread block per row.  Sweep 1 reads the student's and every used teacher's row once (online log-sum-exps), sweep 2 reads
// them again from the cache (the same block touched them a moment ago) and folds q, log q - s into one online (max, sum, weighted sum)
// triple, so the row normaliser of c never needs a pass of its own; sweep 3, when the gradient is asked for, is the third touch.
// Every sweep issues the loads of U units (a unit: VEC = 4 words of every row read, or 1 on the 4-byte path) before it works on any:
// row_reduce.h's row sweep, widened to the several rows of a unit (load_batch below stands on its load_unit; the recurrences are
// row_reduce.h's as well).  The kernels are compiled for MC = 1, 2, 4, 8 members so that the per-member registers are those of the
// members there are, and U shrinks as MC grows.
#include <math.h>

#include <type_traits>

#include "../../include/sat_hip.h"
#include "common.h"
#include "decoder.h"
#include "row_reduce.h"

namespace sat {
namespace {

struct DistillParams {
    int V, M, geometric;
    float inv_tau, tau, alpha, smoothing, inv_rows;
};
// units in flight per thread and sweep, by the member capacity the kernel is compiled for
template <int MC> struct InFlight { static constexpr int U = MC <= 2 ? 4 : (MC <= 4 ? 2 : 1); };

// U units of the student's row and of every read teacher's, all loads issued before any is used
template <int VEC, int MC, int U>
__device__ __forceinline__ void load_batch(const float* __restrict__ z, const float* const (&t)[MC], const EnsembleArgs& a, int M, bool soft, int u0, int n,
                                           float (&zx)[U][VEC], float (&tx)[MC][U][VEC]) {
#pragma unroll
    for (int k = 0; k < U; ++k) {
        const int u = u0 + 256 * k;
        if (u >= n) continue;
        load_unit<VEC>(z, u, zx[k]);
        if (soft) {
#pragma unroll
            for (int i = 0; i < MC; ++i) if (i < M && a.w[i] != 0.f) load_unit<VEC>(t[i], u, tx[i][k]);
        }
    }
}

// the row's gradient: g[v] = sc * ((1 - alpha) (softmax(z)_v - h_v) + alpha tau (softmax(z inv_tau)_v - q_v)); a target outside [0, V)
// equals no column, so its one-hot is left out
template <int VEC, int MC>
__device__ __forceinline__ void grad_row(const float* __restrict__ z, const float* const (&t)[MC], const EnsembleArgs& a, const float (&tlse)[MC],
                                         const DistillParams& k, float lse1, float lse_tau, float cnorm, int target, float sc, float* __restrict__ g,
                                         int tid) {
    constexpr int U = InFlight<MC>::U;
    const bool hard = k.alpha != 1.f, soft = k.alpha != 0.f;
    const float hc = (1.f - k.alpha) * sc, sc_soft = k.alpha * k.tau * sc;
    const float sv = k.smoothing / (float)k.V, conf = 1.f - k.smoothing;
    const int n = k.V / VEC;
    for (int u0 = tid; u0 < n; u0 += 256 * U) {
        float zx[U][VEC], tx[MC][U][VEC];
        load_batch<VEC, MC, U>(z, t, a, k.M, soft, u0, n, zx, tx);
#pragma unroll
        for (int b = 0; b < U; ++b) {
            const int u = u0 + 256 * b;
            if (u >= n) continue;
            float o[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                float r = 0.f;
                if (hard) r = hc * (__expf(zx[b][j] - lse1) - sv - ((u * VEC + j == target) ? conf : 0.f));
                if (soft) {
                    float x[MC];
#pragma unroll
                    for (int i = 0; i < MC; ++i) x[i] = (i < k.M && a.w[i] != 0.f) ? tx[i][b][j] : 0.f;
                    const float c = ensemble_word<MC>(x, tlse, a, k.M, k.geometric, k.inv_tau);
                    r += sc_soft * (__expf(zx[b][j] * k.inv_tau - lse_tau) - __expf(c - cnorm));
                }
                o[j] = r;
            }
            store_unit<VEC>(g, u, o);
        }
    }
}

// Row p: lse_rows[2p] = logsumexp(z), [2p + 1] = logsumexp(z inv_tau); tlse_rows[p M + i] = logsumexp(t_i inv_tau) (0 for a member of
// weight 0, or when alpha == 0); cnorm_rows[p] = logsumexp(c); loss_rows[2p] = hard, [2p + 1] = soft; correct_rows[p].  A part that
// alpha switches off is written as 0 and its inputs are not read.  dlogits (or NULL): the gradient with gscale = 1.
template <int VEC, int MC>
__global__ __launch_bounds__(256) void distill_rows_kernel(const float* __restrict__ logits, EnsembleArgs a, const int* __restrict__ targets, DistillParams k,
                                                           float* __restrict__ lse_rows, float* __restrict__ tlse_rows, float* __restrict__ cnorm_rows,
                                                           float* __restrict__ loss_rows, int* __restrict__ correct_rows, float* __restrict__ dlogits) {
    constexpr int U = InFlight<MC>::U;
    __shared__ float s_m[MC + 2][4], s_s[MC + 2][4], s_t[4], s_b[4], s_cm[4], s_ca[4], s_cb[4];
    __shared__ int s_i[4];
    const int p = blockIdx.x, tid = threadIdx.x, V = k.V, M = k.M;
    const bool hard = k.alpha != 1.f, soft = k.alpha != 0.f;
    const float* z = logits + (long)p * V;
    const float* t[MC];
#pragma unroll
    for (int i = 0; i < MC; ++i) t[i] = (soft && i < M && a.w[i] != 0.f) ? a.z[i] + (long)p * V : nullptr;
    const int n = V / VEC;

    // sweep 1: the log-sum-exps, the row sum and the argmax
    float mx1 = -INFINITY, sum1 = 0.f, mxt = -INFINITY, sumt = 0.f, tot = 0.f, bv = -INFINITY;
    int bi = 0x7fffffff;
    float tm[MC], ts[MC];
#pragma unroll
    for (int i = 0; i < MC; ++i) { tm[i] = -INFINITY; ts[i] = 0.f; }
    for (int u0 = tid; u0 < n; u0 += 256 * U) {
        float zx[U][VEC], tx[MC][U][VEC];
        load_batch<VEC, MC, U>(z, t, a, M, soft, u0, n, zx, tx);
#pragma unroll
        for (int b = 0; b < U; ++b) {
            const int u = u0 + 256 * b;
            if (u >= n) continue;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {                     // ascending index: the first maximum wins, as torch.argmax
                const float xv = zx[b][j];
                const int v = u * VEC + j;
                if (arg_before(xv, v, bv, bi)) { bv = xv; bi = v; }
                if (hard) tot += xv;
            }
            if (hard) lse_unit<VEC>(zx[b], 1.f, mx1, sum1);
            if (soft) {
                lse_unit<VEC>(zx[b], k.inv_tau, mxt, sumt);
#pragma unroll
                for (int i = 0; i < MC; ++i) if (i < M && a.w[i] != 0.f) lse_unit<VEC>(tx[i][b], k.inv_tau, tm[i], ts[i]);
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
    wave_argbest(bv, bi);
    if ((tid & 63) == 0) { s_t[tid >> 6] = tot; s_b[tid >> 6] = bv; s_i[tid >> 6] = bi; }
    lse_wave_put(mx1, sum1, s_m[MC], s_s[MC], tid);
    lse_wave_put(mxt, sumt, s_m[MC + 1], s_s[MC + 1], tid);
#pragma unroll
    for (int i = 0; i < MC; ++i) if (soft && i < M && a.w[i] != 0.f) lse_wave_put(tm[i], ts[i], s_m[i], s_s[i], tid);
    __syncthreads();
    const float lse1 = hard ? lse_block(s_m[MC], s_s[MC]) : 0.f;
    const float lse_tau = soft ? lse_block(s_m[MC + 1], s_s[MC + 1]) : 0.f;
    float tlse[MC];
#pragma unroll
    for (int i = 0; i < MC; ++i) tlse[i] = (soft && i < M && a.w[i] != 0.f) ? lse_block(s_m[i], s_s[i]) : 0.f;

    // sweep 2: with e_v = exp(c_v - cm), A = sum e_v and B = sum e_v (c_v - s_v):  logsumexp(c) = cm + log A,  KL = B / A - logsumexp(c)
    float cnorm = 0.f, kl = 0.f;
    if (soft) {
        float cm = -INFINITY, ca = 0.f, cb = 0.f;
        for (int u0 = tid; u0 < n; u0 += 256 * U) {
            float zx[U][VEC], tx[MC][U][VEC];
            load_batch<VEC, MC, U>(z, t, a, M, true, u0, n, zx, tx);
#pragma unroll
            for (int b = 0; b < U; ++b) {
                const int u = u0 + 256 * b;
                if (u >= n) continue;
                float c[VEC], d[VEC], m = -INFINITY;
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    float x[MC];
#pragma unroll
                    for (int i = 0; i < MC; ++i) x[i] = (i < M && a.w[i] != 0.f) ? tx[i][b][j] : 0.f;
                    c[j] = ensemble_word<MC>(x, tlse, a, M, k.geometric, k.inv_tau);
                    d[j] = c[j] - (zx[b][j] * k.inv_tau - lse_tau);
                    m = fmaxf(m, c[j]);
                }
                if (m > cm) { const float f = __expf(cm - m); ca *= f; cb = f != 0.f ? cb * f : 0.f; cm = m; }
                if (cm != -INFINITY) {
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        const float e = __expf(c[j] - cm);
                        ca += e;
                        if (e != 0.f) cb += e * d[j];           // q_v == 0 (a -inf or an underflowed word) adds exactly 0, whatever d is
                    }
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float om = __shfl_xor(cm, o, 64), oa = __shfl_xor(ca, o, 64), ob = __shfl_xor(cb, o, 64);
            const float nm = fmaxf(cm, om);
            const float fa = (cm == nm) ? 1.f : __expf(cm - nm), fb = (om == nm) ? 1.f : __expf(om - nm);
            ca = ca * fa + oa * fb;
            cb = (fa != 0.f ? cb * fa : 0.f) + (fb != 0.f ? ob * fb : 0.f);
            cm = nm;
        }
        if ((tid & 63) == 0) { s_cm[tid >> 6] = cm; s_ca[tid >> 6] = ca; s_cb[tid >> 6] = cb; }
        __syncthreads();
        const float Mx = fmaxf(fmaxf(s_cm[0], s_cm[1]), fmaxf(s_cm[2], s_cm[3]));
        float A = 0.f, Bs = 0.f;
        for (int w = 0; w < 4; ++w) {
            const float f = (s_cm[w] == Mx) ? 1.f : __expf(s_cm[w] - Mx);
            A += s_ca[w] * f;
            if (f != 0.f) Bs += s_cb[w] * f;
        }
        cnorm = Mx + __logf(A);
        kl = Bs / A - cnorm;
    }
    const int target = targets[p];
    if (tid == 0) {
        float hl = 0.f;
        if (hard) {
            const float Tt = (s_t[0] + s_t[1]) + (s_t[2] + s_t[3]);
            hl = (target >= 0 && target < V) ? (1.f - k.smoothing) * (lse1 - z[target]) + k.smoothing * (lse1 - Tt / (float)V) : NAN;
        }
        int Bi = bi;
        argbest_merge<4>(bv, Bi, s_b, s_i);
        lse_rows[2 * (long)p] = lse1; lse_rows[2 * (long)p + 1] = lse_tau;
#pragma unroll
        for (int i = 0; i < MC; ++i) if (i < M) tlse_rows[(long)p * M + i] = tlse[i];
        cnorm_rows[p] = cnorm;
        loss_rows[2 * (long)p] = hl; loss_rows[2 * (long)p + 1] = kl;
        correct_rows[p] = (Bi == target) ? 1 : 0;
    }
    // sweep 3
    if (dlogits) grad_row<VEC, MC>(z, t, a, tlse, k, lse1, lse_tau, cnorm, target, k.inv_rows, dlogits + (long)p * V, tid);
}

template <int VEC, int MC>
__global__ __launch_bounds__(256) void distill_grad_kernel(const float* __restrict__ logits, EnsembleArgs a, const int* __restrict__ targets, DistillParams k,
                                                           const float* __restrict__ lse_rows, const float* __restrict__ tlse_rows,
                                                           const float* __restrict__ cnorm_rows, const float* __restrict__ gscale, float* __restrict__ dlogits) {
    const int p = blockIdx.x, V = k.V, M = k.M;
    const bool soft = k.alpha != 0.f;
    const float* t[MC];
    float tlse[MC];
#pragma unroll
    for (int i = 0; i < MC; ++i) {
        const bool used = soft && i < M && a.w[i] != 0.f;
        t[i] = used ? a.z[i] + (long)p * V : nullptr;
        tlse[i] = used ? tlse_rows[(long)p * M + i] : 0.f;
    }
    const float sc = k.inv_rows * (gscale ? gscale[0] : 1.f);
    grad_row<VEC, MC>(logits + (long)p * V, t, a, tlse, k, lse_rows[2 * (long)p], lse_rows[2 * (long)p + 1], cnorm_rows[p], targets[p], sc,
                      dlogits + (long)p * V, threadIdx.x);
}

// dlogits *= gscale[0], in place: the whole array as slabs of 256 units, one per block and trip, each a (one-trip) row sweep
template <int VEC>
__global__ __launch_bounds__(256) void distill_scale_kernel(float* g, long units, const float* __restrict__ gscale) {
    const float s = gscale[0];
    for (long u0 = (long)blockIdx.x * 256; u0 < units; u0 += (long)gridDim.x * 256) {
        float* slab = g + u0 * VEC;
        row_sweep<VEC, 1, 256>(slab, (int)(units - u0 < 256 ? units - u0 : 256), threadIdx.x, [&](int u, const float (&e)[VEC]) {
            float o[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) o[j] = e[j] * s;
            store_unit<VEC>(slab, u, o);
        });
    }
}

// out[1] = mean hard, out[2] = mean soft, out[0] = (1 - alpha) out[1] + alpha tau^2 out[2], out[3] = #correct / P: double, one block,
// fixed-order tree.  A part that alpha switches off enters as exactly 0 (its rows are 0, and 0 * NaN cannot arise: the weight is skipped).
__global__ __launch_bounds__(256) void distill_finish_kernel(const float* __restrict__ loss_rows, const int* __restrict__ correct_rows, int P, float alpha, float tau,
                                                             float* __restrict__ out) {
    __shared__ double s_h[256], s_k[256], s_c[256];
    double h = 0.0, kl = 0.0; int c = 0;
    for (int p = threadIdx.x; p < P; p += 256) { h += (double)loss_rows[2 * (long)p]; kl += (double)loss_rows[2 * (long)p + 1]; c += correct_rows[p]; }
    h = block_tree_sum_d(h, s_h); kl = block_tree_sum_d(kl, s_k);
    const int correct = (int)block_tree_sum_d((double)c, s_c);             // a count: exact in double in any order
    if (threadIdx.x == 0) {
        const double hm = h / (double)P, km = kl / (double)P;
        double total = 0.0;
        if (alpha != 1.f) total += (1.0 - (double)alpha) * hm;
        if (alpha != 0.f) total += (double)alpha * (double)tau * (double)tau * km;
        out[0] = (float)total; out[1] = (float)hm; out[2] = (float)km; out[3] = (float)correct / (float)P;
    }
}

// f(VEC, MC) as integral constants: the access width and the smallest compiled member capacity that holds `members`
template <typename F>
void with_form(bool wide, int members, F&& f) {
    auto by_members = [&](auto vec) {
        if (members <= 1) f(vec, std::integral_constant<int, 1>{});
        else if (members <= 2) f(vec, std::integral_constant<int, 2>{});
        else if (members <= 4) f(vec, std::integral_constant<int, 4>{});
        else f(vec, std::integral_constant<int, SAT_ENSEMBLE_MAX>{});
    };
    with_width(wide, by_members);
}

}  // namespace
}  // namespace sat

using namespace sat;

static int distill_check(const char* what, const float* logits, const float* const* teachers, const float* weights, int32_t members, int32_t combine,
                         const int32_t* targets, int32_t P, int32_t V, float inv_tau, float alpha, float smoothing, const void* lse_rows, const void* tlse_rows,
                         const void* cnorm_rows) {
    if (!logits || !teachers || !weights || !targets || !lse_rows || !tlse_rows || !cnorm_rows) return fail(SAT_EINVAL, "%s: null pointer", what);
    if (P < 1 || V < 1) return fail(SAT_EINVAL, "%s: empty input (P=%d V=%d)", what, P, V);
    SAT_TRY(beam_ensemble_check_weights(weights, members, combine, what));
    for (int i = 0; i < members; ++i)
        if (!teachers[i]) return fail(SAT_EINVAL, "%s: null logits pointer for teacher %d", what, i);
    if (!(inv_tau > 0.f) || !(inv_tau < INFINITY)) return fail(SAT_EINVAL, "%s: inv_tau %g is not a positive finite number", what, (double)inv_tau);
    if (!(alpha >= 0.f && alpha <= 1.f)) return fail(SAT_EINVAL, "%s: alpha %g outside [0, 1]", what, (double)alpha);
    if (!(smoothing >= 0.f && smoothing < 1.f)) return fail(SAT_EINVAL, "%s: smoothing %g outside [0, 1)", what, (double)smoothing);
    return SAT_OK;
}

// 16-byte accesses: V % 4 == 0 and every array a sweep touches starts 16-byte aligned (the teachers only when they are read)
static bool distill_wide(const float* logits, const EnsembleArgs& a, int members, float alpha, int V, const float* dlogits) {
    bool wide = rows_wide(V, logits, dlogits);
    if (alpha != 0.f)
        for (int i = 0; i < members; ++i) if (a.w[i] != 0.f) wide = wide && rows_wide(V, a.z[i]);
    return wide;
}

extern "C" {

int sat_distill_fwd(const float* logits, const float* const* teachers, const float* weights, int32_t members, int32_t combine, const int32_t* targets,
                    int32_t P, int32_t V, float inv_tau, float alpha, float smoothing, float* lse_rows, float* teacher_lse_rows, float* cnorm_rows,
                    float* loss_rows, int32_t* correct_rows, float* out, float* dlogits, void* stream) {
    SAT_TRY(distill_check("distill_fwd", logits, teachers, weights, members, combine, targets, P, V, inv_tau, alpha, smoothing, lse_rows, teacher_lse_rows,
                          cnorm_rows));
    if (!loss_rows || !correct_rows || !out) return fail(SAT_EINVAL, "distill_fwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const EnsembleArgs a = ensemble_args(teachers, weights, members);
    const DistillParams k = {V, members, combine == SAT_ENSEMBLE_GEOMETRIC ? 1 : 0, inv_tau, 1.0f / inv_tau, alpha, smoothing, 1.0f / (float)P};
    with_form(distill_wide(logits, a, members, alpha, V, dlogits), members, [&](auto vec, auto mc) {
        hipLaunchKernelGGL((distill_rows_kernel<decltype(vec)::value, decltype(mc)::value>), dim3(P), dim3(256), 0, st, logits, a, targets, k, lse_rows,
                           teacher_lse_rows, cnorm_rows, loss_rows, correct_rows, dlogits);
    });
    SAT_TRY(launch_ok("distill_rows"));
    hipLaunchKernelGGL(distill_finish_kernel, dim3(1), dim3(256), 0, st, loss_rows, correct_rows, P, alpha, k.tau, out);
    return launch_ok("distill_finish");
}

int sat_distill_bwd(const float* logits, const float* const* teachers, const float* weights, int32_t members, int32_t combine, const int32_t* targets,
                    int32_t P, int32_t V, float inv_tau, float alpha, float smoothing, const float* lse_rows, const float* teacher_lse_rows,
                    const float* cnorm_rows, const float* gscale, int32_t dlogits_from_fwd, float* dlogits, void* stream) {
    SAT_TRY(distill_check("distill_bwd", logits, teachers, weights, members, combine, targets, P, V, inv_tau, alpha, smoothing, lse_rows, teacher_lse_rows,
                          cnorm_rows));
    if (!dlogits) return fail(SAT_EINVAL, "distill_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (dlogits_from_fwd) {                     // the forward wrote the gradient: the scale and nothing more
        if (!gscale) return SAT_OK;
        const long n = (long)P * V;
        with_width(rows_wide(n, dlogits), [&](auto vec) {          // the whole array as one row of P * V words
            const long units = n / decltype(vec)::value, blocks = (units + 255) / 256;
            hipLaunchKernelGGL(distill_scale_kernel<decltype(vec)::value>, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, dlogits, units, gscale);
        });
        return launch_ok("distill_scale");
    }
    const EnsembleArgs a = ensemble_args(teachers, weights, members);
    const DistillParams k = {V, members, combine == SAT_ENSEMBLE_GEOMETRIC ? 1 : 0, inv_tau, 1.0f / inv_tau, alpha, smoothing, 1.0f / (float)P};
    with_form(distill_wide(logits, a, members, alpha, V, dlogits), members, [&](auto vec, auto mc) {
        hipLaunchKernelGGL((distill_grad_kernel<decltype(vec)::value, decltype(mc)::value>), dim3(P), dim3(256), 0, st, logits, a, targets, k, lse_rows,
                           teacher_lse_rows, cnorm_rows, gscale, dlogits);
    });
    return launch_ok("distill_grad");
}

}  // extern "C"
