// Activation regularisation of the train step (include/sat_hip.h: sat_activation_reg_fwd / _bwd; DESIGN.md 5, "Activation regularisation"):
//   ar  = 1/(P n) sum over live (t, i) of |h[t][i]|^2                 (Merity et al.: alpha * h.pow(2).mean())
//   tar = 1/(Q n) sum over live (t, i), t >= 1, of |h[t][i] - h[t-1][i]|^2     (beta * (h[1:] - h[:-1]).pow(2).mean())
// over the top-layer hidden states hidden (T1, N, n), time-major; row (t, i) is live when t < lengths[i].  A row that is not live is
// never loaded (it may hold anything) and never written.  Nothing in the decoder's time loop calls these; decoder_bwd adds the
// gradient into dHout once, in front of the loop.
#include <math.h>

#include "../../include/sat_hip.h"
#include "common.h"
#include "decoder.h"
#include "row_reduce.h"

namespace sat {

constexpr int kRegRowsPerBlock = 4;             // one wave per row, four waves per block
static int reg_blocks(long rows) { return (int)cdiv(rows, (long)kRegRowsPerBlock); }

// the wave's row and its caption's length (clamped to T1: a length past the buffer must not become an address); false: nothing to do
__device__ __forceinline__ bool reg_row(const int* __restrict__ lengths, int N, int T1, long& r, int& t, int& len) {
    r = (long)blockIdx.x * kRegRowsPerBlock + (threadIdx.x >> 6);
    if (r >= (long)N * T1) return false;
    t = (int)(r / N);
    len = min(lengths[r - (long)t * N], T1);
    return t < len;
}

// part[2 * block] = sum h^2, part[2 * block + 1] = sum (h_t - h_{t-1})^2 over the block's four rows: squares and differences in fp32,
// sums in double, the block's 256 partials through the fixed-order tree
template <int VEC>
__global__ __launch_bounds__(256) void activation_reg_partial_kernel(const float* __restrict__ hidden, const int* __restrict__ lengths, int N, int T1, int n,
                                                                     double* __restrict__ part) {
    __shared__ double s_a[256], s_b[256];
    double sa = 0.0, sb = 0.0;
    long r; int t, len;
    if (reg_row(lengths, N, T1, r, t, len)) {
        const float* x = hidden + r * n;
        const float* xp = x - (long)N * n;          // row (t - 1, i): read when t >= 1 only
        const bool has_prev = t >= 1;
        // row_sweep's loop over two rows at once: the loads of both rows' units go out before the arithmetic (with the sums captured
        // by a sweep body the 4-byte form kept them in scratch)
        constexpr int U = kSweepDepth<VEC>;
        const int units = n / VEC;
        for (int u0 = threadIdx.x & 63; u0 < units; u0 += 64 * U) {
            float e[U][VEC], p[U][VEC];
#pragma unroll
            for (int k = 0; k < U; ++k) if (u0 + 64 * k < units) { load_unit<VEC>(x, u0 + 64 * k, e[k]); if (has_prev) load_unit<VEC>(xp, u0 + 64 * k, p[k]); }
#pragma unroll
            for (int k = 0; k < U; ++k) if (u0 + 64 * k < units) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    sa += (double)(e[k][j] * e[k][j]);
                    if (has_prev) { const float dlt = e[k][j] - p[k][j]; sb += (double)(dlt * dlt); }
                }
            }
        }
    }
    sa = block_tree_sum_d(sa, s_a);
    sb = block_tree_sum_d(sb, s_b);
    if (threadIdx.x == 0) { part[2 * (long)blockIdx.x] = sa; part[2 * (long)blockIdx.x + 1] = sb; }
}

// out[0] = ar, out[1] = tar (single block, fixed-order tree); an empty denominator gives 0
__global__ void activation_reg_finish_kernel(const double* __restrict__ part, int nparts, double inv_pn, double inv_qn, float* __restrict__ out) {
    __shared__ double s_a[256], s_b[256];
    double sa = 0.0, sb = 0.0;
    for (int p = threadIdx.x; p < nparts; p += 256) { sa += part[2 * (long)p]; sb += part[2 * (long)p + 1]; }
    sa = block_tree_sum_d(sa, s_a);
    sb = block_tree_sum_d(sb, s_b);
    if (threadIdx.x == 0) { out[0] = inv_pn > 0.0 ? (float)(sa * inv_pn) : 0.f; out[1] = inv_qn > 0.0 ? (float)(sb * inv_qn) : 0.f; }
}

// dH[t][i] += a h_t + b ((h_t - h_{t-1}) [t >= 1] - (h_{t+1} - h_t) [t + 1 < len_i]) on live rows, a = gscale[0] * ca, b = gscale[1] * cb.
// A term that is off is not computed: its row is not loaded.
template <int VEC>
__global__ __launch_bounds__(256) void activation_reg_bwd_kernel(const float* __restrict__ hidden, const int* __restrict__ lengths, int N, int T1, int n,
                                                                 double ca, double cb, const float* __restrict__ gscale, float* __restrict__ dH) {
    long r; int t, len;
    if (!reg_row(lengths, N, T1, r, t, len)) return;
    const float a = (float)((double)gscale[0] * ca), b = (float)((double)gscale[1] * cb);
    const float* x = hidden + r * n;
    const float* xp = x - (long)N * n;
    const float* xn = x + (long)N * n;
    float* g = dH + r * n;
    const bool has_prev = t >= 1, has_next = t + 1 < len;
    row_sweep<VEC, kSweepDepth<VEC>, 64>(x, n / VEC, threadIdx.x & 63, [&](int u, const float (&e)[VEC]) {
        float p[VEC], q[VEC], o[VEC];
        load_unit<VEC>(g, u, o);
        if (has_prev) load_unit<VEC>(xp, u, p);
        if (has_next) load_unit<VEC>(xn, u, q);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            float v = a * e[j];
            if (has_prev && has_next) v += b * ((e[j] - p[j]) - (q[j] - e[j]));
            else if (has_prev) v += b * (e[j] - p[j]);
            else if (has_next) v -= b * (q[j] - e[j]);
            o[j] += v;
        }
        store_unit<VEC>(g, u, o);
    });
}

size_t activation_reg_scratch_bytes(int N, int T1, int n) { return (size_t)reg_blocks((long)N * T1) * 2 * sizeof(double); }

int activation_reg_fwd(const float* hidden, const int* lengths, int N, int T1, int n, long P, long Q, void* scratch, float* out, hipStream_t st) {
    SAT_REQUIRE(N > 0 && T1 > 0 && n > 0, "activation_reg_fwd: empty input (N=%d T1=%d n=%d)", N, T1, n);
    SAT_REQUIRE(((uintptr_t)scratch & 7) == 0, "activation_reg_fwd: scratch is not 8-byte aligned");
    const int nb = reg_blocks((long)N * T1);
    with_width(rows_wide(n, hidden), [&](auto vec) {
        hipLaunchKernelGGL(activation_reg_partial_kernel<decltype(vec)::value>, dim3(nb), dim3(256), 0, st, hidden, lengths, N, T1, n, (double*)scratch);
    });
    SAT_TRY(launch_ok("activation_reg_partial"));
    const double inv_pn = P > 0 ? 1.0 / ((double)P * n) : 0.0, inv_qn = Q > 0 ? 1.0 / ((double)Q * n) : 0.0;
    hipLaunchKernelGGL(activation_reg_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)scratch, nb, inv_pn, inv_qn, out);
    return launch_ok("activation_reg_finish");
}

int activation_reg_bwd(const float* hidden, const int* lengths, int N, int T1, int n, long P, long Q, const float* gscale, float* dH, hipStream_t st) {
    SAT_REQUIRE(N > 0 && T1 > 0 && n > 0, "activation_reg_bwd: empty input (N=%d T1=%d n=%d)", N, T1, n);
    if (P <= 0) return SAT_OK;                  // no live row: nothing to add
    const double ca = 2.0 / ((double)P * n), cb = Q > 0 ? 2.0 / ((double)Q * n) : 0.0;
    with_width(rows_wide(n, hidden, dH), [&](auto vec) {
        hipLaunchKernelGGL(activation_reg_bwd_kernel<decltype(vec)::value>, dim3(reg_blocks((long)N * T1)), dim3(256), 0, st, hidden, lengths, N, T1, n, ca, cb,
                           gscale, dH);
    });
    return launch_ok("activation_reg_bwd");
}

}  // namespace sat
