// The row core of the label-smoothed cross entropy, shared by ce_loss.hip (ce_rows_kernel, ce_grad_kernel) and token_loss.hip: the two
// files call these functions and nothing else for the cross-entropy part, so that sat_token_loss_fwd / _bwd with the cross entropy alone
// give sat_ce_label_smooth_fwd / _bwd's bits.  The float expressions are the ones ce_loss.hip has always had; change them here and both
// move together.
#pragma once
#include <math.h>

#include "common.h"
#include "row_reduce.h"

namespace sat {

// what one row's sweep leaves in LDS: per wave the online log-sum-exp pair, the sum of the logits and the arg-best
struct CeRowLds { float m[4], s[4], t[4], b[4]; int i[4]; };

// One sweep of row x (V words) by a 256-thread block: online log-sum-exp, the sum of the logits and the row argmax (ascending index: the
// first maximum wins, as torch.argmax).  Ends with the block's barrier; afterwards any thread may take ce_row_lse / ce_row_total, and
// thread 0 (whose bv, bi are its wave's best) ce_row_argmax.
template <int VEC>
__device__ __forceinline__ void ce_row_sweep(const float* x, int V, int tid, CeRowLds& l, float& bv, int& bi) {
    float mx = -INFINITY, sum = 0.f, tot = 0.f;
    bi = 0x7fffffff; bv = -INFINITY;
    row_sweep<VEC, kSweepDepth<VEC>, 256>(x, V / VEC, tid, [&](int u, const float (&e)[VEC]) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int v = u * VEC + j;
            tot += e[j];
            // a row of nothing but -inf: the 4-byte form names column 0, the 16-byte form no column (open items)
            const bool better = VEC == 1 ? arg_before(e[j], v, bv, bi) : e[j] > bv;
            if (better) { bv = e[j]; bi = v; }
        }
        lse_unit<VEC>(e, mx, sum);
    });
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
    wave_argbest(bv, bi);
    if ((tid & 63) == 0) { l.t[tid >> 6] = tot; l.b[tid >> 6] = bv; l.i[tid >> 6] = bi; }
    lse_wave_put(mx, sum, l.m, l.s, tid);
    __syncthreads();
}
__device__ __forceinline__ float ce_row_lse(const CeRowLds& l) { return lse_block(l.m, l.s); }
__device__ __forceinline__ float ce_row_total(const CeRowLds& l) {
    float Tt = 0.f;
    for (int k = 0; k < 4; ++k) Tt += l.t[k];
    return Tt;
}
__device__ __forceinline__ int ce_row_argmax(const CeRowLds& l, float bv, int bi) {
    argbest_merge<4>(bv, bi, l.b, l.i);
    return bi;
}
// the row loss from the row's log-sum-exp, the target's logit xt and the sum of the logits
__device__ __forceinline__ float ce_row_loss(float lse, float xt, float Tt, int V, float smoothing) {
    float nll = lse - xt;
    float smooth = lse - Tt / (float)V;
    return (1.f - smoothing) * nll + smoothing * smooth;
}
// one word of the gradient: sc * (softmax - smoothing/V - (1 - smoothing) [v == target]), sv = smoothing / V, conf = 1 - smoothing
__device__ __forceinline__ float ce_grad_word(float x, float lse, float sv, float conf, bool is_target, float sc) {
    return (__expf(x - lse) - sv - (is_target ? conf : 0.f)) * sc;
}

}  // namespace sat
