// Device cores shared by the kernels that walk a vocabulary row (decoder_kernels.h, ce_loss.hip and token_loss.hip through ce_row.h,
// policy_loss.hip, distill_loss.hip, temperature.hip): the row sweep and its two access widths, the online log-sum-exp, the block arg-best and its pick loops, the
// ensemble's word, and the double fixed-order tree of the finish kernels.
// The bits depend on the shape of the float expressions, so the two FMAs of the recurrence are spelled out (left to contraction, the
// compiler fused them in one kernel and not in the next); change them here and every user moves together.  A file built with
// -ffp-contract=off takes only what has no floating-point arithmetic of its own to contract: the row sweep (load_unit, store_unit,
// row_sweep, rows_wide, with_width) and block_tree_sum_d.
#pragma once
#include <math.h>

#include <type_traits>

#include "../../include/sat_hip.h"
#include "common.h"

namespace sat {

// ------------------------------------------------------------------ the row sweep: a packed row as units of VEC words
// VEC = 4: one 16-byte access per unit (rows_wide: V % 4 == 0, i.e. every row stays 16-byte aligned); VEC = 1: any V, any base.
template <int VEC>
__device__ __forceinline__ void load_unit(const float* __restrict__ x, int u, float (&e)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 q = reinterpret_cast<const float4*>(x)[u];
        e[0] = q.x; e[1] = q.y; e[2] = q.z; e[3] = q.w;
    } else {
        e[0] = x[u];
    }
}
template <int VEC>
__device__ __forceinline__ void store_unit(float* __restrict__ g, int u, const float (&e)[VEC]) {
    if constexpr (VEC == 4) reinterpret_cast<float4*>(g)[u] = make_float4(e[0], e[1], e[2], e[3]);
    else g[u] = e[0];
}
// units in flight per thread of a single-row sweep.  (One 4-byte load per trip round the online-softmax recurrence was 144 us for the
// 54 MB of C2's logits, four 16-byte loads in flight 66 us.)  The 4-byte form stays at one, the loop it has always been.
template <int VEC> constexpr int kSweepDepth = VEC == 4 ? 4 : 1;
// One thread's share of a row of `units` units: it starts at unit `first` and steps by THREADS * U; every trip issues the loads of its
// (up to U) units inside the row before body(u, e) runs on them in ascending u -- the order a thread-local recurrence sees is that of
// a plain strided loop.  A unit outside the row is neither loaded nor passed on.
template <int VEC, int U, int THREADS, typename Body>
__device__ __forceinline__ void row_sweep(const float* x, int units, int first, Body&& body) {
    for (int u0 = first; u0 < units; u0 += THREADS * U) {
        float e[U][VEC];
#pragma unroll
        for (int k = 0; k < U; ++k) if (u0 + THREADS * k < units) load_unit<VEC>(x, u0 + THREADS * k, e[k]);
#pragma unroll
        for (int k = 0; k < U; ++k) if (u0 + THREADS * k < units) body(u0 + THREADS * k, e[k]);
    }
}
// host: rows of V words take the 16-byte form when V % 4 == 0 and every array a sweep touches starts 16-byte aligned ...
template <typename... T>
inline bool rows_wide(long V, const T*... base) { return V % 4 == 0 && (((uintptr_t)base | ... | (uintptr_t)0) % 16 == 0); }
// ... and f(VEC) gets the width as an integral constant, so that a launcher names its kernel once
template <typename F>
inline void with_width(bool wide, F&& f) {
    if (wide) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 1>{});
}

// ------------------------------------------------------------------ online log-sum-exp of a row: a (max, sum of exp(x - max)) pair
// one word.  A -inf word carries no mass and is skipped: with mx still -inf the difference would be NaN.
__device__ __forceinline__ void lse_word(float x, float& mx, float& sum) {
    if (x == -INFINITY) return;
    if (x > mx) { sum = fmaf(sum, __expf(mx - x), 1.f); mx = x; } else sum += __expf(x - mx);
}
// a unit of four words (one 16-byte load): one rescale per unit, the four exponentials summed pairwise
__device__ __forceinline__ void lse_unit4(const float (&e)[4], float& mx, float& sum) {
    const float m4 = fmaxf(fmaxf(e[0], e[1]), fmaxf(e[2], e[3]));
    if (m4 > mx) { sum *= __expf(mx - m4); mx = m4; }          // exp(-inf) = 0 on the first trip
    if (mx != -INFINITY) sum += (__expf(e[0] - mx) + __expf(e[1] - mx)) + (__expf(e[2] - mx) + __expf(e[3] - mx));
}
// one unit of a sweep, of either width ...
template <int VEC>
__device__ __forceinline__ void lse_unit(const float (&e)[VEC], float& mx, float& sum) {
    if constexpr (VEC == 4) lse_unit4(e, mx, sum);
    else lse_word(e[0], mx, sum);
}
// ... and of the words e * s.  The student's pair at tau and the teachers' pairs of the distillation loss go through this one function,
// so a teacher that is the student gets the student's bits.
template <int VEC>
__device__ __forceinline__ void lse_unit(const float (&e)[VEC], float s, float& mx, float& sum) {
    if constexpr (VEC == 4) {
        const float x[4] = {e[0] * s, e[1] * s, e[2] * s, e[3] * s};
        lse_unit4(x, mx, sum);
    } else {
        lse_word(e[0] * s, mx, sum);
    }
}
// the pairs of a wave: xor butterfly, every lane ends with the wave's pair.  LAST_UNFUSED: the last step rounds both products before
// the add.  That is the rounding beam_scores_row has had since the compiler first packed the two multiplies of that step (and only
// there); the search's scores are pinned bit for bit, so it stays until they are moved on purpose.
template <bool LAST_UNFUSED = false>
__device__ __forceinline__ void lse_wave(float& mx, float& sum) {
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(mx, o, 64), os = __shfl_xor(sum, o, 64);
        const float nm = fmaxf(mx, om);
        const float fa = (mx == nm) ? 1.f : __expf(mx - nm), fb = (om == nm) ? 1.f : __expf(om - nm);   // (-inf) - (-inf) guard
        sum = LAST_UNFUSED && o == 1 ? __fadd_rn(__fmul_rn(sum, fa), __fmul_rn(os, fb)) : fmaf(sum, fa, os * fb);
        mx = nm;
    }
}
// ... which lane 0 of each of the block's four waves leaves in s_m[0..3] / s_s[0..3]; after the caller's barrier lse_block is the row's
template <bool LAST_UNFUSED = false>
__device__ __forceinline__ void lse_wave_put(float mx, float sum, float* s_m, float* s_s, int tid) {
    lse_wave<LAST_UNFUSED>(mx, sum);
    if ((tid & 63) == 0) { s_m[tid >> 6] = mx; s_s[tid >> 6] = sum; }
}
__device__ __forceinline__ float lse_block(const float* s_m, const float* s_s) {
    const float M = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
    float S = 0.f;
    for (int k = 0; k < 4; ++k) S += (s_m[k] == M) ? s_s[k] : s_s[k] * __expf(s_m[k] - M);
    return M + __logf(S);
}

// ------------------------------------------------------------------ block arg-best: value descending, ties to the lowest index
// The order is strict (no two entries share an index), so the winner does not depend on the order of the merges.
template <typename I>
__device__ __forceinline__ bool arg_before(float av, I ai, float bv, I bi) { return av > bv || (av == bv && ai < bi); }
template <typename I>
__device__ __forceinline__ void wave_argbest(float& bv, I& bi) {
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64); const I oi = __shfl_xor(bi, o, 64);
        if (arg_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
}
// thread 0, after the barrier behind "lane 0 of wave w wrote its wave's best to s_v[w], s_i[w]": the best of the block's WAVES waves
template <int WAVES, typename I>
__device__ __forceinline__ void argbest_merge(float& bv, I& bi, const float* s_v, const I* s_i) {
    for (int w = 1; w < WAVES; ++w) if (arg_before(s_v[w], s_i[w], bv, bi)) { bv = s_v[w]; bi = s_i[w]; }
}
// every thread's best in, the block's best out in thread 0 (and nowhere else), through one barrier
template <int WAVES, typename I>
__device__ __forceinline__ void block_argbest(float& bv, I& bi, float* s_v, I* s_i, int tid) {
    wave_argbest(bv, bi);
    if ((tid & 63) == 0) { s_v[tid >> 6] = bv; s_i[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) argbest_merge<WAVES>(bv, bi, s_v, s_i);
}
// k picks from a scratch copy wk of n scores, by a block of 1024 threads: a winner is marked as taken with NaN, which the scan skips --
// apart from -inf entries, which come last in index order.  Thread 0 calls emit(pick, value, index) (index >= n: nothing was left).
template <typename Emit>
__device__ __forceinline__ void block_picks_marking(float* __restrict__ wk, long n, int k, Emit&& emit, int tid) {
    __shared__ float s_v[16]; __shared__ long s_i[16];
    for (int it = 0; it < k; ++it) {
        float bv = -INFINITY; long bi = 0x7fffffffffffffffL;
        for (long i = tid; i < n; i += 1024) { const float v = wk[i]; if (v != v) continue; if (arg_before(v, i, bv, bi)) { bv = v; bi = i; } }
        block_argbest<16>(bv, bi, s_v, s_i, tid);
        if (tid == 0) {
            emit(it, bv, bi);
            if (bi < n) wk[bi] = __int_as_float(0x7fc00000);
        }
        __syncthreads();
    }
}
// `picks` picks from n entries without scratch, by a block of WAVES waves: every pass looks for the best entry strictly after the previous
// pick.  entry(i, value, id) reads entry i < n; thread 0 calls emit(pick, value, id) (id == INT_MAX: nothing was left, and with
// stop_when_out the loop ends there).
template <int WAVES, typename Entry, typename Emit>
__device__ __forceinline__ void block_picks_in_order(int n, int picks, bool stop_when_out, Entry&& entry, Emit&& emit, int tid) {
    __shared__ float s_v[WAVES]; __shared__ int s_i[WAVES]; __shared__ float s_b; __shared__ int s_bi;
    float lastv = INFINITY; int lasti = -1;
    for (int t = 0; t < picks; ++t) {
        float bv = -INFINITY; int bi = 0x7fffffff;
        for (int i = tid; i < n; i += WAVES * 64) {
            float x; int id;
            entry(i, x, id);
            const bool after = x < lastv || (x == lastv && id > lasti);      // strictly after the previous pick in (value desc, index asc) order
            if (after && arg_before(x, id, bv, bi)) { bv = x; bi = id; }
        }
        block_argbest<WAVES>(bv, bi, s_v, s_i, tid);
        if (tid == 0) { s_b = bv; s_bi = bi; emit(t, bv, bi); }
        __syncthreads();
        lastv = s_b; lasti = s_bi;
        if (stop_when_out && lasti == 0x7fffffff) break;
    }
}

// ------------------------------------------------------------------ ensemble: the combined word of M members ("Ensemble decoding")
struct EnsembleArgs {
    const float* z[SAT_ENSEMBLE_MAX];           // the members' logits (rows, V)
    float w[SAT_ENSEMBLE_MAX];
    float logw[SAT_ENSEMBLE_MAX];
};
inline EnsembleArgs ensemble_args(const float* const* logits, const float* weight, int members) {
    EnsembleArgs a;
    for (int i = 0; i < SAT_ENSEMBLE_MAX; ++i) {
        a.z[i] = i < members ? logits[i] : nullptr;
        a.w[i] = i < members ? weight[i] : 0.f;
        a.logw[i] = i < members && weight[i] > 0.f ? logf(weight[i]) : 0.f;
    }
    return a;
}
// c of one word from the members' raw logits x and their rows' log-sum-exps at inv_temp; MC = the member capacity the caller is compiled
// for.  The search (sat_beam_search_ensemble) and the distillation loss share it: the student learns the distribution the search decodes.
template <int MC>
__device__ __forceinline__ float ensemble_word(const float (&x)[MC], const float (&lse)[MC], const EnsembleArgs& a, int M, int geometric, float inv_temp) {
    if (geometric) {
        float c = 0.f;
#pragma unroll
        for (int i = 0; i < MC; ++i) if (i < M && a.w[i] != 0.f) c += a.w[i] * (x[i] * inv_temp - lse[i]);
        return c;
    }
    float t[MC];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < MC; ++i) if (i < M && a.w[i] != 0.f) { t[i] = x[i] * inv_temp - lse[i] + a.logw[i]; mx = fmaxf(mx, t[i]); }
    if (mx == -INFINITY) return mx;             // only from -inf logits: no member gives this word any mass
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MC; ++i) if (i < M && a.w[i] != 0.f) s += __expf(t[i] - mx);
    return mx + __logf(s);
}

// ------------------------------------------------------------------ the finish kernels' sum: double, 256 threads, fixed order
// x is the thread's strided partial; the tree 128, 64, .., 1 over s256 (256 doubles of LDS) follows.  Every thread gets the sum.
__device__ __forceinline__ double block_tree_sum_d(double x, double* s256) {
    s256[threadIdx.x] = x;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) s256[threadIdx.x] += s256[threadIdx.x + o]; __syncthreads(); }
    return s256[0];
}

}  // namespace sat
