// Temperature-scaling calibration (the reference's temperature_scaling.py:51-59): fit one scalar T by SGD on
//     loss(T) = mean_i [ log sum_j exp(x_ij / T) - x_iy / T ]          (F.cross_entropy(logits / T, targets))
//     dloss/dT = mean_i [ x_iy - sum_j p_ij x_ij ] / T^2                 with p_i = softmax(x_i / T)
// over packed logits x (P, V).  max_j(x_ij / T) = max_j(x_ij) / T for T > 0, so the row maximum m_i is computed ONCE per fit
// (temperature_rowmax_kernel, which also keeps x_iy - m_i); after that one evaluation is ONE streaming read of the logits that
// accumulates, per row and per temperature,
//     s = sum_j e_j,   w = sum_j d_j e_j,      d_j = x_ij - m_i <= 0,   e_j = exp(d_j / T) = exp2(d_j * (log2(e) / T))
// and nothing of size P*V is written:  loss_i = log s - (x_iy - m_i) / T,   g_i = ((x_iy - m_i) - w / s) / T^2.
//
// One wave per row (V = 6400: exactly 25 16-byte loads per lane; no LDS and no barrier in the streaming loop), four rows per
// workgroup.  Up to 8 temperatures share the pass: d_j is formed once, each temperature costs a multiply, two FMAs, one v_exp_f32
// and an add per element.  log2(e) / T is computed in double by a one-thread kernel and split into two floats, so the only error of
// the exponent is the rounding of the product d * c (relative 2^-24: in e_j it is |d/T| e^-|d/T| 2^-24 <= 0.37 * 2^-24 of the
// largest term, below the rounding of the sum itself).
// Reductions are in a fixed order: xor-butterfly inside the wave, the four rows of a workgroup summed in double in row order
// into one partial per workgroup, and temperature_finish_kernel (one workgroup per temperature) adds the partials in a fixed
// strided order + tree in double.  No atomics: the same input gives the same bits, on any stream.
// Every temperature goes through the same instructions whatever their number (this file is built with -ffp-contract=off and
// spells its FMAs out), so 8 temperatures in one call equal 8 single calls bit for bit.
//
// The fit enqueues kernels only (no memset / memcpy, no host synchronisation): T, the momentum buffer, the step count and the
// latch live in the workspace; temperature_sgd_kernel applies torch.optim.SGD's update in fp32 (the reference's T is an fp32
// tensor) and appends T and the loss to the device-side traces.  If T leaves (0, inf) the latch is set: later row / finish
// launches return at once, T stays, the T trace repeats it and the loss trace gets NaN, which is how the caller sees it.
#include "temperature.h"
#include "row_reduce.h"

#include <math.h>

namespace sat {
namespace {

constexpr int kRowsPerBlock = 4;          // one wave per row
constexpr float kDmin = -1e30f;           // d = x - m is clamped here: -inf logits give e = 0 and d * e = 0 instead of NaN

struct TempCoef { float c_hi, c_lo, T, pad; };                  // log2(e) / T split in two floats, and T itself
struct FitState { float T, buf; int step, latch; float loss, grad; int pad[2]; };

__global__ void temperature_coef_kernel(const float* __restrict__ temps, int n, TempCoef* __restrict__ coef) {
    const int t = threadIdx.x;
    if (t >= n) return;
    const float T = temps[t];
    const double c = 1.4426950408889634 / (double)T;
    TempCoef k; k.c_hi = (float)c; k.c_lo = (float)(c - (double)k.c_hi); k.T = T; k.pad = 0.f;
    coef[t] = k;
}

// rowmax[p] = max_j x_pj;  xt[p] = x_py - rowmax[p]  (NaN for a target outside [0, V): the loss then says so, nothing is read out of bounds)
template <int VEC>
__global__ __launch_bounds__(256) void temperature_rowmax_kernel(const float* __restrict__ logits, const int* __restrict__ target, int P, int V,
                                                                 float* __restrict__ rowmax, float* __restrict__ xt) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (p >= P) return;
    const float* x = logits + (long)p * V;
    float mx = -INFINITY;
    row_sweep<VEC, kSweepDepth<VEC>, 64>(x, V / VEC, lane, [&](int, const float (&e)[VEC]) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) mx = fmaxf(mx, e[j]);
    });
    mx = wave_max(mx);
    if (lane == 0) {
        const int t = target[p];
        rowmax[p] = mx;
        xt[p] = (t >= 0 && t < V) ? x[t] - mx : NAN;
    }
}

template <int NT>
__device__ __forceinline__ void accumulate(float xv, float m, const float (&c_hi)[NT], const float (&c_lo)[NT], float (&s)[NT], float (&w)[NT]) {
    float d = xv - m;
    d = d < kDmin ? kDmin : d;                 // not fmaxf: a NaN logit must stay NaN
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const float y = __fmaf_rn(d, c_lo[t], d * c_hi[t]);
        const float e = __builtin_amdgcn_exp2f(y);          // v_exp_f32; y <= 0, results below 2^-126 may flush to 0
        s[t] += e;
        w[t] = __fmaf_rn(d, e, w[t]);
    }
}

template <int NT>
__device__ __forceinline__ void accumulate4(const float4& q, float m, const float (&c_hi)[NT], const float (&c_lo)[NT], float (&s)[NT], float (&w)[NT]) {
    accumulate<NT>(q.x, m, c_hi, c_lo, s, w);
    accumulate<NT>(q.y, m, c_hi, c_lo, s, w);
    accumulate<NT>(q.z, m, c_hi, c_lo, s, w);
    accumulate<NT>(q.w, m, c_hi, c_lo, s, w);
}

// part[(t * gridDim.x + block) * 2 + {0, 1}] = sum over the rows of this workgroup of {loss_i, g_i} at temperature t
template <int NT, int VEC>
__global__ __launch_bounds__(256) void temperature_rows_kernel(const float* __restrict__ logits, const float* __restrict__ rowmax,
                                                               const float* __restrict__ xt, int P, int V, const TempCoef* __restrict__ coef,
                                                               const int* __restrict__ latch, double* __restrict__ part) {
    if (latch && *latch) return;
    __shared__ float s_term[kRowsPerBlock][kMaxTemperatures][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int p = blockIdx.x * kRowsPerBlock + wv;
    float li = 0.f, gi = 0.f;
    if (p < P) {                               // wave-uniform
        float c_hi[NT], c_lo[NT], s[NT], w[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) { c_hi[t] = coef[t].c_hi; c_lo[t] = coef[t].c_lo; s[t] = 0.f; w[t] = 0.f; }
        const float* x = logits + (long)p * V;
        const float m = rowmax[p];
        if (VEC == 4) {
            // trips of U 16-byte loads per lane; the loads of the next trip are issued before the arithmetic of this one (two register
            // sets, so that no copy is needed), the last partial trip is guarded per load
            constexpr int U = 4;
            const int V4 = V >> 2, full = V4 / (64 * U);
            const float4* x4 = reinterpret_cast<const float4*>(x) + lane;
            float4 qa[U], qb[U];
            if (full > 0) {
#pragma unroll
                for (int u = 0; u < U; ++u) qa[u] = x4[64 * u];
            }
            for (int k = 0; k < full; k += 2) {
                if (k + 1 < full) {
#pragma unroll
                    for (int u = 0; u < U; ++u) qb[u] = x4[(k + 1) * 64 * U + 64 * u];
                }
#pragma unroll
                for (int u = 0; u < U; ++u) accumulate4<NT>(qa[u], m, c_hi, c_lo, s, w);
                if (k + 2 < full) {
#pragma unroll
                    for (int u = 0; u < U; ++u) qa[u] = x4[(k + 2) * 64 * U + 64 * u];
                }
                if (k + 1 < full) {
#pragma unroll
                    for (int u = 0; u < U; ++u) accumulate4<NT>(qb[u], m, c_hi, c_lo, s, w);
                }
            }
            const int rest = V4 - full * 64 * U - lane;          // 16-byte groups left for this lane: every 64th of them
#pragma unroll
            for (int u = 0; u < U; ++u) if (64 * u < rest) qa[u] = x4[full * 64 * U + 64 * u];
#pragma unroll
            for (int u = 0; u < U; ++u) if (64 * u < rest) accumulate4<NT>(qa[u], m, c_hi, c_lo, s, w);
        } else {
            for (int v = lane; v < V; v += 64) accumulate<NT>(x[v], m, c_hi, c_lo, s, w);
        }
        // lane t finishes temperature t: the same instructions for every temperature count
        float ss = 0.f, ww = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float st = wave_sum(s[t]), wt = wave_sum(w[t]);
            if (lane == t) { ss = st; ww = wt; }
        }
        if (lane < NT) {
            const float T = coef[lane].T, xtp = xt[p];
            li = logf(ss) - xtp / T;
            gi = (xtp - ww / ss) / (T * T);
        }
    }
    if (lane < NT) { s_term[wv][lane][0] = li; s_term[wv][lane][1] = gi; }
    __syncthreads();
    if ((int)threadIdx.x < NT) {
        double L = 0.0, G = 0.0;
#pragma unroll
        for (int r = 0; r < kRowsPerBlock; ++r) { L += (double)s_term[r][threadIdx.x][0]; G += (double)s_term[r][threadIdx.x][1]; }
        double* o = part + ((long)threadIdx.x * gridDim.x + blockIdx.x) * 2;
        o[0] = L; o[1] = G;
    }
}

// workgroup t: loss_out[t] = sum_b part[t][b][0] / P, grad_out[t] = sum_b part[t][b][1] / P   (fixed strided order, then a tree; double)
__global__ __launch_bounds__(256) void temperature_finish_kernel(const double* __restrict__ part, int nb, int P, const int* __restrict__ latch,
                                                                 float* __restrict__ loss_out, float* __restrict__ grad_out) {
    if (latch && *latch) return;
    __shared__ double s_l[256], s_g[256];
    const double* q = part + (long)blockIdx.x * nb * 2;
    double L = 0.0, G = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) { L += q[2 * b]; G += q[2 * b + 1]; }
    L = block_tree_sum_d(L, s_l); G = block_tree_sum_d(G, s_g);
    if (threadIdx.x == 0) { loss_out[blockIdx.x] = (float)(L / (double)P); grad_out[blockIdx.x] = (float)(G / (double)P); }
}

__device__ __forceinline__ void set_coef(TempCoef* coef, float T) {
    const double c = 1.4426950408889634 / (double)T;
    TempCoef k; k.c_hi = (float)c; k.c_lo = (float)(c - (double)k.c_hi); k.T = T; k.pad = 0.f;
    coef[0] = k;
}

__global__ void temperature_fit_init_kernel(FitState* __restrict__ state, TempCoef* __restrict__ coef, float init, float* __restrict__ t_trace) {
    if (threadIdx.x != 0) return;
    FitState s; s.T = init; s.buf = 0.f; s.step = 0; s.latch = 0; s.loss = 0.f; s.grad = 0.f; s.pad[0] = s.pad[1] = 0;
    *state = s;
    set_coef(coef, init);
    t_trace[0] = init;
}

// One step of torch.optim.SGD(momentum, nesterov) on the device-resident scalar, in fp32 and without contraction:
// first step buf = g, afterwards buf = momentum * buf + g;  step = g + momentum * buf (nesterov) or buf;  T -= lr * step.
__global__ void temperature_sgd_kernel(FitState* __restrict__ state, TempCoef* __restrict__ coef, float lr, float momentum, int nesterov, int k,
                                       float* __restrict__ t_trace, float* __restrict__ loss_trace) {
    if (threadIdx.x != 0) return;
    FitState s = *state;
    if (s.latch) { t_trace[k + 1] = s.T; loss_trace[k] = NAN; return; }
    const float g = s.grad;
    loss_trace[k] = s.loss;
    s.buf = s.step == 0 ? g : momentum * s.buf + g;
    const float step = nesterov ? g + momentum * s.buf : s.buf;
    s.T = s.T - lr * step;
    s.step += 1;
    if (!(s.T > 0.f) || !(s.T < INFINITY)) s.latch = 1; else set_coef(coef, s.T);
    *state = s;
    t_trace[k + 1] = s.T;
}

struct TempWs { float* rowmax; float* xt; double* part; TempCoef* coef; FitState* state; int nb; };

size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }
TempWs carve(char* ws, int P) {
    TempWs w; w.nb = cdiv(P, kRowsPerBlock);
    w.rowmax = (float*)ws; w.xt = w.rowmax + P; ws += round256((size_t)P * 8);
    w.part = (double*)ws; ws += round256((size_t)w.nb * kMaxTemperatures * 2 * sizeof(double));
    w.coef = (TempCoef*)ws; ws += round256(sizeof(TempCoef) * kMaxTemperatures);
    w.state = (FitState*)ws;
    return w;
}

int launch_rowmax(const float* logits, const int* targets, int P, int V, const TempWs& w, hipStream_t st) {
    with_width(rows_wide(V, logits), [&](auto vec) {
        hipLaunchKernelGGL(temperature_rowmax_kernel<decltype(vec)::value>, dim3(w.nb), dim3(256), 0, st, logits, targets, P, V, w.rowmax, w.xt);
    });
    return launch_ok("temperature_rowmax");
}

template <int NT>
void launch_rows_nt(const float* logits, int P, int V, const TempWs& w, const int* latch, hipStream_t st) {
    with_width(rows_wide(V, logits), [&](auto vec) {
        hipLaunchKernelGGL((temperature_rows_kernel<NT, decltype(vec)::value>), dim3(w.nb), dim3(256), 0, st, logits, w.rowmax, w.xt, P, V, w.coef, latch, w.part);
    });
}

// loss and derivative at the n temperatures of w.coef: one read of the logits, then the fixed-order reduction
int launch_eval(const float* logits, int P, int V, int n, const TempWs& w, const int* latch, float* loss_out, float* grad_out, hipStream_t st) {
    switch (n) {
        case 1: launch_rows_nt<1>(logits, P, V, w, latch, st); break;
        case 2: launch_rows_nt<2>(logits, P, V, w, latch, st); break;
        case 3: launch_rows_nt<3>(logits, P, V, w, latch, st); break;
        case 4: launch_rows_nt<4>(logits, P, V, w, latch, st); break;
        case 5: launch_rows_nt<5>(logits, P, V, w, latch, st); break;
        case 6: launch_rows_nt<6>(logits, P, V, w, latch, st); break;
        case 7: launch_rows_nt<7>(logits, P, V, w, latch, st); break;
        case 8: launch_rows_nt<8>(logits, P, V, w, latch, st); break;
        default: return fail(SAT_EINVAL, "temperature: %d temperatures (1..%d)", n, kMaxTemperatures);
    }
    SAT_TRY(launch_ok("temperature_rows"));
    hipLaunchKernelGGL(temperature_finish_kernel, dim3(n), dim3(256), 0, st, w.part, w.nb, P, latch, loss_out, grad_out);
    return launch_ok("temperature_finish");
}

}  // namespace

size_t temperature_workspace_bytes(int P, int V) {
    (void)V;                                   // no term of size V: a row never has to fit anywhere
    const int nb = cdiv(P, kRowsPerBlock);
    return round256((size_t)P * 8) + round256((size_t)nb * kMaxTemperatures * 2 * sizeof(double)) + round256(sizeof(TempCoef) * kMaxTemperatures) +
           round256(sizeof(FitState));
}

int temperature_nll(const float* logits, const int* targets, int P, int V, const float* temperatures, int n, float* loss_out, float* grad_out,
                    char* ws, hipStream_t st) {
    const TempWs w = carve(ws, P);
    hipLaunchKernelGGL(temperature_coef_kernel, dim3(1), dim3(64), 0, st, temperatures, n, w.coef);
    SAT_TRY(launch_ok("temperature_coef"));
    SAT_TRY(launch_rowmax(logits, targets, P, V, w, st));
    return launch_eval(logits, P, V, n, w, nullptr, loss_out, grad_out, st);
}

int temperature_fit(const float* logits, const int* targets, int P, int V, float init, float lr, float momentum, int nesterov, int iters,
                    float* t_trace, float* loss_trace, char* ws, hipStream_t st) {
    const TempWs w = carve(ws, P);
    hipLaunchKernelGGL(temperature_fit_init_kernel, dim3(1), dim3(64), 0, st, w.state, w.coef, init, t_trace);
    SAT_TRY(launch_ok("temperature_fit_init"));
    SAT_TRY(launch_rowmax(logits, targets, P, V, w, st));
    for (int k = 0; k < iters; ++k) {
        SAT_TRY(launch_eval(logits, P, V, 1, w, &w.state->latch, &w.state->loss, &w.state->grad, st));
        hipLaunchKernelGGL(temperature_sgd_kernel, dim3(1), dim3(64), 0, st, w.state, w.coef, lr, momentum, nesterov, k, t_trace, loss_trace);
        SAT_TRY(launch_ok("temperature_sgd"));
    }
    return SAT_OK;
}

}  // namespace sat
