// Multi-tensor optimizer step on device: every parameter tensor of the model in ONE launch.
// Reference: SAT.configure_optimizers (model.py:723-757) builds torch.optim.SGD / Adam / AdamW over per-module
// parameter groups (lr, weight_decay per group); Lightning clips gradients by value or by global norm before the
// step (train.py:93-96, 273-274).  The arithmetic below is torch's single-tensor formulation of those optimizers
// (the reference's defaults: amsgrad off, maximize off, dampening 0), applied per element.
#include "../../include/sat_hip.h"
#include "common.h"

namespace sat {

constexpr int OPT_CHUNK = 1 << 16;      // elements per workgroup

// sum of squares of every gradient, fixed order: one partial per chunk, then one block over the partials
__global__ __launch_bounds__(256) void grad_sqsum_part_kernel(const sat_opt_tensor* __restrict__ tensors, const sat_opt_chunk* __restrict__ chunks,
                                                              double* __restrict__ part) {
    const sat_opt_chunk c = chunks[blockIdx.x];
    const sat_opt_tensor t = tensors[c.tensor];
    const long end = (c.start + OPT_CHUNK < t.n) ? c.start + OPT_CHUNK : t.n;
    double s = 0.0;
    for (long i = c.start + threadIdx.x; i < end; i += 256) { const float g = t.g[i]; s += (double)g * g; }
    __shared__ double sh[256];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}
// coef[0] = min(1, max_norm / (norm + 1e-6))  (torch.nn.utils.clip_grad_norm_), coef[1] = norm
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ part, int n, float max_norm, float* __restrict__ coef) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += part[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(sh[0]);
        const float c = max_norm / (norm + 1e-6f);
        coef[0] = c > 1.f ? 1.f : c; coef[1] = norm;          // a NaN norm hands on a NaN coefficient (clip_grad_norm_ does): the step then writes NaN
    }
}

// the gradient element both updates start from: scaled by the norm coefficient, then clipped by value as clip_grad_value_ clips it -
// +-inf clamp to +-clip_value and NaN stays NaN (fminf / fmaxf return the other operand for a NaN, hence the select)
__device__ __forceinline__ float clipped_grad(float g, float coef, float clip_value) {
    g *= coef;
    if (clip_value > 0.f) g = (g != g) ? g : fminf(fmaxf(g, -clip_value), clip_value);
    return g;
}

__device__ __forceinline__ void opt_update(const sat_opt_hyper& h, float lr, float wd, float coef, float& p, float g, float& m, float& v) {
    g = clipped_grad(g, coef, h.clip_value);
    if (h.kind == SAT_OPT_SGD) {
        if (wd != 0.f) g = fmaf(wd, p, g);
        if (h.momentum != 0.f) {
            m = h.first_step ? g : fmaf(h.momentum, m, g);                            // torch: buf = grad on the first step
            g = h.nesterov ? fmaf(h.momentum, m, g) : m;
        }
        p -= lr * g;
    } else {
        if (h.kind == SAT_OPT_ADAMW) p *= 1.f - lr * wd;                              // decoupled decay
        else if (wd != 0.f) g = fmaf(wd, p, g);                                       // Adam: L2 term joins the gradient
        m = m + (g - m) * (1.f - h.beta1);                                            // exp_avg.lerp_(grad, 1 - beta1)
        v = h.beta2 * v + (1.f - h.beta2) * g * g;
        const float denom = sqrtf(v) / h.bias_correction2_sqrt + h.eps;
        p -= (lr / h.bias_correction1) * (m / denom);
    }
}

__global__ __launch_bounds__(256) void optimizer_step_kernel(const sat_opt_tensor* __restrict__ tensors, const sat_opt_chunk* __restrict__ chunks,
                                                             sat_opt_hyper h, const sat_opt_hyper* __restrict__ h_dev, const float* __restrict__ clip_coef) {
    if (h_dev) h = *h_dev;          // hyper-parameters read from device memory (sat_optimizer_step_dev: the launch is replayed from a graph, the step count moves on)
    const sat_opt_chunk c = chunks[blockIdx.x];
    const sat_opt_tensor t = tensors[c.tensor];
    const long end = (c.start + OPT_CHUNK < t.n) ? c.start + OPT_CHUNK : t.n;
    const float coef = clip_coef ? clip_coef[0] : 1.f;
    const float lr = t.lr, wd = t.weight_decay;
    const bool has_m = t.m != nullptr, has_v = t.v != nullptr;
    // 16 bytes per lane where the tensor allows it (chunk starts are multiples of 64 Ki elements; bases come 16-byte aligned
    // from the allocator, checked here; the bf16 copy is stored 8 bytes at a time), scalar tail
    const bool vec = ((reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g) | reinterpret_cast<uintptr_t>(t.m) |
                       reinterpret_cast<uintptr_t>(t.v)) & 15) == 0 && (reinterpret_cast<uintptr_t>(t.shadow_bf16) & 7) == 0;
    long i = c.start;
    if (vec) {
        const long nv = (end - c.start) / 4;
        for (long q = threadIdx.x; q < nv; q += 256) {
            const long e = c.start + q * 4;
            float4 p4 = *reinterpret_cast<const float4*>(t.p + e);
            const float4 g4 = *reinterpret_cast<const float4*>(t.g + e);
            float4 m4 = has_m ? *reinterpret_cast<const float4*>(t.m + e) : make_float4(0, 0, 0, 0);
            float4 v4 = has_v ? *reinterpret_cast<const float4*>(t.v + e) : make_float4(0, 0, 0, 0);
            opt_update(h, lr, wd, coef, p4.x, g4.x, m4.x, v4.x); opt_update(h, lr, wd, coef, p4.y, g4.y, m4.y, v4.y);
            opt_update(h, lr, wd, coef, p4.z, g4.z, m4.z, v4.z); opt_update(h, lr, wd, coef, p4.w, g4.w, m4.w, v4.w);
            *reinterpret_cast<float4*>(t.p + e) = p4;
            if (t.shadow_bf16) {
                typedef __bf16 b4 __attribute__((ext_vector_type(4)));
                b4 o; o[0] = (__bf16)p4.x; o[1] = (__bf16)p4.y; o[2] = (__bf16)p4.z; o[3] = (__bf16)p4.w;
                *reinterpret_cast<b4*>(reinterpret_cast<__bf16*>(t.shadow_bf16) + e) = o;
            }
            if (has_m) *reinterpret_cast<float4*>(t.m + e) = m4;
            if (has_v) *reinterpret_cast<float4*>(t.v + e) = v4;
        }
        i = c.start + nv * 4;
    }
    for (i += threadIdx.x; i < end; i += 256) {
        float p = t.p[i], m = has_m ? t.m[i] : 0.f, v = has_v ? t.v[i] : 0.f;
        opt_update(h, lr, wd, coef, p, t.g[i], m, v);
        t.p[i] = p;
        if (t.shadow_bf16) reinterpret_cast<__bf16*>(t.shadow_bf16)[i] = (__bf16)p;
        if (has_m) t.m[i] = m;
        if (has_v) t.v[i] = v;
    }
}

// ---- averaged weights: the step above with one more stream, the average `a` of every element (ASGD's ax / an EMA), read and written in the
// pass that updates p.  A kernel of its own, so that a step without averaging launches exactly the kernel above.
// torch.optim.ASGD (single-tensor form): g += wd * p;  p *= 1 - lambd * eta;  p -= eta * g  (eta travels in the table's lr field)
__device__ __forceinline__ void asgd_update(const sat_opt_hyper& h, float lambd, float eta, float wd, float coef, float& p, float g) {
    g = clipped_grad(g, coef, h.clip_value);
    if (wd != 0.f) g = fmaf(wd, p, g);
    p *= fmaf(-lambd, eta, 1.f);
    p = fmaf(-eta, g, p);
}
__device__ __forceinline__ void avg_elem(const sat_opt_hyper& h, const sat_opt_avg_hyper& ah, float lr, float wd, float coef, float& p, float g,
                                         float& m, float& v, float& a) {
    if (h.kind == SAT_OPT_ASGD) asgd_update(h, ah.lambd, lr, wd, coef, p, g);
    else opt_update(h, lr, wd, coef, p, g, m, v);
    a = ah.coef == 1.f ? p : a + (p - a) * ah.coef;          // a coefficient of exactly 1 stores p itself: the average starts as a copy
}

__global__ __launch_bounds__(256) void optimizer_step_avg_kernel(const sat_opt_tensor* __restrict__ tensors, float* const* __restrict__ avg,
                                                                 const sat_opt_chunk* __restrict__ chunks, sat_opt_hyper h,
                                                                 const sat_opt_hyper* __restrict__ h_dev, sat_opt_avg_hyper ah,
                                                                 const sat_opt_avg_hyper* __restrict__ ah_dev, const float* __restrict__ clip_coef) {
    if (h_dev) { h = *h_dev; ah = *ah_dev; }
    const sat_opt_chunk c = chunks[blockIdx.x];
    const sat_opt_tensor t = tensors[c.tensor];
    float* const ta = avg[c.tensor];
    const long end = (c.start + OPT_CHUNK < t.n) ? c.start + OPT_CHUNK : t.n;
    const float coef = clip_coef ? clip_coef[0] : 1.f;
    const float lr = t.lr, wd = t.weight_decay;
    const bool asgd = h.kind == SAT_OPT_ASGD;
    const bool has_m = !asgd && t.m != nullptr, has_v = !asgd && t.v != nullptr, has_a = ta != nullptr;
    // the vector path needs every stream of the tensor 16-byte aligned: a parameter that is a view at an odd storage offset has a
    // freshly allocated (aligned) average, and the other way round after a loaded checkpoint
    const bool vec = ((reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g) | (has_m ? reinterpret_cast<uintptr_t>(t.m) : 0) |
                       (has_v ? reinterpret_cast<uintptr_t>(t.v) : 0) | reinterpret_cast<uintptr_t>(ta)) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(t.shadow_bf16) & 7) == 0;
    long i = c.start;
    if (vec) {
        const long nv = (end - c.start) / 4;
        for (long q = threadIdx.x; q < nv; q += 256) {
            const long e = c.start + q * 4;
            float4 p4 = *reinterpret_cast<const float4*>(t.p + e);
            const float4 g4 = *reinterpret_cast<const float4*>(t.g + e);
            float4 m4 = has_m ? *reinterpret_cast<const float4*>(t.m + e) : make_float4(0, 0, 0, 0);
            float4 v4 = has_v ? *reinterpret_cast<const float4*>(t.v + e) : make_float4(0, 0, 0, 0);
            float4 a4 = has_a ? *reinterpret_cast<const float4*>(ta + e) : make_float4(0, 0, 0, 0);
            avg_elem(h, ah, lr, wd, coef, p4.x, g4.x, m4.x, v4.x, a4.x); avg_elem(h, ah, lr, wd, coef, p4.y, g4.y, m4.y, v4.y, a4.y);
            avg_elem(h, ah, lr, wd, coef, p4.z, g4.z, m4.z, v4.z, a4.z); avg_elem(h, ah, lr, wd, coef, p4.w, g4.w, m4.w, v4.w, a4.w);
            *reinterpret_cast<float4*>(t.p + e) = p4;
            if (t.shadow_bf16) {
                typedef __bf16 b4 __attribute__((ext_vector_type(4)));
                b4 o; o[0] = (__bf16)p4.x; o[1] = (__bf16)p4.y; o[2] = (__bf16)p4.z; o[3] = (__bf16)p4.w;
                *reinterpret_cast<b4*>(reinterpret_cast<__bf16*>(t.shadow_bf16) + e) = o;
            }
            if (has_m) *reinterpret_cast<float4*>(t.m + e) = m4;
            if (has_v) *reinterpret_cast<float4*>(t.v + e) = v4;
            if (has_a) *reinterpret_cast<float4*>(ta + e) = a4;
        }
        i = c.start + nv * 4;
    }
    for (i += threadIdx.x; i < end; i += 256) {
        float p = t.p[i], m = has_m ? t.m[i] : 0.f, v = has_v ? t.v[i] : 0.f, a = has_a ? ta[i] : 0.f;
        avg_elem(h, ah, lr, wd, coef, p, t.g[i], m, v, a);
        t.p[i] = p;
        if (t.shadow_bf16) reinterpret_cast<__bf16*>(t.shadow_bf16)[i] = (__bf16)p;
        if (has_m) t.m[i] = m;
        if (has_v) t.v[i] = v;
        if (has_a) ta[i] = a;
    }
}

// p <-> a for every tensor that keeps an average; the bf16 filter copy follows the values that now sit in p
__global__ __launch_bounds__(256) void optimizer_swap_kernel(const sat_opt_tensor* __restrict__ tensors, float* const* __restrict__ avg,
                                                             const sat_opt_chunk* __restrict__ chunks) {
    const sat_opt_chunk c = chunks[blockIdx.x];
    const sat_opt_tensor t = tensors[c.tensor];
    float* const ta = avg[c.tensor];
    if (!ta) return;
    const long end = (c.start + OPT_CHUNK < t.n) ? c.start + OPT_CHUNK : t.n;
    const bool vec = ((reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(ta)) & 15) == 0 && (reinterpret_cast<uintptr_t>(t.shadow_bf16) & 7) == 0;
    long i = c.start;
    if (vec) {
        const long nv = (end - c.start) / 4;
        for (long q = threadIdx.x; q < nv; q += 256) {
            const long e = c.start + q * 4;
            const float4 p4 = *reinterpret_cast<const float4*>(t.p + e);
            const float4 a4 = *reinterpret_cast<const float4*>(ta + e);
            *reinterpret_cast<float4*>(t.p + e) = a4;
            *reinterpret_cast<float4*>(ta + e) = p4;
            if (t.shadow_bf16) {
                typedef __bf16 b4 __attribute__((ext_vector_type(4)));
                b4 o; o[0] = (__bf16)a4.x; o[1] = (__bf16)a4.y; o[2] = (__bf16)a4.z; o[3] = (__bf16)a4.w;
                *reinterpret_cast<b4*>(reinterpret_cast<__bf16*>(t.shadow_bf16) + e) = o;
            }
        }
        i = c.start + nv * 4;
    }
    for (i += threadIdx.x; i < end; i += 256) {
        const float p = t.p[i], a = ta[i];
        t.p[i] = a; ta[i] = p;
        if (t.shadow_bf16) reinterpret_cast<__bf16*>(t.shadow_bf16)[i] = (__bf16)a;
    }
}

}  // namespace sat

using namespace sat;

extern "C" {

int32_t sat_optimizer_chunk_elems(void) { return OPT_CHUNK; }

int sat_grad_clip_coef(const sat_opt_tensor* tensors, const sat_opt_chunk* chunks, int32_t n_chunks, float max_norm, double* scratch /* n_chunks */,
                       float* coef /* 2 floats */, void* stream) {
    if (!tensors || !chunks || !scratch || !coef) return fail(SAT_EINVAL, "grad_clip_coef: null pointer");
    SAT_REQUIRE(n_chunks > 0 && max_norm > 0.f, "grad_clip_coef: n_chunks=%d max_norm=%g", n_chunks, max_norm);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(grad_sqsum_part_kernel, dim3(n_chunks), dim3(256), 0, st, tensors, chunks, scratch);
    SAT_TRY(launch_ok("grad_sqsum_part"));
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, st, scratch, n_chunks, max_norm, coef);
    return launch_ok("grad_norm_finish");
}

int sat_optimizer_step(const sat_opt_tensor* tensors, const sat_opt_chunk* chunks, int32_t n_chunks, const sat_opt_hyper* hyper,
                       const float* clip_coef, void* stream) {
    if (!tensors || !chunks || !hyper) return fail(SAT_EINVAL, "optimizer_step: null pointer");
    if (n_chunks <= 0) return SAT_OK;
    SAT_REQUIRE(hyper->kind == SAT_OPT_SGD || hyper->kind == SAT_OPT_ADAM || hyper->kind == SAT_OPT_ADAMW, "optimizer_step: kind %d", hyper->kind);
    SAT_REQUIRE(hyper->kind == SAT_OPT_SGD || (hyper->bias_correction1 > 0.f && hyper->bias_correction2_sqrt > 0.f), "optimizer_step: bias corrections must be positive");
    hipLaunchKernelGGL(optimizer_step_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, tensors, chunks, *hyper, (const sat_opt_hyper*)nullptr, clip_coef);
    return launch_ok("optimizer_step");
}

int sat_optimizer_step_dev(const sat_opt_tensor* tensors, const sat_opt_chunk* chunks, int32_t n_chunks, const sat_opt_hyper* hyper_dev,
                           const float* clip_coef, void* stream) {
    if (!tensors || !chunks || !hyper_dev) return fail(SAT_EINVAL, "optimizer_step_dev: null pointer");
    if (n_chunks <= 0) return SAT_OK;
    sat_opt_hyper none = {};
    hipLaunchKernelGGL(optimizer_step_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, tensors, chunks, none, hyper_dev, clip_coef);
    return launch_ok("optimizer_step_dev");
}

int sat_optimizer_step_avg(const sat_opt_tensor* tensors, float* const* avg, const sat_opt_chunk* chunks, int32_t n_chunks,
                           const sat_opt_hyper* hyper, const sat_opt_avg_hyper* avg_hyper, const float* clip_coef, void* stream) {
    if (!tensors || !avg || !chunks || !hyper || !avg_hyper) return fail(SAT_EINVAL, "optimizer_step_avg: null pointer");
    SAT_REQUIRE(hyper->kind >= SAT_OPT_SGD && hyper->kind <= SAT_OPT_ASGD, "optimizer_step_avg: kind %d", hyper->kind);
    SAT_REQUIRE(avg_hyper->coef >= 0.f && avg_hyper->coef <= 1.f, "optimizer_step_avg: coefficient %g outside [0, 1]", avg_hyper->coef);
    SAT_REQUIRE(avg_hyper->lambd >= 0.f, "optimizer_step_avg: lambd %g is negative", avg_hyper->lambd);
    SAT_REQUIRE(hyper->kind == SAT_OPT_SGD || hyper->kind == SAT_OPT_ASGD || (hyper->bias_correction1 > 0.f && hyper->bias_correction2_sqrt > 0.f),
                "optimizer_step_avg: bias corrections must be positive");
    if (n_chunks <= 0) return SAT_OK;
    hipLaunchKernelGGL(optimizer_step_avg_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, tensors, avg, chunks, *hyper,
                       (const sat_opt_hyper*)nullptr, *avg_hyper, (const sat_opt_avg_hyper*)nullptr, clip_coef);
    return launch_ok("optimizer_step_avg");
}

int sat_optimizer_step_avg_dev(const sat_opt_tensor* tensors, float* const* avg, const sat_opt_chunk* chunks, int32_t n_chunks,
                               const sat_opt_hyper* hyper_dev, const sat_opt_avg_hyper* avg_hyper_dev, const float* clip_coef, void* stream) {
    if (!tensors || !avg || !chunks || !hyper_dev || !avg_hyper_dev) return fail(SAT_EINVAL, "optimizer_step_avg_dev: null pointer");
    if (n_chunks <= 0) return SAT_OK;
    sat_opt_hyper none = {};
    sat_opt_avg_hyper anone = {};
    hipLaunchKernelGGL(optimizer_step_avg_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, tensors, avg, chunks, none, hyper_dev, anone,
                       avg_hyper_dev, clip_coef);
    return launch_ok("optimizer_step_avg_dev");
}

int sat_optimizer_swap(const sat_opt_tensor* tensors, float* const* avg, const sat_opt_chunk* chunks, int32_t n_chunks, void* stream) {
    if (!tensors || !avg || !chunks) return fail(SAT_EINVAL, "optimizer_swap: null pointer");
    if (n_chunks <= 0) return SAT_OK;
    hipLaunchKernelGGL(optimizer_swap_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, tensors, avg, chunks);
    return launch_ok("optimizer_swap");
}

}
