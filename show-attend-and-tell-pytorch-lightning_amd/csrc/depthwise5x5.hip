// Depthwise 5x5 convolutions, pad 2, stride 1 | 2 (torchvision's mobilenet_v3_small, blocks 4 - 11: InvertedResidual's depthwise
// ConvBNActivation with kernel_size 5).  NHWC activations (fp32 or bf16), fp32 filters (master weights in both modes), fp32 accumulation.
//
// Register budget: the 3x3 kernels of depthwise.hip keep 9 taps x 8 channels (bf16) in registers.  25 taps x 8 channels would be 200 VGPRs of
// taps alone, so here a thread owns FOUR channels in both storage types (16-byte loads in fp32, 8-byte loads in bf16): 100 tap registers,
// 4 accumulators.  Like the 3x3 layers these are memory-bound streaming kernels (50 FLOP per output element against 2 - 4 bytes).
#include "../../include/sat_hip.h"
#include "common.h"

namespace sat {
namespace {

typedef __bf16 bf;
constexpr int V5 = 4;          // channels per thread
constexpr int K5 = 25;         // taps

__device__ __forceinline__ void ld4c(const float* p, float (&o)[V5]) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
}
__device__ __forceinline__ void ld4c(const bf* p, float (&o)[V5]) {
    const uint2 q = *reinterpret_cast<const uint2*>(p);
    o[0] = __uint_as_float(q.x << 16); o[1] = __uint_as_float(q.x & 0xffff0000u);
    o[2] = __uint_as_float(q.y << 16); o[3] = __uint_as_float(q.y & 0xffff0000u);
}
__device__ __forceinline__ void st4c(float* p, const float (&o)[V5]) { *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]); }
__device__ __forceinline__ void st4c(bf* p, const float (&o)[V5]) {
    typedef __bf16 b4 __attribute__((ext_vector_type(4)));
    b4 q;
#pragma unroll
    for (int i = 0; i < V5; ++i) q[i] = (__bf16)o[i];
    *reinterpret_cast<b4*>(p) = q;
}

// w: the (C, 1, 5, 5) parameter = [C][25] fp32; the 25 x 4 taps of channels c .. c + 3 are 100 consecutive floats (c % 4 == 0: 16-byte aligned)
__device__ __forceinline__ void load_taps5(const float* __restrict__ w, int c, float (&wr)[K5][V5]) {
    const float4* wp = reinterpret_cast<const float4*>(w + (long)c * K5);
    float flat[V5 * K5];
#pragma unroll
    for (int j = 0; j < V5 * K5 / 4; ++j) { const float4 f = wp[j]; flat[4 * j] = f.x; flat[4 * j + 1] = f.y; flat[4 * j + 2] = f.z; flat[4 * j + 3] = f.w; }
#pragma unroll
    for (int i = 0; i < V5; ++i)
#pragma unroll
        for (int k = 0; k < K5; ++k) wr[k][i] = flat[i * K5 + k];
}

// y[n, p, q, c] = sum over taps (r, s) inside the map of x[n, p * stride + r - 2, q * stride + s - 2, c] * w[c, r, s]; taps in (r, s) order
template <typename T>
__global__ __launch_bounds__(256) void dw5x5_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w, T* __restrict__ y, int N, int H, int W, int C,
                                                        int P, int Q, int stride) {
    const int cv = C / V5;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)N * P * Q * cv) return;
    const int c = (int)(e % cv) * V5; long t = e / cv;
    const int q = (int)(t % Q); t /= Q; const int p = (int)(t % P); const int n = (int)(t / P);
    float wr[K5][V5];
    load_taps5(w, c, wr);
    float acc[V5] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const int h = p * stride + r - 2;
        if (h < 0 || h >= H) continue;
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            const int ww = q * stride + s - 2;
            if (ww < 0 || ww >= W) continue;
            float xv[V5];
            ld4c(x + (((long)n * H + h) * W + ww) * C + c, xv);
#pragma unroll
            for (int i = 0; i < V5; ++i) acc[i] = fmaf(xv[i], wr[r * 5 + s][i], acc[i]);
        }
    }
    st4c(y + e * V5, acc);          // (n, p, q, c) row-major = e * V5
}

// dx[n, h, w, c] = sum over taps (r, s) with h + 2 - r = p * stride, w + 2 - s = q * stride (0 <= p < P, 0 <= q < Q) of dy[n, p, q, c] * w[c, r, s]
template <typename T>
__global__ __launch_bounds__(256) void dw5x5_dgrad_kernel(const T* __restrict__ dy, const float* __restrict__ w, T* __restrict__ dx, int N, int H, int W, int C,
                                                          int P, int Q, int stride) {
    const int cv = C / V5;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)N * H * W * cv) return;
    const int c = (int)(e % cv) * V5; long t = e / cv;
    const int ww = (int)(t % W); t /= W; const int h = (int)(t % H); const int n = (int)(t / H);
    float wr[K5][V5];
    load_taps5(w, c, wr);
    float acc[V5] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const int ph = h + 2 - r;
        if (ph < 0 || ph % stride) continue;
        const int p = ph / stride;
        if (p >= P) continue;
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            const int qw = ww + 2 - s;
            if (qw < 0 || qw % stride) continue;
            const int q = qw / stride;
            if (q >= Q) continue;
            float gv[V5];
            ld4c(dy + (((long)n * P + p) * Q + q) * C + c, gv);
#pragma unroll
            for (int i = 0; i < V5; ++i) acc[i] = fmaf(gv[i], wr[r * 5 + s][i], acc[i]);
        }
    }
    st4c(dx + e * V5, acc);
}

// dw[c][r][s] = sum over output pixels of dy * x(tap).  Block (pixel chunk blockIdx.x, group blockIdx.y of cvb channel vectors): thread = channel
// vector tid % cvb, pixel lane tid / cvb; 25 x 4 accumulators per thread; the pixel lanes are combined through LDS in a fixed order, one tap at a
// time, into the partial [chunk][25][C]; a second launch adds the chunks in a fixed order.
template <typename T>
__global__ __launch_bounds__(256) void dw5x5_wgrad_part_kernel(const T* __restrict__ dy, const T* __restrict__ x, float* __restrict__ part, int N, int H, int W, int C,
                                                               int P, int Q, int stride, int chunk, int cvb) {
    const int cv = C / V5;
    const int pix_par = blockDim.x / cvb;
    const int vl = threadIdx.x % cvb, pl = threadIdx.x / cvb;
    const int vi = blockIdx.y * cvb + vl;
    const bool live = pl < pix_par && vi < cv;
    const int c = vi * V5;
    float acc[K5][V5];
#pragma unroll
    for (int k = 0; k < K5; ++k)
#pragma unroll
        for (int i = 0; i < V5; ++i) acc[k][i] = 0.f;
    const long npix = (long)N * P * Q;
    const long p0 = (long)blockIdx.x * chunk, p1 = p0 + chunk < npix ? p0 + chunk : npix;
    if (live) {
        for (long pix = p0 + pl; pix < p1; pix += pix_par) {
            const int q = (int)(pix % Q); long t = pix / Q; const int p = (int)(t % P); const int n = (int)(t / P);
            float gv[V5];
            ld4c(dy + pix * C + c, gv);
#pragma unroll
            for (int r = 0; r < 5; ++r) {
                const int h = p * stride + r - 2;
                if (h < 0 || h >= H) continue;
#pragma unroll
                for (int s = 0; s < 5; ++s) {
                    const int ww = q * stride + s - 2;
                    if (ww < 0 || ww >= W) continue;
                    float xv[V5];
                    ld4c(x + (((long)n * H + h) * W + ww) * C + c, xv);
#pragma unroll
                    for (int i = 0; i < V5; ++i) acc[r * 5 + s][i] = fmaf(gv[i], xv[i], acc[r * 5 + s][i]);
                }
            }
        }
    }
    extern __shared__ float sm[];
    const int CB = cvb * V5;
#pragma unroll
    for (int k = 0; k < K5; ++k) {
        if (pl < pix_par)
#pragma unroll
            for (int i = 0; i < V5; ++i) sm[pl * CB + vl * V5 + i] = acc[k][i];
        __syncthreads();
        for (int o = threadIdx.x; o < CB; o += blockDim.x) {
            const int ch = blockIdx.y * CB + o;
            if (ch < C) {
                float tsum = 0.f;
                for (int l = 0; l < pix_par; ++l) tsum += sm[l * CB + o];
                part[((long)blockIdx.x * K5 + k) * C + ch] = tsum;
            }
        }
        __syncthreads();
    }
}
// one wave per filter element: lane l adds partials l, l + 64, ... in double, then a fixed xor tree
__global__ __launch_bounds__(64) void dw5x5_wgrad_finish_kernel(const float* __restrict__ part, int nparts, int C, float* __restrict__ dw) {
    const int o = blockIdx.x;                                     // o = k * C + c in the partials; dw is [C][25]
    double s = 0.0;
    for (int b = threadIdx.x; b < nparts; b += 64) s += (double)part[(long)b * K5 * C + o];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
    if (threadIdx.x == 0) {
        const int k = o / C, c = o - k * C;
        dw[c * K5 + k] = (float)s;
    }
}

}  // namespace
}  // namespace sat

using namespace sat;

// output pixels per partial: ~1024 chunks per launch, at least 64 pixels, at most 2048 (as the 3x3 filter gradient)
static inline int dw5_chunk(long npix) {
    long c = (npix + 1023) / 1024;
    c = (c + 63) / 64 * 64;
    return (int)(c < 64 ? 64 : (c > 2048 ? 2048 : c));
}
static inline int dw5_cvb(int C) {          // the largest divisor of C / 4 up to 32: no idle lanes, >= 8 pixel lanes per block
    const int cv = C / V5;
    int cvb = cv < 32 ? cv : 32;
    while (cv % cvb) --cvb;
    return cvb;
}
static inline void dw5_out(int H, int W, int stride, int& P, int& Q) { P = (H + 4 - 5) / stride + 1; Q = (W + 4 - 5) / stride + 1; }

extern "C" {

static int dw5_check(const void* a, const void* b, const void* c, int N, int H, int W, int C, int stride, int dtype, const char* what) {
    if (!a || !b || !c) return fail(SAT_EINVAL, "%s: null pointer", what);
    SAT_REQUIRE(dtype == 0 || dtype == 1, "%s: dtype %d (0 = fp32, 1 = bf16)", what, dtype);
    SAT_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % V5 == 0 && (stride == 1 || stride == 2), "%s: bad shape (N=%d H=%d W=%d C=%d stride=%d; C %% 4 == 0)",
                what, N, H, W, C, stride);
    SAT_REQUIRE((long)N * H * W * C < (1L << 40), "%s: tensor too large", what);
    return SAT_OK;
}

int sat_dwconv5x5_fwd_t(int32_t dtype, const void* x, const float* w, void* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t stride, void* stream) {
    SAT_TRY(dw5_check(x, w, y, N, H, W, C, stride, dtype, "dwconv5x5_fwd"));
    int P, Q; dw5_out(H, W, stride, P, Q);
    const long total = (long)N * P * Q * (C / V5);
    if (dtype) hipLaunchKernelGGL(dw5x5_fwd_kernel<bf>, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (const bf*)x, w, (bf*)y, N, H, W, C, P, Q, stride);
    else hipLaunchKernelGGL(dw5x5_fwd_kernel<float>, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)x, w, (float*)y, N, H, W, C, P, Q, stride);
    return launch_ok("dwconv5x5_fwd");
}

int sat_dwconv5x5_dgrad_t(int32_t dtype, const void* dy, const float* w, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t stride, void* stream) {
    SAT_TRY(dw5_check(dy, w, dx, N, H, W, C, stride, dtype, "dwconv5x5_dgrad"));
    int P, Q; dw5_out(H, W, stride, P, Q);
    const long total = (long)N * H * W * (C / V5);
    if (dtype) hipLaunchKernelGGL(dw5x5_dgrad_kernel<bf>, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (const bf*)dy, w, (bf*)dx, N, H, W, C, P, Q, stride);
    else hipLaunchKernelGGL(dw5x5_dgrad_kernel<float>, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)dy, w, (float*)dx, N, H, W, C, P, Q, stride);
    return launch_ok("dwconv5x5_dgrad");
}

size_t sat_dwconv5x5_wgrad_scratch_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t stride) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % V5 || (stride != 1 && stride != 2)) return 0;
    int P, Q; dw5_out(H, W, stride, P, Q);
    const long npix = (long)N * P * Q;
    return (size_t)cdiv(npix, (long)dw5_chunk(npix)) * K5 * C * sizeof(float);
}

int sat_dwconv5x5_wgrad_t(int32_t dtype, const void* dy, const void* x, float* dw, int32_t N, int32_t H, int32_t W, int32_t C, int32_t stride, float* scratch,
                          void* stream) {
    SAT_TRY(dw5_check(dy, x, dw, N, H, W, C, stride, dtype, "dwconv5x5_wgrad"));
    if (!scratch) return fail(SAT_EINVAL, "dwconv5x5_wgrad: null scratch");
    int P, Q; dw5_out(H, W, stride, P, Q);
    const long npix = (long)N * P * Q;
    const int chunk = dw5_chunk(npix), nparts = cdiv(npix, (long)chunk);
    const int cvb = dw5_cvb(C), pix_par = 256 / cvb;
    const size_t lds = (size_t)pix_par * cvb * V5 * sizeof(float);
    const dim3 grid(nparts, cdiv(C / V5, cvb));
    if (dtype) hipLaunchKernelGGL(dw5x5_wgrad_part_kernel<bf>, grid, dim3(256), lds, (hipStream_t)stream, (const bf*)dy, (const bf*)x, scratch, N, H, W, C, P, Q, stride, chunk, cvb);
    else hipLaunchKernelGGL(dw5x5_wgrad_part_kernel<float>, grid, dim3(256), lds, (hipStream_t)stream, (const float*)dy, (const float*)x, scratch, N, H, W, C, P, Q, stride, chunk, cvb);
    SAT_TRY(launch_ok("dwconv5x5_wgrad (partials)"));
    hipLaunchKernelGGL(dw5x5_wgrad_finish_kernel, dim3(K5 * C), dim3(64), 0, (hipStream_t)stream, scratch, nparts, C, dw);
    return launch_ok("dwconv5x5_wgrad (finish)");
}

}
