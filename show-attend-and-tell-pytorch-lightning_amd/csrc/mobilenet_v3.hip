// The two operations mobilenet_v3_small adds to the BatchNorm / convolution kit of the other encoders (torchvision 0.10's MobileNetV3;
// Howard et al. 2019, "Searching for MobileNetV3"):
//
//   BatchNorm + hard-swish: hardswish(v) = v * min(max(v + 3, 0), 6) / 6 of the BatchNorm output v.  Its own kernels, not a run-time branch of
//     encoder.hip's bn_apply_kernel.  Training statistics come from the existing statistics passes (sat_bn_train_fwd_t /
//     sat_bn_train_fwd_tiles_bf16 with y = NULL).  Hard-swish is not invertible from its output and a 1-bit mask cannot carry its slope, so the
//     backward recomputes v from x, mean, invstd, gamma and beta (the same association as the forward: bit-identical v, same region decision)
//     and uses torch's kink conventions: v <= -3 -> 0, v < 3 -> g (v / 3 + 0.5), else g.
//   Squeeze-and-excitation: s[n, c] = hardsigmoid(fc2(relu(fc1(mean_hw x[n, :, :, c])))), y = x * s.  One block per image forms the pooled
//     means (fixed order), both 1x1 layers and the scale; backward: ds = sum_hw g x (fixed order), the layer gradients per image, then the weight
//     and bias gradients summed over the images in image order, and dx = g s + dpool / HW.  No atomics, no memset / memcpy: capturable.
//
// NHWC activations (fp32 or bf16 storage), fp32 statistics / SE vectors / parameter gradients, reductions in double.
#include "../../include/sat_hip.h"
#include "common.h"

namespace sat {
namespace {

typedef __bf16 bf;
template <typename T> struct EV { static constexpr int n = 16 / sizeof(T); };          // elements per 16-byte vector

template <typename T, int N> __device__ __forceinline__ void unpk(const uint4& r, float (&o)[N]);
template <> __device__ __forceinline__ void unpk<float, 4>(const uint4& r, float (&o)[4]) {
    o[0] = __uint_as_float(r.x); o[1] = __uint_as_float(r.y); o[2] = __uint_as_float(r.z); o[3] = __uint_as_float(r.w);
}
template <> __device__ __forceinline__ void unpk<bf, 8>(const uint4& r, float (&o)[8]) {
    o[0] = __uint_as_float(r.x << 16); o[1] = __uint_as_float(r.x & 0xFFFF0000u); o[2] = __uint_as_float(r.y << 16); o[3] = __uint_as_float(r.y & 0xFFFF0000u);
    o[4] = __uint_as_float(r.z << 16); o[5] = __uint_as_float(r.z & 0xFFFF0000u); o[6] = __uint_as_float(r.w << 16); o[7] = __uint_as_float(r.w & 0xFFFF0000u);
}
template <typename T, int N> __device__ __forceinline__ uint4 pk(const float (&v)[N]);
template <> __device__ __forceinline__ uint4 pk<float, 4>(const float (&v)[4]) {
    return make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
}
template <> __device__ __forceinline__ uint4 pk<bf, 8>(const float (&v)[8]) {
    typedef __bf16 b8 __attribute__((ext_vector_type(8)));
    b8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = (__bf16)v[i];
    return *reinterpret_cast<uint4*>(&o);
}

__device__ __forceinline__ float hswish(float v) { return v * fminf(fmaxf(v + 3.f, 0.f), 6.f) / 6.f; }          // ATen's association
// torch's hardswish_backward (ATen BinaryOpsKernel): v <= -3 -> 0, v < 3 -> g (v / 3 + 0.5), else g - both kinks take the outer branch
__device__ __forceinline__ float hswish_grad(float v, float g) { return v <= -3.f ? 0.f : (v < 3.f ? g * (v / 3.f + 0.5f) : g); }

// ------------------------------------------------------------------ BatchNorm + hard-swish
// y = hardswish((x - mean) * invstd * gamma + beta); EVAL: `invstd` holds the running variance, 1 / sqrt(var + eps) is taken here (as
// bn_apply_kernel<EVAL> does).  One 16-byte vector per thread.
template <typename T, bool EVAL>
__global__ __launch_bounds__(256) void bn_hswish_apply_kernel(const T* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta, T* __restrict__ y, long totalv,
                                                              int CV, float eps) {
    constexpr int E = EV<T>::n;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= totalv) return;
    const int c0 = (int)(e % CV) * E;
    const uint4 xr = reinterpret_cast<const uint4*>(x)[e];
    float xv[E], o[E];
    unpk<T, E>(xr, xv);
#pragma unroll
    for (int i = 0; i < E; ++i) {
        float is = invstd[c0 + i];
        if (EVAL) is = 1.f / sqrtf(is + eps);
        const float v = (xv[i] - mean[c0 + i]) * is * gamma[c0 + i] + beta[c0 + i];
        o[i] = hswish(v);
    }
    reinterpret_cast<uint4*>(y)[e] = pk<T, E>(o);
}

// backward statistics: per channel sum g' and sum g' xhat with g' = dy * hardswish'(v).  Block = CV vector columns x 256 / CV row lanes over
// a chunk of rows_per rows; the row lanes are combined in a fixed order; one partial per block and channel (double).
template <typename T>
__global__ __launch_bounds__(256) void bn_hswish_bwd_stats_kernel(const T* __restrict__ dy, const T* __restrict__ x, const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, long rows, int C, int CV, long rows_per,
                                                                  double* __restrict__ part0, double* __restrict__ part1) {
    constexpr int E = EV<T>::n;
    __shared__ double sh[2][256][4];
    const int tid = threadIdx.x, tc = tid % CV, tr = tid / CV, RL = 256 / CV;
    const int cv = blockIdx.x * CV + tc, CVT = C / E;
    double a0[E], a1[E];
#pragma unroll
    for (int i = 0; i < E; ++i) { a0[i] = 0.0; a1[i] = 0.0; }
    if (cv < CVT && tr < RL) {
        float mu[E], is[E], gm[E], bt[E];
#pragma unroll
        for (int i = 0; i < E; ++i) { mu[i] = mean[cv * E + i]; is[i] = invstd[cv * E + i]; gm[i] = gamma[cv * E + i]; bt[i] = beta[cv * E + i]; }
        const long r0 = (long)blockIdx.y * rows_per, r1 = r0 + rows_per < rows ? r0 + rows_per : rows;
        for (long r = r0 + tr; r < r1; r += RL) {
            const long iv = r * CVT + cv;
            float xv[E], gv[E];
            unpk<T, E>(reinterpret_cast<const uint4*>(x)[iv], xv);
            unpk<T, E>(reinterpret_cast<const uint4*>(dy)[iv], gv);
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const float xh = (xv[i] - mu[i]) * is[i];
                const float g = hswish_grad(xh * gm[i] + bt[i], gv[i]);
                a0[i] += (double)g; a1[i] += (double)g * (double)xh;
            }
        }
    }
#pragma unroll
    for (int h = 0; h < E; h += 4) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) { sh[0][tid][i] = a0[h + i]; sh[1][tid][i] = a1[h + i]; }
        __syncthreads();
        if (tr == 0 && cv < CVT) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                double s0 = 0.0, s1 = 0.0;
                for (int k = 0; k < RL; ++k) { s0 += sh[0][k * CV + tc][i]; s1 += sh[1][k * CV + tc][i]; }
                part0[(long)blockIdx.y * C + cv * E + h + i] = s0;
                part1[(long)blockIdx.y * C + cv * E + h + i] = s1;
            }
        }
    }
}
// one thread per channel adds the partials in order: dbeta = sum g', dgamma = sum g' xhat
__global__ void bn_hswish_bwd_finalize_kernel(const double* __restrict__ part0, const double* __restrict__ part1, int nparts, int C, float* __restrict__ dbeta,
                                              float* __restrict__ dgamma) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s = 0.0, q = 0.0;
    for (int p = 0; p < nparts; ++p) { s += part0[(long)p * C + c]; q += part1[(long)p * C + c]; }
    dbeta[c] = (float)s; dgamma[c] = (float)q;
}
// dx = gamma * invstd * (g' - dbeta / M - xhat * dgamma / M)  (the association of encoder.hip's bn_bwd_apply_kernel)
template <typename T>
__global__ __launch_bounds__(256) void bn_hswish_bwd_apply_kernel(const T* __restrict__ dy, const T* __restrict__ x, const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, const float* __restrict__ dbeta,
                                                                  const float* __restrict__ dgamma, float inv_rows, T* __restrict__ dx, long totalv, int CV) {
    constexpr int E = EV<T>::n;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= totalv) return;
    const int c0 = (int)(e % CV) * E;
    float xv[E], gv[E], o[E];
    unpk<T, E>(reinterpret_cast<const uint4*>(x)[e], xv);
    unpk<T, E>(reinterpret_cast<const uint4*>(dy)[e], gv);
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const int c = c0 + i;
        const float is = invstd[c], xh = (xv[i] - mean[c]) * is;
        const float g = hswish_grad(xh * gamma[c] + beta[c], gv[i]);
        const float fa = gamma[c] * is, fb = dbeta[c] * inv_rows, fc = is * dgamma[c] * inv_rows;
        o[i] = fa * (g - fb - (xv[i] - mean[c]) * fc);
    }
    reinterpret_cast<uint4*>(dx)[e] = pk<T, E>(o);
}

// ------------------------------------------------------------------ squeeze-and-excitation
constexpr int SE_MAXC = 1024, SE_MAXS = 256;

// sum over the HW pixels of one image of f(pixel, channel) for every channel, in a fixed order: thread = (channel c0 + tid % CB, pixel lane
// tid / CB), lanes combined through LDS in lane order.  Writes out[c] (double -> float, times `scale`).
template <typename T, bool PROD>
__device__ __forceinline__ void image_colsum(const T* __restrict__ a, const T* __restrict__ b, int HW, int C, float scale, float* __restrict__ out, double* sh) {
    const int tid = threadIdx.x;
    for (int cb = 0; cb < C; cb += 64) {
        const int CB = C - cb < 64 ? C - cb : 64, lanes = 256 / CB;
        const int cl = tid % CB, ln = tid / CB, c = cb + cl;
        double s = 0.0;
        if (ln < lanes)
            for (int p = ln; p < HW; p += lanes) {
                const long i = (long)p * C + c;
                s += PROD ? (double)((float)a[i] * (float)b[i]) : (double)(float)a[i];
            }
        __syncthreads();
        sh[tid] = s;
        __syncthreads();
        if (tid < CB) {
            double t = 0.0;
            for (int l = 0; l < lanes; ++l) t += sh[l * CB + tid];
            out[cb + tid] = (float)(t * (double)scale);
        }
    }
    __syncthreads();
}

// one block per image: pool = mean_hw x; h = relu(W1 pool + b1); z2 = W2 h + b2; s = hardsigmoid(z2).  Saved: pool, h, z2, s ([N][C] / [N][S])
template <typename T>
__global__ __launch_bounds__(256) void se_fwd_image_kernel(const T* __restrict__ x, int HW, int C, int S, const float* __restrict__ w1, const float* __restrict__ b1,
                                                           const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ pool,
                                                           float* __restrict__ hsave, float* __restrict__ z2save, float* __restrict__ ssave) {
    __shared__ double sh[256];
    __shared__ float pl[SE_MAXC], hs[SE_MAXS];
    const int n = blockIdx.x, tid = threadIdx.x;
    image_colsum<T, false>(x + (long)n * HW * C, nullptr, HW, C, 1.f, pl, sh);
    // torch: adaptive_avg_pool2d = sum / HW; here the double sum is divided after rounding to float, as the mean of a float tensor
    for (int c = tid; c < C; c += 256) { pl[c] = pl[c] / (float)HW; pool[(long)n * C + c] = pl[c]; }
    __syncthreads();
    for (int j = tid; j < S; j += 256) {
        float z = 0.f;
        const float* wr = w1 + (long)j * C;
        for (int c = 0; c < C; ++c) z = fmaf(wr[c], pl[c], z);
        z += b1[j];
        const float h = z > 0.f ? z : 0.f;
        hs[j] = h; hsave[(long)n * S + j] = h;
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        float z = 0.f;
        const float* wr = w2 + (long)c * S;
        for (int j = 0; j < S; ++j) z = fmaf(wr[j], hs[j], z);
        z += b2[c];
        z2save[(long)n * C + c] = z;
        ssave[(long)n * C + c] = fminf(fmaxf(z + 3.f, 0.f), 6.f) / 6.f;
    }
}

// y = x * s[n][c] (SCALE) or dx = g * s[n][c] + dpool[n][c] / HW (backward), 16 bytes per thread
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void se_scale_kernel(const T* __restrict__ a, const float* __restrict__ s, const float* __restrict__ dpool, float inv_hw,
                                                       T* __restrict__ out, long totalv, int CV, long per_image) {
    constexpr int E = EV<T>::n;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= totalv) return;
    const long n = e / per_image;
    const long c0 = n * CV * E + (e % CV) * E;
    float v[E], o[E];
    unpk<T, E>(reinterpret_cast<const uint4*>(a)[e], v);
#pragma unroll
    for (int i = 0; i < E; ++i) o[i] = BWD ? v[i] * s[c0 + i] + dpool[c0 + i] * inv_hw : s[c0 + i] * v[i];
    reinterpret_cast<uint4*>(out)[e] = pk<T, E>(o);
}

// backward, one block per image: ds = sum_hw g x; dz2 = ds / 6 where -3 < z2 < 3 (torch's hardsigmoid_backward); dh = W2^T dz2;
// dz1 = dh where h > 0; dpool = W1^T dz1.  Saved for the weight gradients: dz2 [N][C], dz1 [N][S], dpool [N][C].
template <typename T>
__global__ __launch_bounds__(256) void se_bwd_image_kernel(const T* __restrict__ g, const T* __restrict__ x, int HW, int C, int S, const float* __restrict__ w1,
                                                           const float* __restrict__ w2, const float* __restrict__ hsave, const float* __restrict__ z2save,
                                                           float* __restrict__ dz2, float* __restrict__ dz1, float* __restrict__ dpool) {
    __shared__ double sh[256];
    __shared__ float dz[SE_MAXC], d1[SE_MAXS];
    const int n = blockIdx.x, tid = threadIdx.x;
    image_colsum<T, true>(g + (long)n * HW * C, x + (long)n * HW * C, HW, C, 1.f, dz, sh);
    for (int c = tid; c < C; c += 256) {
        const float z = z2save[(long)n * C + c];
        const float d = (z > -3.f && z < 3.f) ? dz[c] / 6.f : 0.f;
        dz[c] = d; dz2[(long)n * C + c] = d;
    }
    __syncthreads();
    for (int j = tid; j < S; j += 256) {
        float d = 0.f;
        for (int c = 0; c < C; ++c) d = fmaf(w2[(long)c * S + j], dz[c], d);
        d = hsave[(long)n * S + j] > 0.f ? d : 0.f;
        d1[j] = d; dz1[(long)n * S + j] = d;
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        float d = 0.f;
        for (int j = 0; j < S; ++j) d = fmaf(w1[(long)j * C + c], d1[j], d);
        dpool[(long)n * C + c] = d;
    }
}

// parameter gradients, one thread per element, images added in order (double): dW1[j][c] = sum dz1[n][j] pool[n][c], db1[j] = sum dz1[n][j],
// dW2[c][j] = sum dz2[n][c] h[n][j], db2[c] = sum dz2[n][c]
__global__ __launch_bounds__(256) void se_wgrad_kernel(int N, int C, int S, const float* __restrict__ pool, const float* __restrict__ hsave,
                                                       const float* __restrict__ dz2, const float* __restrict__ dz1, float* __restrict__ dw1,
                                                       float* __restrict__ db1, float* __restrict__ dw2, float* __restrict__ db2) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long n1 = (long)S * C, n2 = n1 + S, n3 = n2 + (long)C * S, n4 = n3 + C;
    if (e >= n4) return;
    double s = 0.0;
    if (e < n1) {
        const int j = (int)(e / C), c = (int)(e % C);
        for (int n = 0; n < N; ++n) s += (double)dz1[(long)n * S + j] * (double)pool[(long)n * C + c];
        dw1[e] = (float)s;
    } else if (e < n2) {
        const int j = (int)(e - n1);
        for (int n = 0; n < N; ++n) s += (double)dz1[(long)n * S + j];
        db1[j] = (float)s;
    } else if (e < n3) {
        const long o = e - n2;
        const int c = (int)(o / S), j = (int)(o % S);
        for (int n = 0; n < N; ++n) s += (double)dz2[(long)n * C + c] * (double)hsave[(long)n * S + j];
        dw2[o] = (float)s;
    } else {
        const int c = (int)(e - n3);
        for (int n = 0; n < N; ++n) s += (double)dz2[(long)n * C + c];
        db2[c] = (float)s;
    }
}

}  // namespace
}  // namespace sat

using namespace sat;

// backward statistics grid: CV = the largest divisor of 256 up to C / E; row chunks so that the partials fit the sat_bn_scratch_bytes scratch
static void hs_grid(long rows, int C, int E, int& CV, long& rows_per, int& nparts) {
    const int CVT = C / E;
    CV = CVT < 256 ? CVT : 256;
    while (256 % CV) --CV;
    const int RL = 256 / CV, colblocks = cdiv(CVT, CV);
    long want = 512 / colblocks; if (want < 1) want = 1;
    const long cap = ((long)sat_bn_scratch_bytes(rows, C) - 64) / ((long)C * 2 * (long)sizeof(double));
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    rows_per = cdiv(rows, want);
    const long minrows = (long)RL * 8;
    if (rows_per < minrows) rows_per = minrows;
    nparts = cdiv(rows, rows_per);
}

template <typename T>
static int bn_hswish_bwd(const T* dy, const T* x, long rows, int C, const float* mean, const float* invstd, const float* gamma, const float* beta, T* dx,
                         float* dgamma, float* dbeta, float* scratch, hipStream_t st) {
    constexpr int E = EV<T>::n;
    int CV, nparts; long rp;
    hs_grid(rows, C, E, CV, rp, nparts);
    double* p0 = reinterpret_cast<double*>(scratch); double* p1 = p0 + (long)nparts * C;
    hipLaunchKernelGGL(bn_hswish_bwd_stats_kernel<T>, dim3(cdiv(C / E, CV), nparts), dim3(256), 0, st, dy, x, mean, invstd, gamma, beta, rows, C, CV, rp, p0, p1);
    SAT_TRY(launch_ok("bn_hswish_bwd_stats"));
    hipLaunchKernelGGL(bn_hswish_bwd_finalize_kernel, dim3(cdiv(C, 256)), dim3(256), 0, st, p0, p1, nparts, C, dbeta, dgamma);
    SAT_TRY(launch_ok("bn_hswish_bwd_finalize"));
    const long totalv = rows * (C / E);
    hipLaunchKernelGGL(bn_hswish_bwd_apply_kernel<T>, dim3(cdiv(totalv, 256)), dim3(256), 0, st, dy, x, mean, invstd, gamma, beta, dbeta, dgamma, 1.0f / (float)rows, dx,
                       totalv, C / E);
    return launch_ok("bn_hswish_bwd_apply");
}

static int hs_shape(int32_t dtype, int64_t rows, int32_t C, const char* what) {
    SAT_REQUIRE(dtype == 0 || dtype == 1, "%s: dtype %d (0 = fp32, 1 = bf16)", what, dtype);
    const int E = dtype ? 8 : 4;
    SAT_REQUIRE(rows > 0 && C > 0 && C % E == 0, "%s: rows=%ld C=%d (C must be a multiple of %d for this storage type)", what, (long)rows, C, E);
    SAT_REQUIRE(rows * (C / E) < (1L << 40), "%s: tensor too large", what);
    return SAT_OK;
}

static int se_shape(int32_t dtype, int32_t N, int32_t HW, int32_t C, int32_t S, const char* what) {
    SAT_REQUIRE(dtype == 0 || dtype == 1, "%s: dtype %d (0 = fp32, 1 = bf16)", what, dtype);
    const int E = dtype ? 8 : 4;
    SAT_REQUIRE(N > 0 && HW > 0 && C > 0 && S > 0 && C % E == 0 && C <= SE_MAXC && S <= SE_MAXS,
                "%s: N=%d HW=%d C=%d S=%d (C a multiple of %d, C <= %d, S <= %d)", what, N, HW, C, S, E, SE_MAXC, SE_MAXS);
    return SAT_OK;
}

extern "C" {

int sat_bn_hswish_train_fwd_t(int32_t dtype, const void* x, int64_t rows, int32_t C, const float* tile_stats, int32_t tile_rows, const float* gamma,
                              const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* save_mean, float* save_invstd,
                              void* y, float* scratch, void* stream) {
    if (!x || !gamma || !beta || !save_mean || !save_invstd || !y || !scratch) return fail(SAT_EINVAL, "bn_hswish_train_fwd: null pointer");
    SAT_TRY(hs_shape(dtype, rows, C, "bn_hswish_train_fwd"));
    if (tile_stats) {          // statistics from the producing convolution's epilogue (bf16 storage)
        SAT_REQUIRE(dtype == 1 && tile_rows > 0, "bn_hswish_train_fwd: tile statistics need bf16 storage and tile_rows > 0 (tile_rows=%d)", tile_rows);
        SAT_TRY(sat_bn_train_fwd_tiles_bf16(x, rows, C, tile_stats, tile_rows, gamma, beta, eps, momentum, running_mean, running_var, save_mean, save_invstd,
                                            nullptr, 0, nullptr, nullptr, scratch, stream));
    } else
        SAT_TRY(sat_bn_train_fwd_t(dtype, x, rows, C, gamma, beta, eps, momentum, running_mean, running_var, save_mean, save_invstd, nullptr, 0, nullptr, nullptr,
                                   scratch, stream));
    const int E = dtype ? 8 : 4;
    const long totalv = rows * (C / E);
    if (dtype) hipLaunchKernelGGL((bn_hswish_apply_kernel<bf, false>), dim3(cdiv(totalv, 256)), dim3(256), 0, (hipStream_t)stream, (const bf*)x, save_mean, save_invstd,
                                  gamma, beta, (bf*)y, totalv, C / E, 0.f);
    else hipLaunchKernelGGL((bn_hswish_apply_kernel<float, false>), dim3(cdiv(totalv, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)x, save_mean, save_invstd,
                            gamma, beta, (float*)y, totalv, C / E, 0.f);
    return launch_ok("bn_hswish_apply");
}

int sat_bn_hswish_eval_fwd_t(int32_t dtype, const void* x, int64_t rows, int32_t C, const float* running_mean, const float* running_var, float eps,
                             const float* gamma, const float* beta, void* y, void* stream) {
    if (!x || !running_mean || !running_var || !gamma || !beta || !y) return fail(SAT_EINVAL, "bn_hswish_eval_fwd: null pointer");
    SAT_TRY(hs_shape(dtype, rows, C, "bn_hswish_eval_fwd"));
    SAT_REQUIRE(eps >= 0.f, "bn_hswish_eval_fwd: eps < 0");
    const int E = dtype ? 8 : 4;
    const long totalv = rows * (C / E);
    if (dtype) hipLaunchKernelGGL((bn_hswish_apply_kernel<bf, true>), dim3(cdiv(totalv, 256)), dim3(256), 0, (hipStream_t)stream, (const bf*)x, running_mean, running_var,
                                  gamma, beta, (bf*)y, totalv, C / E, eps);
    else hipLaunchKernelGGL((bn_hswish_apply_kernel<float, true>), dim3(cdiv(totalv, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)x, running_mean, running_var,
                            gamma, beta, (float*)y, totalv, C / E, eps);
    return launch_ok("bn_hswish_apply(eval)");
}

int sat_bn_hswish_train_bwd_t(int32_t dtype, const void* dy, const void* x, int64_t rows, int32_t C, const float* save_mean, const float* save_invstd,
                              const float* gamma, const float* beta, void* dx, float* dgamma, float* dbeta, float* scratch, void* stream) {
    if (!dy || !x || !save_mean || !save_invstd || !gamma || !beta || !dx || !dgamma || !dbeta || !scratch) return fail(SAT_EINVAL, "bn_hswish_train_bwd: null pointer");
    SAT_TRY(hs_shape(dtype, rows, C, "bn_hswish_train_bwd"));
    if (dtype) return bn_hswish_bwd<bf>((const bf*)dy, (const bf*)x, rows, C, save_mean, save_invstd, gamma, beta, (bf*)dx, dgamma, dbeta, scratch, (hipStream_t)stream);
    return bn_hswish_bwd<float>((const float*)dy, (const float*)x, rows, C, save_mean, save_invstd, gamma, beta, (float*)dx, dgamma, dbeta, scratch, (hipStream_t)stream);
}

int sat_se_fwd_t(int32_t dtype, const void* x, int32_t N, int32_t HW, int32_t C, int32_t S, const float* w1, const float* b1, const float* w2, const float* b2,
                 float* pool, float* h, float* z2, float* s, void* y, void* stream) {
    if (!x || !w1 || !b1 || !w2 || !b2 || !pool || !h || !z2 || !s || !y) return fail(SAT_EINVAL, "se_fwd: null pointer");
    SAT_TRY(se_shape(dtype, N, HW, C, S, "se_fwd"));
    hipStream_t st = (hipStream_t)stream;
    const int E = dtype ? 8 : 4;
    const long per = (long)HW * (C / E), totalv = (long)N * per;
    if (dtype) {
        hipLaunchKernelGGL(se_fwd_image_kernel<bf>, dim3(N), dim3(256), 0, st, (const bf*)x, HW, C, S, w1, b1, w2, b2, pool, h, z2, s);
        SAT_TRY(launch_ok("se_fwd_image"));
        hipLaunchKernelGGL((se_scale_kernel<bf, false>), dim3(cdiv(totalv, 256)), dim3(256), 0, st, (const bf*)x, s, nullptr, 0.f, (bf*)y, totalv, C / E, per);
    } else {
        hipLaunchKernelGGL(se_fwd_image_kernel<float>, dim3(N), dim3(256), 0, st, (const float*)x, HW, C, S, w1, b1, w2, b2, pool, h, z2, s);
        SAT_TRY(launch_ok("se_fwd_image"));
        hipLaunchKernelGGL((se_scale_kernel<float, false>), dim3(cdiv(totalv, 256)), dim3(256), 0, st, (const float*)x, s, nullptr, 0.f, (float*)y, totalv, C / E, per);
    }
    return launch_ok("se_scale");
}

size_t sat_se_bwd_scratch_bytes(int32_t N, int32_t C, int32_t S) {
    if (N <= 0 || C <= 0 || S <= 0) return 0;
    return (size_t)N * (2 * (size_t)C + (size_t)S) * sizeof(float);
}

int sat_se_bwd_t(int32_t dtype, const void* dy, const void* x, int32_t N, int32_t HW, int32_t C, int32_t S, const float* w1, const float* w2, const float* pool,
                 const float* h, const float* z2, const float* s, void* dx, float* dw1, float* db1, float* dw2, float* db2, float* scratch, void* stream) {
    if (!dy || !x || !w1 || !w2 || !pool || !h || !z2 || !s || !dx || !dw1 || !db1 || !dw2 || !db2 || !scratch) return fail(SAT_EINVAL, "se_bwd: null pointer");
    SAT_TRY(se_shape(dtype, N, HW, C, S, "se_bwd"));
    hipStream_t st = (hipStream_t)stream;
    float* dz2 = scratch; float* dpool = dz2 + (long)N * C; float* dz1 = dpool + (long)N * C;
    const int E = dtype ? 8 : 4;
    const long per = (long)HW * (C / E), totalv = (long)N * per;
    if (dtype) hipLaunchKernelGGL(se_bwd_image_kernel<bf>, dim3(N), dim3(256), 0, st, (const bf*)dy, (const bf*)x, HW, C, S, w1, w2, h, z2, dz2, dz1, dpool);
    else hipLaunchKernelGGL(se_bwd_image_kernel<float>, dim3(N), dim3(256), 0, st, (const float*)dy, (const float*)x, HW, C, S, w1, w2, h, z2, dz2, dz1, dpool);
    SAT_TRY(launch_ok("se_bwd_image"));
    const long nw = 2L * S * C + S + C;
    hipLaunchKernelGGL(se_wgrad_kernel, dim3(cdiv(nw, 256)), dim3(256), 0, st, N, C, S, pool, h, dz2, dz1, dw1, db1, dw2, db2);
    SAT_TRY(launch_ok("se_wgrad"));
    if (dtype) hipLaunchKernelGGL((se_scale_kernel<bf, true>), dim3(cdiv(totalv, 256)), dim3(256), 0, st, (const bf*)dy, s, dpool, 1.f / (float)HW, (bf*)dx, totalv, C / E, per);
    else hipLaunchKernelGGL((se_scale_kernel<float, true>), dim3(cdiv(totalv, 256)), dim3(256), 0, st, (const float*)dy, s, dpool, 1.f / (float)HW, (float*)dx, totalv, C / E, per);
    return launch_ok("se_dx");
}

}
