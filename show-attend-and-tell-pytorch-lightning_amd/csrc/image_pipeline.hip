// Input pipeline on device: a ragged batch of decoded uint8 RGB pictures -> the (B, 3, S, S) fp32 batch the
// reference's DataLoader hands to SAT.train_batch.
// Reference: train.py:208-233 composes, per picture, T.RandomResizedCrop | T.Resize + T.CenterCrop, T.RandomHorizontalFlip,
// T.ToTensor and util.py:121-130 AddGaussianNoise.  On PIL images torchvision's resize is Pillow's Image.resize(BILINEAR): a
// separable, antialiased (support scaled by the shrink factor) triangle filter evaluated in 8-bit fixed point, horizontal pass
// first, each pass rounded and clipped to bytes.  The kernels of pillow_resample.h (shared with the BICUBIC path of
// attention_panels.hip) compute exactly those bytes (22-bit coefficients from double-precision weights, the same rounding), then
// byte/255 in fp32 and + noise * std.
// Byte work, HBM/L2 bound: one read of the source box, a 4-byte-per-pixel intermediate, one fp32 write.
// ColorJitter (train.py:223-224, on the mirrored bytes before ToTensor): the vertical-pass kernel applies the adjustments in front of
// contrast and leaves the bytes plus each picture's luma sum in the workspace; a second kernel applies contrast (a blend with the
// picture's mean luma, which needs the whole picture) and the adjustments after it, then ToTensor and noise.
// Optical augmentation (train.py:225-231, after ColorJitter): the last byte stage writes its bytes to the workspace instead of
// finishing, and one more kernel warps them (Pillow's fixed-point affine NEAREST or double perspective BILINEAR sampling, fill 0),
// then ToTensor and noise.
#include "pillow_resample.h"

// Every floating-point operation in this file must round on its own, as the host code it reproduces does: the Makefile
// compiles it with -ffp-contract=off (hipcc's default lets the backend fuse a product with a following sum whatever the
// source says - hip's __fmul_rn / __fadd_rn are plain inline operators and fuse too).  Plain operators below.
#pragma clang fp contract(off)

namespace sat {

// the resample itself (coefficient tables, the two passes, ToTensor + noise) is pillow_resample.h, here with the triangle filter and
// every number of the geometry read from the descriptor
struct DescGeometry {
    static constexpr int TABLES = 2;
    static __device__ ResampleGeometry of(const sat_image_desc& d, int, int) {
        return {d.crop_top, d.crop_left, d.crop_h, d.crop_w, d.resized_h, d.resized_w, d.out_top, d.out_left, d.flip};
    }
};


// ---------------------------------------------------------------------------------------------------------------------------------
// ColorJitter (train.py:223-224, torchvision's functional_pil): every step is Pillow's C arithmetic on bytes, reproduced operation for
// operation (float where Pillow computes in float, double where a double literal promotes, each operation rounded on its own).
enum : int { CJ_BRIGHTNESS = 0, CJ_CONTRAST = 1, CJ_SATURATION = 2, CJ_HUE = 3 };

// Image.convert("L"): ITU-R 601-2 luma in 16-bit fixed point
__device__ inline int luma8(const int v[3]) { return (v[0] * 19595 + v[1] * 38470 + v[2] * 7471 + 0x8000) >> 16; }

// Image.blend(degenerate, image, f) per byte: d + f * (x - d) in float, truncated and clipped to a byte
__device__ inline int blend8(int d, int x, float f) {
    const float t = (float)d + f * ((float)x - (float)d);
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

// Image.convert("HSV") (Pillow's rgb2hsv)
__device__ inline void rgb_to_hsv8(const int v[3], int& H, int& S, int& V) {
    const int r = v[0], g = v[1], b = v[2];
    const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
    V = mx;
    if (mx == mn) { H = 0; S = 0; return; }
    const float cr = (float)(mx - mn);
    const float s = (float)(mx - mn) / (float)mx;
    const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
    float h;
    if (r == mx) h = bc - gc;
    else if (g == mx) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    // Pillow: fmod(h / 6.0 + 1.0, 1.0).  h lies in [-1, 5], so the argument lies in [5/6, 11/6) and fmod is a subtraction of 1,
    // exact there (Sterbenz)
    const double a = (double)h / 6.0 + 1.0;
    h = (float)(a >= 1.0 ? a - 1.0 : a);
    const int hi = (int)((double)h * 255.0), si = (int)((double)s * 255.0);
    H = hi < 0 ? 0 : (hi > 255 ? 255 : hi);
    S = si < 0 ? 0 : (si > 255 ? 255 : si);
}

__device__ inline int round8(double x) {
    const int r = (int)round(x);                        // half away from zero, as C's round()
    return r < 0 ? 0 : (r > 255 ? 255 : r);
}

// Image.convert("RGB") of HSV bytes (Pillow's hsv2rgb)
__device__ inline void hsv_to_rgb8(int H, int S, int V, int v[3]) {
    if (S == 0) { v[0] = v[1] = v[2] = V; return; }
    const double hx = (double)(float)H * 6.0 / 255.0;
    const int i = (int)floor(hx);
    const float f = (float)(hx - (double)(float)i);
    const float fs = (float)((double)(float)S / 255.0);
    const double vv = (double)(float)V;
    const int p = round8(vv * (1.0 - (double)fs));
    const int q = round8(vv * (1.0 - (double)(fs * f)));
    const int t = round8(vv * (1.0 - (double)fs * (1.0 - (double)f)));
    switch (i % 6) {
        case 0: v[0] = V; v[1] = t; v[2] = p; break;
        case 1: v[0] = q; v[1] = V; v[2] = p; break;
        case 2: v[0] = p; v[1] = V; v[2] = t; break;
        case 3: v[0] = p; v[1] = q; v[2] = V; break;
        case 4: v[0] = t; v[1] = p; v[2] = V; break;
        default: v[0] = V; v[1] = p; v[2] = q; break;
    }
}

// one adjustment other than contrast, in place
__device__ inline void jitter_op(int op, const sat_image_jitter& j, int v[3]) {
    if (op == CJ_BRIGHTNESS) {                          // ImageEnhance.Brightness: degenerate = black
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = blend8(0, v[c], j.brightness);
    } else if (op == CJ_SATURATION) {                   // ImageEnhance.Color: degenerate = the picture's own luma
        const int l = luma8(v);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = blend8(l, v[c], j.saturation);
    } else {                                            // F_pil.adjust_hue: H + shift as a wrapping byte
        int H, S, V;
        rgb_to_hsv8(v, H, S, V);
        hsv_to_rgb8((H + j.hue_shift) & 255, S, V, v);
    }
}

// vertical pass + flip + the adjustments in front of contrast.  The bytes go to `pre` (output layout, mirrored), and each picture's
// luma sum - what ImageEnhance.Contrast averages - to sums[img]: one 64-bit integer atomic per block, so the sum is exact and does
// not depend on the order of arrival.
__global__ __launch_bounds__(256) void resample_cols_jitter_kernel(const sat_image_desc* __restrict__ desc, const sat_image_jitter* __restrict__ jit,
                                                                   int out_h, int out_w, int omax, int KT, int hmax, const int* __restrict__ bounds,
                                                                   const int* __restrict__ coeffs, const uchar4* __restrict__ tmp,
                                                                   uchar4* __restrict__ pre, unsigned long long* __restrict__ sums) {
    __shared__ int part[4];
    const int img = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    int l = 0;
    if (x < out_w && y < out_h) {
        const sat_image_desc d = desc[img];
        const sat_image_jitter j = jit[img];
        int v[3];
        resample_col<DescGeometry>(img, x, y, omax, KT, hmax, out_w, bounds, coeffs, tmp, v);
        for (int k = 0; k < 4 && j.order[k] != CJ_CONTRAST; ++k) jitter_op(j.order[k], j, v);
        pre[((long)img * out_h + y) * out_w + (d.flip ? out_w - 1 - x : x)] = make_uchar4((unsigned char)v[0], (unsigned char)v[1], (unsigned char)v[2], 0);
        l = luma8(v);
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) l += __shfl_xor(l, m, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = l;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sums + img, (unsigned long long)(part[0] + part[1] + part[2] + part[3]));
}

// contrast against the picture's mean luma, the adjustments after it, ToTensor + noise; one thread per output pixel
__global__ __launch_bounds__(256) void color_jitter_finish_kernel(const sat_image_jitter* __restrict__ jit, int out_h, int out_w,
                                                                  const uchar4* __restrict__ pre, const unsigned long long* __restrict__ sums,
                                                                  const float* __restrict__ noise, float noise_std, float* __restrict__ out,
                                                                  uint8_t* __restrict__ out_u8) {
    const int img = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= out_w || y >= out_h) return;
    const sat_image_jitter j = jit[img];
    // ImageEnhance.Contrast: degenerate = int(ImageStat mean of L + 0.5), the mean an exact integer sum over the pixel count
    const int mean = (int)((double)sums[img] / (double)((long)out_h * out_w) + 0.5);
    const uchar4 p = pre[((long)img * out_h + y) * out_w + x];
    int v[3] = {p.x, p.y, p.z};
    int k = 0;
    while (k < 3 && j.order[k] != CJ_CONTRAST) ++k;     // the order is a permutation (validated on the host)
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = blend8(mean, v[c], j.contrast);
    for (++k; k < 4; ++k) jitter_op(j.order[k], j, v);
    finish_pixel(v, img, y, x, out_h, out_w, noise, noise_std, out, out_u8);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The "optical" augmentation (train.py:225-231: RandomPerspective | RandomAffine | RandomRotation on the S x S picture after
// ColorJitter): Pillow's Image.transform of the picture onto itself with fill 0.  The record holds Pillow's inverse map.

// RandomAffine / RandomRotation: Pillow's affine_fixed (NEAREST).  16.16 fixed point; the closed form below is Pillow's running
// sums (xx += a0 along a row, a2 += a1 per row) evaluated modulo 2^32, as its int32 sums are.
__device__ inline int fix16(double v) { return (int)floor(v * 65536.0 + 0.5); }

__device__ inline void warp_affine_nearest(const double c[8], int x, int y, int W, int H, const uint8_t* __restrict__ pic, int v[3]) {
    const unsigned a0 = (unsigned)fix16(c[0]), a1 = (unsigned)fix16(c[1]), a3 = (unsigned)fix16(c[3]), a4 = (unsigned)fix16(c[4]);
    const unsigned a2 = (unsigned)fix16(c[2] + c[0] * 0.5 + c[1] * 0.5);
    const unsigned a5 = (unsigned)fix16(c[5] + c[3] * 0.5 + c[4] * 0.5);
    const int xin = (int)(a2 + (unsigned)y * a1 + (unsigned)x * a0) >> 16;
    const int yin = (int)(a5 + (unsigned)y * a4 + (unsigned)x * a3) >> 16;
    if (xin >= 0 && xin < W && yin >= 0 && yin < H) {
        const uint8_t* p = pic + ((long)yin * W + xin) * 3;
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
    }
}

// RandomPerspective: Pillow's generic transform with perspective_transform and bilinear_filter32RGB, all in double.  A point
// outside the picture (or a NaN from a zero denominator) is fill; the column and row indices are clamped, so no read leaves it.
__device__ inline void warp_perspective_bilinear(const double c[8], int x, int y, int W, int H, const uint8_t* __restrict__ pic, int v[3]) {
    const double xi = (double)x + 0.5, yi = (double)y + 0.5;
    const double den = c[6] * xi + c[7] * yi + 1.0;
    double xo = (c[0] * xi + c[1] * yi + c[2]) / den;
    double yo = (c[3] * xi + c[4] * yi + c[5]) / den;
    if (!(xo >= 0.0 && xo < (double)W && yo >= 0.0 && yo < (double)H)) return;
    xo -= 0.5;
    yo -= 0.5;
    const double fx = floor(xo), fy = floor(yo);
    const double dx = xo - fx, dy = yo - fy;
    const int ix = (int)fx, iy = (int)fy;                                    // in [-1, W - 1] and [-1, H - 1]
    const int x0 = min(max(ix, 0), W - 1), x1 = min(max(ix + 1, 0), W - 1);
    const int y0 = min(max(iy, 0), H - 1), y1 = iy + 1;
    const bool row2 = y1 >= 0 && y1 < H;
    const uint8_t* r0 = pic + (long)y0 * W * 3;
    const uint8_t* r1 = pic + (long)(row2 ? y1 : y0) * W * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int p0 = r0[x0 * 3 + k], p1 = r0[x1 * 3 + k];
        const double v1 = (double)p0 + (double)(p1 - p0) * dx;              // BILINEAR(v, a, b, d): a + (b - a) * d
        double v2 = v1;
        if (row2) {
            const int q0 = r1[x0 * 3 + k], q1 = r1[x1 * 3 + k];
            v2 = (double)q0 + (double)(q1 - q0) * dx;
        }
        v[k] = (int)(v1 + (v2 - v1) * dy);                                   // (UINT8) v: truncated, in [0, 255]
    }
}

// warp of the byte stage's output `src` (n, H, W, 3) + ToTensor + noise; one thread per output pixel
__global__ __launch_bounds__(256) void warp_finish_kernel(const sat_image_warp* __restrict__ warp, int out_h, int out_w, const uint8_t* __restrict__ src,
                                                          const float* __restrict__ noise, float noise_std, float* __restrict__ out,
                                                          uint8_t* __restrict__ out_u8) {
    const int img = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= out_w || y >= out_h) return;
    const sat_image_warp w = warp[img];
    const uint8_t* pic = src + (long)img * out_h * out_w * 3;
    int v[3] = {0, 0, 0};                                                    // fillcolor (0, 0, 0)
    if (w.kind == 0) warp_affine_nearest(w.coeffs, x, y, out_w, out_h, pic, v);
    else warp_perspective_bilinear(w.coeffs, x, y, out_w, out_h, pic, v);
    finish_pixel(v, img, y, x, out_h, out_w, noise, noise_std, out, out_u8);
}

struct ImagePlan : ResamplePlan { size_t pre_off, sums_off, warp_off; };

// jit (host, or NULL: no ColorJitter) adds the jitter checks and the workspace of the two jitter kernels; warp (host, or NULL: no
// optical augmentation) adds the warp checks and the bytes in front of the warp
static int image_plan(const sat_image_desc* d, const sat_image_jitter* jit, const sat_image_warp* warp, int n, int64_t pixels_bytes, int out_h,
                      int out_w, ImagePlan* p) {
    SAT_REQUIRE(n > 0 && out_h > 0 && out_w > 0, "image_batch: n=%d out=%dx%d", n, out_h, out_w);
    int KT = 3, hmax = 1;
    for (int i = 0; i < n; ++i) {
        const sat_image_desc& e = d[i];
        SAT_TRY(picture_in_buffer("image_batch", i, e, pixels_bytes));
        SAT_REQUIRE(e.crop_h > 0 && e.crop_w > 0 && e.crop_top >= 0 && e.crop_left >= 0 && e.crop_top + e.crop_h <= e.height && e.crop_left + e.crop_w <= e.width,
                    "image_batch: picture %d crop box (%d,%d,%d,%d) outside %dx%d", i, e.crop_top, e.crop_left, e.crop_h, e.crop_w, e.height, e.width);
        SAT_REQUIRE(e.resized_h > 0 && e.resized_w > 0 && e.out_top >= 0 && e.out_left >= 0 && e.out_top + out_h <= e.resized_h && e.out_left + out_w <= e.resized_w,
                    "image_batch: picture %d output window (%d,%d)+%dx%d outside the resampled %dx%d", i, e.out_top, e.out_left, out_h, out_w, e.resized_h, e.resized_w);
        const int kh = resample_taps<Bilinear>(e.crop_h, e.resized_h), kw = resample_taps<Bilinear>(e.crop_w, e.resized_w);
        const int k = kh > kw ? kh : kw;
        SAT_REQUIRE(k <= RS_MAX_TAPS, "image_batch: picture %d shrinks by more than 64x", i);
        if (k > KT) KT = k;
        if (e.crop_h > hmax) hmax = e.crop_h;
        if (jit) {
            const sat_image_jitter& j = jit[i];
            int seen = 0;
            for (int k = 0; k < 4; ++k) seen |= (j.order[k] >= 0 && j.order[k] < 4) ? 1 << j.order[k] : 16;
            SAT_REQUIRE(seen == 15, "image_batch: picture %d jitter order (%d,%d,%d,%d) is not a permutation of 0..3", i, j.order[0], j.order[1],
                        j.order[2], j.order[3]);
            SAT_REQUIRE(std::isfinite(j.brightness) && std::isfinite(j.contrast) && std::isfinite(j.saturation) && j.brightness >= 0.0f &&
                        j.contrast >= 0.0f && j.saturation >= 0.0f,
                        "image_batch: picture %d jitter factors (%g, %g, %g) must be finite and >= 0", i, (double)j.brightness, (double)j.contrast,
                        (double)j.saturation);
            SAT_REQUIRE(j.hue_shift >= -128 && j.hue_shift <= 127, "image_batch: picture %d hue shift %d outside [-128, 127]", i, j.hue_shift);
        }
        if (warp) {
            const sat_image_warp& w = warp[i];
            SAT_REQUIRE(w.kind == 0 || w.kind == 1, "image_batch: picture %d warp kind %d is neither 0 (affine) nor 1 (perspective)", i, w.kind);
            const double* c = w.coeffs;
            for (int k = 0; k < (w.kind == 0 ? 6 : 8); ++k)
                SAT_REQUIRE(std::isfinite(c[k]), "image_batch: picture %d warp coefficient %d is not finite (%g)", i, k, c[k]);
            if (w.kind == 0) {
                // Pillow's check_fixed at the four corners: where it fails Pillow samples in double, which is not restated here
                const int cx[4] = {0, out_w, 0, out_w}, cy[4] = {0, 0, out_h, out_h};
                for (int k = 0; k < 4; ++k) {
                    const double xs = cx[k] * c[0] + cy[k] * c[1] + c[2], ys = cx[k] * c[3] + cy[k] * c[4] + c[5];
                    SAT_REQUIRE(std::fabs(xs) < 32768.0 && std::fabs(ys) < 32768.0,
                                "image_batch: picture %d affine warp maps corner (%d,%d) to (%g,%g), outside the fixed-point range |v| < 32768", i,
                                cx[k], cy[k], xs, ys);
                }
            }
        }
    }
    p->KT = KT; p->hmax = hmax; p->omax = out_h > out_w ? out_h : out_w;
    Workspace ws;
    carve_resample<DescGeometry>(ws, p, n, out_w);
    p->pre_off = jit ? ws.take((size_t)n * out_h * out_w * sizeof(uchar4)) : 0;
    p->sums_off = jit ? ws.take((size_t)n * sizeof(unsigned long long)) : 0;
    p->warp_off = warp ? ws.take((size_t)n * out_h * out_w * 3) : 0;
    p->total = ws.total;
    return SAT_OK;
}

}  // namespace sat
using namespace sat;

extern "C" {

size_t sat_image_batch_workspace_bytes(const sat_image_desc* desc_host, int32_t n, int32_t out_h, int32_t out_w) {
    if (!desc_host) { fail(SAT_EINVAL, "image_batch: null descriptors"); return 0; }
    ImagePlan p;
    if (image_plan(desc_host, nullptr, nullptr, n, -1, out_h, out_w, &p) != SAT_OK) return 0;
    return p.total;
}

size_t sat_image_batch_jitter_workspace_bytes(const sat_image_desc* desc_host, const sat_image_jitter* jitter_host, int32_t n, int32_t out_h,
                                              int32_t out_w) {
    if (!desc_host) { fail(SAT_EINVAL, "image_batch: null descriptors"); return 0; }
    ImagePlan p;
    if (image_plan(desc_host, jitter_host, nullptr, n, -1, out_h, out_w, &p) != SAT_OK) return 0;
    return p.total;
}

size_t sat_image_batch_warp_workspace_bytes(const sat_image_desc* desc_host, const sat_image_jitter* jitter_host, const sat_image_warp* warp_host,
                                            int32_t n, int32_t out_h, int32_t out_w) {
    if (!desc_host) { fail(SAT_EINVAL, "image_batch: null descriptors"); return 0; }
    ImagePlan p;
    if (image_plan(desc_host, jitter_host, warp_host, n, -1, out_h, out_w, &p) != SAT_OK) return 0;
    return p.total;
}

int sat_image_batch_transform(const uint8_t* pixels, int64_t pixels_bytes, const sat_image_desc* desc_host, const sat_image_desc* desc_dev, int32_t n,
                              int32_t out_h, int32_t out_w, const float* noise, float noise_std, float* out_nchw, uint8_t* out_u8,
                              void* workspace, size_t workspace_bytes, void* stream) {
    return sat_image_batch_transform_jitter(pixels, pixels_bytes, desc_host, desc_dev, nullptr, nullptr, n, out_h, out_w, noise, noise_std, out_nchw,
                                            out_u8, workspace, workspace_bytes, stream);
}

int sat_image_batch_transform_jitter(const uint8_t* pixels, int64_t pixels_bytes, const sat_image_desc* desc_host, const sat_image_desc* desc_dev,
                                     const sat_image_jitter* jitter_host, const sat_image_jitter* jitter_dev, int32_t n, int32_t out_h,
                                     int32_t out_w, const float* noise, float noise_std, float* out_nchw, uint8_t* out_u8, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    return sat_image_batch_transform_warp(pixels, pixels_bytes, desc_host, desc_dev, jitter_host, jitter_dev, nullptr, nullptr, n, out_h, out_w, noise,
                                          noise_std, out_nchw, out_u8, workspace, workspace_bytes, stream);
}

int sat_image_batch_transform_warp(const uint8_t* pixels, int64_t pixels_bytes, const sat_image_desc* desc_host, const sat_image_desc* desc_dev,
                                   const sat_image_jitter* jitter_host, const sat_image_jitter* jitter_dev, const sat_image_warp* warp_host,
                                   const sat_image_warp* warp_dev, int32_t n, int32_t out_h, int32_t out_w, const float* noise, float noise_std,
                                   float* out_nchw, uint8_t* out_u8, void* workspace, size_t workspace_bytes, void* stream) {
    if (!pixels || !desc_host || !desc_dev || !workspace || (!out_nchw && !out_u8)) return fail(SAT_EINVAL, "image_batch: null pointer");
    if (!jitter_host != !jitter_dev) return fail(SAT_EINVAL, "image_batch: jitter records given in %s memory only", jitter_host ? "host" : "device");
    if (!warp_host != !warp_dev) return fail(SAT_EINVAL, "image_batch: warp records given in %s memory only", warp_host ? "host" : "device");
    ImagePlan p;
    SAT_TRY(image_plan(desc_host, jitter_host, warp_host, n, pixels_bytes, out_h, out_w, &p));
    SAT_REQUIRE(workspace_bytes >= p.total, "image_batch: workspace %zu < %zu bytes", workspace_bytes, p.total);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int* bounds = (int*)(ws + p.bounds_off);
    int* coeffs = (int*)(ws + p.coeffs_off);
    uchar4* tmp = (uchar4*)(ws + p.tmp_off);
    // with a warp the last byte stage writes its bytes (no ToTensor, no noise) to the workspace, and the warp kernel finishes
    uint8_t* warp_src = warp_host ? (uint8_t*)(ws + p.warp_off) : nullptr;
    const float* stage_noise = warp_host ? nullptr : noise;
    float* stage_out = warp_host ? nullptr : out_nchw;
    uint8_t* stage_u8 = warp_host ? warp_src : out_u8;
    SAT_TRY((launch_resample_rows<Bilinear, DescGeometry>(st, pixels, desc_dev, n, out_h, out_w, p, ws)));
    if (jitter_host) {
        uchar4* pre = (uchar4*)(ws + p.pre_off);
        unsigned long long* sums = (unsigned long long*)(ws + p.sums_off);
        SAT_TRY(dev_fill_bytes(st, sums, 0, (size_t)n * sizeof(unsigned long long)));
        hipLaunchKernelGGL(resample_cols_jitter_kernel, dim3((out_w + 63) / 64, (out_h + 3) / 4, n), dim3(256), 0, st, desc_dev, jitter_dev, out_h, out_w,
                           p.omax, p.KT, p.hmax, bounds, coeffs, tmp, pre, sums);
        SAT_TRY(launch_ok("resample_cols_jitter"));
        hipLaunchKernelGGL(color_jitter_finish_kernel, dim3((out_w + 63) / 64, (out_h + 3) / 4, n), dim3(256), 0, st, jitter_dev, out_h, out_w, pre, sums,
                           stage_noise, noise_std, stage_out, stage_u8);
        SAT_TRY(launch_ok("color_jitter_finish"));
    } else {
        hipLaunchKernelGGL(resample_cols_finish_kernel<DescGeometry>, dim3((out_w + 63) / 64, (out_h + 3) / 4, n), dim3(256), 0, st, desc_dev, out_h, out_w, p.omax, p.KT,
                           p.hmax, bounds, coeffs, tmp, stage_noise, noise_std, stage_out, stage_u8);
        SAT_TRY(launch_ok("resample_cols_finish"));
    }
    if (!warp_host) return SAT_OK;
    hipLaunchKernelGGL(warp_finish_kernel, dim3((out_w + 63) / 64, (out_h + 3) / 4, n), dim3(256), 0, st, warp_dev, out_h, out_w, warp_src, noise, noise_std,
                       out_nchw, out_u8);
    return launch_ok("warp_finish");
}

}
