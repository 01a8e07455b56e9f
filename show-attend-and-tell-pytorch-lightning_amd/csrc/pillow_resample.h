// Pillow's Resample.c for 8-bit pixels, stated once: a separable, antialiased (support scaled by the shrink factor) filter evaluated in
// fixed point - 22-bit integer coefficients from double-precision weights, horizontal pass first, each pass rounded and clipped to
// bytes.  image_pipeline.hip instantiates it for BILINEAR and the descriptor's geometry (sat_image_batch_transform*),
// attention_panels.hip for BICUBIC and the centred square (sat_image_square_bicubic, and the tables of sat_attention_panels).
// A filter is a support and a weight function; a geometry is a struct with
//   static constexpr int TABLES                                   2: a table per axis and picture;  1: one table serves both axes
//   static __device__ ResampleGeometry of(const sat_image_desc&, int out_h, int out_w)
#pragma once
#include "../../include/sat_hip.h"
#include "common.h"

#include <cmath>

// Every floating-point operation here must round on its own, as the host code it reproduces does, wherever this file is included (the
// Makefile also compiles both including files with -ffp-contract=off).
#pragma clang fp contract(off)

namespace sat {

constexpr int RS_BITS = 32 - 8 - 2;          // Pillow's PRECISION_BITS for 8-bit pixels
constexpr int RS_MAX_TAPS = 129;             // BILINEAR shrink factors up to 64, BICUBIC up to 32

__device__ inline int clip8(int v) { v >>= RS_BITS; return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Resample.c bilinear_filter
struct Bilinear {
    static constexpr double SUPPORT = 1.0;
    static __device__ double weight(double x) {
        if (x < 0.0) x = -x;
        return x < 1.0 ? __dsub_rn(1.0, x) : 0.0;
    }
};

// Resample.c bicubic_filter with a = -0.5, in its order of evaluation
struct Bicubic {
    static constexpr double SUPPORT = 2.0;
    static __device__ double weight(double x) {
        if (x < 0.0) x = -x;
        if (x < 1.0) return __dadd_rn(__dmul_rn(__dmul_rn(__dsub_rn(__dmul_rn(1.5, x), 2.5), x), x), 1.0);
        if (x < 2.0) return __dmul_rn(__dsub_rn(__dmul_rn(__dadd_rn(__dmul_rn(__dsub_rn(x, 5.0), x), 8.0), x), 4.0), -0.5);
        return 0.0;
    }
};

// Pillow's ksize: ceil(support) * 2 + 1 with support = SUPPORT * max(1, in / out)
template <class F>
__host__ __device__ inline int resample_taps(int in_size, int out_size) {
    double fs = (double)in_size / (double)out_size;
    if (fs < 1.0) fs = 1.0;
    return (int)ceil(F::SUPPORT * fs) * 2 + 1;
}

// precompute_coeffs + normalize_coeffs_8bpc for output index xx of in_size samples resampled to out_size: the first tap, the tap count
// (at most KT: the caller sizes KT by resample_taps) and the integer weights k[0..KT), zero past the count.  Every double operation is
// a single correctly rounded IEEE operation in the order Pillow's C evaluates it.
template <class F>
__device__ inline void resample_entry(int in_size, int out_size, int xx, int KT, int* __restrict__ first, int* __restrict__ count, int* __restrict__ k) {
    const double scale = __ddiv_rn((double)in_size, (double)out_size);
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = __dmul_rn(F::SUPPORT, filterscale);
    const double ss = __ddiv_rn(1.0, filterscale);
    const double center = __dadd_rn(0.0, __dmul_rn(__dadd_rn((double)xx, 0.5), scale));
    int xmin = (int)__dadd_rn(__dsub_rn(center, support), 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)__dadd_rn(__dadd_rn(center, support), 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    if (xmax > KT) xmax = KT;                          // cannot happen (KT from the same rule); keeps the table in bounds
    if (xmax < 0) xmax = 0;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x)
        ww = __dadd_rn(ww, F::weight(__dmul_rn(__dadd_rn(__dsub_rn((double)(x + xmin), center), 0.5), ss)));
    for (int x = 0; x < xmax; ++x) {
        double wv = F::weight(__dmul_rn(__dadd_rn(__dsub_rn((double)(x + xmin), center), 0.5), ss));
        if (ww != 0.0) wv = __ddiv_rn(wv, ww);
        const double scaled = __dmul_rn(wv, (double)(1 << RS_BITS));
        k[x] = wv < 0.0 ? (int)__dadd_rn(-0.5, scaled) : (int)__dadd_rn(0.5, scaled);      // negative lobes round away from zero too
    }
    for (int x = xmax; x < KT; ++x) k[x] = 0;
    *first = xmin;
    *count = xmax;
}

// what the passes need to know of one picture: the box cut out of it, the size the box is resampled to, the (out_h, out_w) window of
// the resampled picture, the mirror
struct ResampleGeometry { int top, left, box_h, box_w, resized_h, resized_w, out_top, out_left, flip; };

// table row of output index 0 of (picture, axis): axis 0 = columns (horizontal pass), 1 = rows (vertical pass)
template <class G>
__device__ inline long table_row(int img, int axis, int omax) { return ((long)img * G::TABLES + (G::TABLES == 2 ? axis : 0)) * omax; }

// coefficient tables: output index o of the window -> first tap, tap count (bounds), integer weights (coeffs)
template <class F, class G>
__global__ __launch_bounds__(64) void resample_coeffs_kernel(const sat_image_desc* __restrict__ desc, int out_h, int out_w, int omax, int KT,
                                                             int* __restrict__ bounds, int* __restrict__ coeffs) {
    const int img = blockIdx.z, axis = blockIdx.y;
    const int o = blockIdx.x * 64 + threadIdx.x;
    if (o >= (axis ? out_h : out_w)) return;
    const ResampleGeometry g = G::of(desc[img], out_h, out_w);
    const long e = table_row<G>(img, axis, omax) + o;
    resample_entry<F>(axis ? g.box_h : g.box_w, axis ? g.resized_h : g.resized_w, o + (axis ? g.out_top : g.out_left), KT, bounds + e * 2,
                      bounds + e * 2 + 1, coeffs + e * KT);
}

// horizontal pass over every row of the box: tmp[img][row][x] = RGBX bytes
template <class G>
__global__ __launch_bounds__(256) void resample_rows_kernel(const uint8_t* __restrict__ pixels, const sat_image_desc* __restrict__ desc, int out_h, int out_w,
                                                            int omax, int KT, int hmax, const int* __restrict__ bounds, const int* __restrict__ coeffs,
                                                            uchar4* __restrict__ tmp) {
    const int img = blockIdx.z;
    const sat_image_desc d = desc[img];
    const ResampleGeometry g = G::of(d, out_h, out_w);
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int row = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= out_w || row >= g.box_h) return;
    const long e = table_row<G>(img, 0, omax) + x;
    const int* k = coeffs + e * KT;
    const int xmin = bounds[e * 2], n = bounds[e * 2 + 1];
    const uint8_t* src = pixels + d.offset + ((long)(g.top + row) * d.width + g.left + xmin) * 3;
    int s0 = 1 << (RS_BITS - 1), s1 = s0, s2 = s0;
    for (int t = 0; t < n; ++t) {
        const int kv = k[t];
        s0 += src[t * 3 + 0] * kv; s1 += src[t * 3 + 1] * kv; s2 += src[t * 3 + 2] * kv;
    }
    tmp[((long)img * hmax + row) * out_w + x] = make_uchar4((unsigned char)clip8(s0), (unsigned char)clip8(s1), (unsigned char)clip8(s2), 0);
}

// vertical pass of output pixel (x, y) of picture img: its RGB bytes
template <class G>
__device__ inline void resample_col(int img, int x, int y, int omax, int KT, int hmax, int out_w, const int* __restrict__ bounds,
                                    const int* __restrict__ coeffs, const uchar4* __restrict__ tmp, int v[3]) {
    const long e = table_row<G>(img, 1, omax) + y;
    const int* k = coeffs + e * KT;
    const int ymin = bounds[e * 2], n = bounds[e * 2 + 1];
    const uchar4* src = tmp + ((long)img * hmax + ymin) * out_w + x;
    int s0 = 1 << (RS_BITS - 1), s1 = s0, s2 = s0;
    for (int t = 0; t < n; ++t) {
        const int kv = k[t];
        const uchar4 p = src[(long)t * out_w];
        s0 += p.x * kv; s1 += p.y * kv; s2 += p.z * kv;
    }
    v[0] = clip8(s0); v[1] = clip8(s1); v[2] = clip8(s2);
}

// T.ToTensor() (byte / 255, one correctly rounded fp32 division) + noise (or NULL) of the bytes of output pixel (xo, y) (after the
// flip): three fp32 planes and / or the HWC bytes
__device__ inline void finish_pixel(const int v[3], int img, int y, int xo, int out_h, int out_w, const float* __restrict__ noise, float noise_std,
                                    float* __restrict__ out, uint8_t* __restrict__ out_u8) {
    const long plane = (long)out_h * out_w;
    const long o = (long)img * 3 * plane + (long)y * out_w + xo;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (out) {
            float f = __fdiv_rn((float)v[c], 255.0f);
            if (noise) f = __fadd_rn(f, __fmul_rn(noise[o + c * plane], noise_std));
            out[o + c * plane] = f;
        }
        if (out_u8) out_u8[(((long)img * out_h + y) * out_w + xo) * 3 + c] = (uint8_t)v[c];
    }
}

// vertical pass + flip + ToTensor + noise; one thread per output pixel, the three colour planes written coalesced along x
template <class G>
__global__ __launch_bounds__(256) void resample_cols_finish_kernel(const sat_image_desc* __restrict__ desc, int out_h, int out_w, int omax, int KT, int hmax,
                                                                   const int* __restrict__ bounds, const int* __restrict__ coeffs,
                                                                   const uchar4* __restrict__ tmp, const float* __restrict__ noise, float noise_std,
                                                                   float* __restrict__ out, uint8_t* __restrict__ out_u8) {
    const int img = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= out_w || y >= out_h) return;
    int v[3];
    resample_col<G>(img, x, y, omax, KT, hmax, out_w, bounds, coeffs, tmp, v);
    finish_pixel(v, img, y, G::of(desc[img], out_h, out_w).flip ? out_w - 1 - x : x, out_h, out_w, noise, noise_std, out, out_u8);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side, shared by image_plan and square_plan

inline int picture_in_buffer(const char* who, int i, const sat_image_desc& e, int64_t pixels_bytes) {
    SAT_REQUIRE(e.height > 0 && e.width > 0 && e.offset >= 0 && (pixels_bytes < 0 || e.offset + (int64_t)e.height * e.width * 3 <= pixels_bytes),
                "%s: picture %d (%dx%d at byte %lld) lies outside the pixel buffer", who, i, e.height, e.width, (long long)e.offset);
    return SAT_OK;
}

// carves 256-byte aligned pieces off a workspace
struct Workspace {
    size_t total = 0;
    size_t take(size_t bytes) { size_t at = total; total += (bytes + 255) & ~(size_t)255; return at; }
};

// KT: taps per table row; hmax: rows of the tallest box; omax: outputs per table; total: bytes of the whole workspace
struct ResamplePlan { int KT, hmax, omax; size_t bounds_off, coeffs_off, tmp_off, total; };

template <class G>
inline void carve_resample(Workspace& ws, ResamplePlan* p, int n, int out_w) {
    p->bounds_off = ws.take((size_t)n * G::TABLES * p->omax * 2 * sizeof(int));
    p->coeffs_off = ws.take((size_t)n * G::TABLES * p->omax * p->KT * sizeof(int));
    p->tmp_off = ws.take((size_t)n * p->hmax * out_w * sizeof(uchar4));
}

// the two launches every entry point starts with: tables, then the horizontal pass into tmp
template <class F, class G>
inline int launch_resample_rows(hipStream_t st, const uint8_t* pixels, const sat_image_desc* desc_dev, int n, int out_h, int out_w, const ResamplePlan& p,
                                char* ws) {
    int* bounds = (int*)(ws + p.bounds_off);
    int* coeffs = (int*)(ws + p.coeffs_off);
    hipLaunchKernelGGL((resample_coeffs_kernel<F, G>), dim3((p.omax + 63) / 64, G::TABLES, n), dim3(64), 0, st, desc_dev, out_h, out_w, p.omax, p.KT, bounds,
                       coeffs);
    SAT_TRY(launch_ok("resample_coeffs"));
    hipLaunchKernelGGL((resample_rows_kernel<G>), dim3((out_w + 63) / 64, (p.hmax + 3) / 4, n), dim3(256), 0, st, pixels, desc_dev, out_h, out_w, p.omax, p.KT,
                       p.hmax, bounds, coeffs, (uchar4*)(ws + p.tmp_off));
    return launch_ok("resample_rows");
}

}  // namespace sat
