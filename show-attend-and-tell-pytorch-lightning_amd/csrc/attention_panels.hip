// visualize.ipynb's make_visual on device: the single-image inference front end (util.py:141-164 load_square / prepare_image) and
// the attention overlays of a decoded caption.
//   sat_image_square_bicubic   crop_center(min side) + Image.resize((S, S)) - no filter given, which is Pillow's BICUBIC - of a ragged
//                              batch of HWC uint8 pictures, bit exact, with T.ToTensor()'s fp32 planes on request
//   sat_attention_panels       per caption step: the (h, w) attention map normalised to [0, 1], raised to a power, cut to bytes,
//                              enlarged to (V, V) by the same BICUBIC resample and blended over the picture; plus "Total Attention"
// The resample is pillow_resample.h, shared with image_pipeline.hip's BILINEAR path: the same coefficient, rows and column-finish
// kernels, here with the BICUBIC filter (support 2.0 * filterscale, the cubic weights with a = -0.5, negative coefficients rounded away
// from zero) and the centred square as geometry.  The panels kernel builds its 5-tap tables with the same resample_entry.
#include "pillow_resample.h"

// every floating-point operation rounds on its own, as the host code it reproduces does (Makefile: -ffp-contract=off)
#pragma clang fp contract(off)

namespace sat {

constexpr int BC_MAX_SHRINK = SAT_BICUBIC_MAX_SHRINK;   // ceil(2 * 32) * 2 + 1 = 129 = RS_MAX_TAPS
constexpr int BC_UP_TAPS = 5;                // enlarging: ceil(2.0) * 2 + 1

// util.py:152-157 crop_center(img, s, s) with s = min(width, height): ((W - s) // 2, (H - s) // 2, (W + s) // 2, (H + s) // 2); the
// box is s wide and high whatever the parities, because W - s and W + s are both even or both odd
__host__ __device__ inline void square_box(int height, int width, int* top, int* left, int* side) {
    const int s = height < width ? height : width;
    *side = s;
    *left = (width - s) / 2;
    *top = (height - s) / 2;
}

// sat_image_square_bicubic reads ONLY height and width (and offset) of a descriptor: the box is the centred square, resampled to the
// output size, no window, no mirror.  The box is square and so is the output: one coefficient table per picture serves both passes.
struct SquareGeometry {
    static constexpr int TABLES = 1;
    static __device__ ResampleGeometry of(const sat_image_desc& d, int out_h, int out_w) {
        int top, left, side;
        square_box(d.height, d.width, &top, &left, &side);
        return {top, left, side, side, out_h, out_w, 0, 0, 0};
    }
};

static int square_plan(const sat_image_desc* d, int n, int64_t pixels_bytes, int S, ResamplePlan* p) {
    SAT_REQUIRE(n > 0 && n <= 65535, "square_bicubic: n=%d outside [1, 65535]", n);
    SAT_REQUIRE(S > 0 && S <= 16384, "square_bicubic: output size %d outside [1, 16384]", S);
    int KT = BC_UP_TAPS, hmax = 1;
    for (int i = 0; i < n; ++i) {
        const sat_image_desc& e = d[i];
        SAT_TRY(picture_in_buffer("square_bicubic", i, e, pixels_bytes));
        int top, left, side;
        square_box(e.height, e.width, &top, &left, &side);
        SAT_REQUIRE((int64_t)side <= (int64_t)BC_MAX_SHRINK * S, "square_bicubic: picture %d (side %d -> %d) shrinks by more than %dx", i, side, S,
                    BC_MAX_SHRINK);
        const int k = resample_taps<Bicubic>(side, S);
        SAT_REQUIRE(k <= RS_MAX_TAPS, "square_bicubic: picture %d needs %d taps (at most %d)", i, k, RS_MAX_TAPS);
        if (k > KT) KT = k;
        if (side > hmax) hmax = side;
    }
    SAT_REQUIRE((hmax + 3) / 4 <= 65535, "square_bicubic: a side of %d pixels is too large", hmax);
    p->KT = KT; p->hmax = hmax; p->omax = S;
    Workspace ws;
    carve_resample<SquareGeometry>(ws, p, n, S);
    p->total = ws.total;
    return SAT_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Attention panels.  One block = one 64 x 16 tile of one panel.  The block rebuilds what the tile needs in LDS - the (h, w) map of
// its step (or the sum of the steps), its minimum and maximum, the byte mask, and the 5-tap tables of its 64 columns and 16 rows -
// and every thread then resamples and blends four pixels.  The masks never go through global memory.
constexpr int AP_MAX_MAP = SAT_ATTENTION_MAX_MAP;
constexpr int AP_TW = 64, AP_TH = 16;

// Image.blend(picture, mask, opacity) per byte: p + opacity * (m - p) in fp32, truncated (Pillow's (UINT8) cast)
__device__ inline int blend_over(int p, int m, float opacity) {
    const float t = __fadd_rn((float)p, __fmul_rn(opacity, (float)(m - p)));
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

__global__ __launch_bounds__(256) void attention_panels_kernel(const uint8_t* __restrict__ square, const float* __restrict__ cap_alpha,
                                                               const int* __restrict__ cap_len, int Tmax, int h, int w, int V, int tiles_x,
                                                               float power, float opacity, uint8_t* __restrict__ panels) {
    __shared__ float att[AP_MAX_MAP];
    __shared__ uint8_t mask[AP_MAX_MAP];
    __shared__ float red_min[4], red_max[4];
    __shared__ int tab_first[AP_TW + AP_TH], tab_count[AP_TW + AP_TH], tab_k[AP_TW + AP_TH][BC_UP_TAPS];
    const int b = blockIdx.z, p = blockIdx.y, tid = threadIdx.x;
    const int x = (blockIdx.x % tiles_x) * AP_TW + (tid & 63);
    const int y0 = (blockIdx.x / tiles_x) * AP_TH + (tid >> 6);
    int n = cap_len[b];
    n = n < 0 ? 0 : (n > Tmax ? Tmax : n);             // read from device memory: clamped before it addresses anything
    const uint8_t* pic = square + (long)b * V * V * 3;
    uint8_t* dst = panels + ((long)b * (Tmax + 2) + p) * V * V * 3;
    if (p == 0 || p > n + 1) {                         // the picture itself / nothing (the whole block takes the same branch)
        for (int i = 0; i < AP_TH / 4; ++i) {
            const int y = y0 + 4 * i;
            if (x >= V || y >= V) continue;
            const long o = ((long)y * V + x) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[o + c] = p == 0 ? pic[o + c] : (uint8_t)0;
        }
        return;
    }
    const bool total = p == n + 1;
    const int L = h * w;
    const float* a = cap_alpha + (long)b * Tmax * L;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = tid; i < L; i += 256) {
        float s;
        if (total) {                                   // alpha[b, :n].sum(0): fp32, added in step order
            s = n > 0 ? a[i] : 0.0f;
            for (int t = 1; t < n; ++t) s = __fadd_rn(s, a[(long)t * L + i]);
        } else {
            s = a[(long)(p - 1) * L + i];
        }
        att[i] = s;
        mn = fminf(mn, s); mx = fmaxf(mx, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o, 64)); mx = fmaxf(mx, __shfl_xor(mx, o, 64)); }
    if ((tid & 63) == 0) { red_min[tid >> 6] = mn; red_max[tid >> 6] = mx; }
    if (tid < AP_TW + AP_TH) {                         // the tables of this tile's columns (w -> V) and rows (h -> V)
        const bool col = tid < AP_TW;
        const int o = col ? (blockIdx.x % tiles_x) * AP_TW + tid : (blockIdx.x / tiles_x) * AP_TH + (tid - AP_TW);
        if (o < V) resample_entry<Bicubic>(col ? w : h, V, o, BC_UP_TAPS, &tab_first[tid], &tab_count[tid], tab_k[tid]);
    }
    __syncthreads();
    mn = fminf(fminf(red_min[0], red_min[1]), fminf(red_min[2], red_min[3]));
    mx = fmaxf(fmaxf(red_max[0], red_max[1]), fmaxf(red_max[2], red_max[3]));
    const float range = __fsub_rn(mx, mn);
    for (int i = tid; i < L; i += 256) {
        int m = 0;                                     // a flat map (0 / 0 in the notebook) is defined as a zero mask
        if (mx > mn) {
            float v = __fdiv_rn(__fsub_rn(att[i], mn), range);
            // x ** power as the host's powf gives it: evaluated in double and rounded once to fp32
            if (!total && power != 1.0f) v = (float)pow((double)v, (double)power);
            m = (int)__fmul_rn(v, 255.0f);             // np.uint8(): truncation
            m = m < 0 ? 0 : (m > 255 ? 255 : m);
        }
        mask[i] = (uint8_t)m;
    }
    __syncthreads();
    if (x >= V) return;
    const int cx = tid & 63, xmin = tab_first[cx], nx = tab_count[cx];
    for (int i = 0; i < AP_TH / 4; ++i) {
        const int y = y0 + 4 * i;
        if (y >= V) continue;
        const int ry = AP_TW + (tid >> 6) + 4 * i, ymin = tab_first[ry], ny = tab_count[ry];
        int v = 1 << (RS_BITS - 1);
        for (int t = 0; t < ny; ++t) {                 // the horizontal pass of row ymin + t at column x, then its vertical weight
            const uint8_t* row = mask + (ymin + t) * w + xmin;
            int s = 1 << (RS_BITS - 1);
            for (int u = 0; u < nx; ++u) s += row[u] * tab_k[cx][u];
            v += clip8(s) * tab_k[ry][t];
        }
        const int m = clip8(v);
        const long o = ((long)y * V + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[o + c] = (uint8_t)(total ? m : blend_over(pic[o + c], m, opacity));
    }
}

}  // namespace sat
using namespace sat;

extern "C" {

size_t sat_image_square_bicubic_workspace_bytes(const sat_image_desc* desc_host, int32_t n, int32_t S) {
    if (!desc_host) { fail(SAT_EINVAL, "square_bicubic: null descriptors"); return 0; }
    ResamplePlan p;
    if (square_plan(desc_host, n, -1, S, &p) != SAT_OK) return 0;
    return p.total;
}

int sat_image_square_bicubic(const uint8_t* pixels, int64_t pixels_bytes, const sat_image_desc* desc_host, const sat_image_desc* desc_dev, int32_t n,
                             int32_t S, uint8_t* out_u8, float* out_nchw, void* workspace, size_t workspace_bytes, void* stream) {
    if (!pixels || !desc_host || !desc_dev || !workspace || (!out_u8 && !out_nchw)) return fail(SAT_EINVAL, "square_bicubic: null pointer");
    ResamplePlan p;
    SAT_TRY(square_plan(desc_host, n, pixels_bytes, S, &p));
    SAT_REQUIRE(workspace_bytes >= p.total, "square_bicubic: workspace %zu < %zu bytes", workspace_bytes, p.total);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    SAT_TRY((launch_resample_rows<Bicubic, SquareGeometry>(st, pixels, desc_dev, n, S, S, p, ws)));
    hipLaunchKernelGGL(resample_cols_finish_kernel<SquareGeometry>, dim3((S + 63) / 64, (S + 3) / 4, n), dim3(256), 0, st, desc_dev, S, S, p.omax, p.KT, p.hmax,
                       (const int*)(ws + p.bounds_off), (const int*)(ws + p.coeffs_off), (const uchar4*)(ws + p.tmp_off), (const float*)nullptr, 0.0f,
                       out_nchw, out_u8);
    return launch_ok("resample_cols_finish");
}

int sat_attention_panels(const uint8_t* square, const float* cap_alpha, const int32_t* cap_len, int32_t B, int32_t Tmax, int32_t V, int32_t h, int32_t w,
                         float power, float opacity, uint8_t* panels, void* stream) {
    if (!square || !cap_alpha || !cap_len || !panels) return fail(SAT_EINVAL, "attention_panels: null pointer");
    SAT_REQUIRE(B > 0 && B <= 65535 && Tmax > 0 && Tmax + 2 <= 65535, "attention_panels: B=%d Tmax=%d outside [1, 65535] / [1, 65533]", B, Tmax);
    SAT_REQUIRE(V > 0 && V <= 16384, "attention_panels: visual size %d outside [1, 16384]", V);
    SAT_REQUIRE(h > 0 && w > 0 && (int64_t)h * w <= AP_MAX_MAP, "attention_panels: map %dx%d outside [1, %d] elements", h, w, AP_MAX_MAP);
    SAT_REQUIRE(h <= V && w <= V, "attention_panels: the %dx%d map is larger than the %d-pixel panel (the mask is enlarged, never shrunk)", h, w, V);
    SAT_REQUIRE(opacity >= 0.0f && opacity <= 1.0f, "attention_panels: opacity %g outside [0, 1]", (double)opacity);
    SAT_REQUIRE(std::isfinite(power) && power > 0.0f, "attention_panels: power %g must be finite and > 0", (double)power);
    const int tiles_x = (V + AP_TW - 1) / AP_TW, tiles_y = (V + AP_TH - 1) / AP_TH;
    hipLaunchKernelGGL(attention_panels_kernel, dim3(tiles_x * tiles_y, Tmax + 2, B), dim3(256), 0, (hipStream_t)stream, square, cap_alpha, cap_len, Tmax, h,
                       w, V, tiles_x, power, opacity, panels);
    return launch_ok("attention_panels");
}

}
