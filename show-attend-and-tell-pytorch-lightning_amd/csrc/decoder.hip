// Host-side orchestration of the SAT decoder on one HIP stream: the whole train_batch time loop
// (model.py:487-548) and its backward through time, as a fixed sequence of kernel launches.
// No allocation, no synchronisation: everything lives in the caller's workspace.
#include "../../include/sat_hip.h"
#include <stdlib.h>
#include <map>
#include <mutex>
#include <utility>
#include "decoder_step.h"
#include "profile.h"
#include "decoder_kernels.h"

namespace sat {

// ------------------------------------------------------------------ workspace layout
struct Ws {
    size_t total = 0;
    // saved by forward
    float *U, *mean, *f, *init_img, *H_all, *C_all, *HC, *Z, *XZ, *Y, *GY, *Uact, *Wcat, *bcat;
    float *Udrop, *mean_rows, *f_rows, *init_rows, *df_rows;     // only carved when dropout > 0
    float *GU, *DGU, *bup;                                       // stacked LSTM layers (layers > 1): gates, gate grads, bias sums
    __bf16 *Wb_out, *Ub;                                         // bf16 mode: bf16 copies of output.output.weight and of the packed deep-output rows
    __bf16 *annb;                                                // bf16 mode: annotations as the attention context / dalpha kernels stream them
    __bf16 *Hb, *XZb, *Wcat_b, *Wz_b, *DHCb;                            // bf16 mode, one LSTM layer: operands of the per-step GEMMs (state, gated context, weights)
    int* Tok; int* flags;
    int *emb_count, *emb_offset, *emb_cursor, *emb_list;         // embedding gradient: per-row token segments
    float *SC, *DA;                                              // attention: raw scores / score gradients of one step (N, L)
    // backward scratch
    float *dA, *dHout, *dZout, *DZ, *DHC, *dXZ, *dHc, *dCc, *dU, *dwf_part, *dY, *colpart, *dinit_img, *df, *dmean, *slab;
    float *dmean_rows;                                           // dropout > 0: d(mean rows) of the InitLSTM backward
    float *colpart2, *slab2;                                     // scratch of decoder_bwd's leaf part when it runs on a side stream
    float *Wup;                                                  // weight_drop > 0, layers > 1: masked W_hh of the stacked layers, [layers - 1][4n][n]
    // layer-normalised cell only, carved last (every other pointer is where the plain cell has it): what the forward saves for the backward,
    // [layers][T1][N][5n] normalised values and [layers][T1][N][5] reciprocal standard deviations; the parameter-gradient partials [layers][slots][10n]
    float *ln_xhat, *ln_rstd, *ln_part;
    int ln_nslots;
    char *zero_begin, *zero_end;                                 // [dHout .. dwf_part]: what decoder_bwd zeroes in one memset
    long slab_elems;
};

Ws layout(const sat_decoder_dims& d, char* base, bool ln = false) {
    Ws w; size_t off = 0;
    const long N = (long)d.B * d.R, T1 = d.T - 1, HCW = d.A + d.D + 4L * d.n;
    auto take = [&](size_t elems, size_t esz = 4) { size_t o = off; off += (elems * esz + 255) & ~(size_t)255; return base ? base + o : (char*)nullptr; };
    w.U = (float*)take((size_t)d.B * d.L * d.A);
    w.mean = (float*)take((size_t)d.B * d.D);
    w.f = (float*)take((size_t)d.B * d.m);
    const int NL = d.layers;
    w.init_img = (float*)take((size_t)d.B * 2 * d.n * NL);
    // hidden / cell state of every layer and step, one time-major run per layer: [layer][T1 + 1][N][n]
    w.H_all = (float*)take((size_t)NL * (T1 + 1) * N * d.n);
    w.C_all = (float*)take((size_t)NL * (T1 + 1) * N * d.n);
    w.GU = w.DGU = w.bup = nullptr;
    if (NL > 1) {
        w.GU = (float*)take((size_t)(NL - 1) * T1 * N * 4 * d.n); w.DGU = (float*)take((size_t)(NL - 1) * T1 * N * 4 * d.n);
        w.bup = (float*)take((size_t)(NL - 1) * 4 * d.n);
    }
    w.HC = (float*)take((size_t)T1 * N * HCW);
    w.Z = (float*)take((size_t)T1 * N * d.D);
    w.XZ = (float*)take((size_t)T1 * N * d.D);
    w.Y = (float*)take((size_t)T1 * N * d.m);
    w.GY = (float*)take((size_t)T1 * N * 4 * d.n);
    w.Uact = (float*)take((size_t)(d.P > 0 ? d.P : 1) * d.m);
    w.Wcat = (float*)take((size_t)HCW * d.n);
    w.bcat = (float*)take((size_t)HCW);
    w.Tok = (int*)take((size_t)T1 * N);
    w.Udrop = w.mean_rows = w.f_rows = w.init_rows = w.df_rows = w.dmean_rows = nullptr;
    if (d.dropout > 0.f) {
        w.Udrop = (float*)take((size_t)(d.P > 0 ? d.P : 1) * d.m); w.mean_rows = (float*)take((size_t)N * d.D); w.f_rows = (float*)take((size_t)N * d.m);
        w.init_rows = (float*)take((size_t)N * 2 * d.n * NL); w.df_rows = (float*)take((size_t)N * d.m);
        w.dmean_rows = (float*)take((size_t)N * d.D);
    }
    w.Wb_out = w.Ub = nullptr;
    if (d.precision && d.m % 64 == 0 && d.V % 8 == 0) {           // operands of the vocabulary projection for the direct-to-LDS GEMM
        w.Wb_out = (__bf16*)take((size_t)d.V * d.m, 2); w.Ub = (__bf16*)take((size_t)(d.P > 0 ? d.P : 1) * d.m, 2);
    }
    w.Hb = w.XZb = w.Wcat_b = w.Wz_b = w.DHCb = nullptr;
    // bf16 mode: a bf16 copy of the annotations for the two kernels that stream them every time step (attention context / dalpha)
    w.annb = (d.precision && d.D % 4 == 0 && d.A % 4 == 0) ? (__bf16*)take((size_t)d.B * d.L * d.D, 2) : nullptr;
    if (d.precision && d.layers == 1 && d.n % 64 == 0 && d.D % 64 == 0 && d.A % 4 == 0 && d.m % 4 == 0) {
        w.Hb = (__bf16*)take((size_t)(T1 + 1) * N * d.n, 2); w.XZb = (__bf16*)take((size_t)N * d.D, 2);
        w.Wcat_b = (__bf16*)take((size_t)HCW * d.n, 2); w.Wz_b = (__bf16*)take((size_t)4 * d.n * d.D, 2);
        w.DHCb = (__bf16*)take((size_t)N * HCW, 2);
    }
    w.flags = (int*)take((size_t)d.V);
    w.emb_count = (int*)take((size_t)d.V); w.emb_offset = (int*)take((size_t)d.V + 1); w.emb_cursor = (int*)take((size_t)d.V);
    w.emb_list = (int*)take((size_t)T1 * N);
    w.SC = (float*)take((size_t)N * d.L); w.DA = (float*)take((size_t)N * d.L);
    w.dA = (float*)take((size_t)(d.P > 0 ? d.P : 1) * d.m);
    w.DZ = (float*)take((size_t)T1 * N * d.D);
    w.DHC = (float*)take((size_t)T1 * N * HCW);
    w.dXZ = (float*)take((size_t)N * d.D);
    // the accumulators the backward pass starts from zero, adjacent: one memset (zero_begin .. zero_end)
    w.dHout = (float*)take((size_t)T1 * N * d.n); w.zero_begin = (char*)w.dHout;
    w.dZout = (float*)take((size_t)T1 * N * d.D);
    w.dHc = (float*)take((size_t)NL * N * d.n);
    w.dCc = (float*)take((size_t)NL * N * d.n);
    w.dU = (float*)take((size_t)d.B * d.L * d.A);
    w.dwf_part = (float*)take((size_t)d.B * d.A);
    w.zero_end = base ? base + off : (char*)nullptr;
    w.dY = (float*)take((size_t)T1 * N * d.m);
    long maxrows = d.P > T1 * N ? d.P : T1 * N; if (maxrows < d.B * (long)d.L) maxrows = d.B * (long)d.L;
    long maxcols = d.V > HCW ? d.V : HCW;
    w.colpart = (float*)take((size_t)cdiv(maxrows, 256) * maxcols);
    w.dinit_img = (float*)take((size_t)d.B * 2 * d.n * NL);
    w.df = (float*)take((size_t)d.B * d.m);
    w.dmean = (float*)take((size_t)d.B * d.D);
    w.slab_elems = 8L << 20;   // 32 MiB of split-K partials
    w.slab = (float*)take((size_t)w.slab_elems);
    // a second column-sum and split-K scratch: the leaf part of decoder_bwd on its side stream runs while the main stream uses the first
    w.colpart2 = (float*)take((size_t)cdiv(maxrows, 256) * maxcols);
    w.slab2 = (float*)take((size_t)w.slab_elems);
    w.Wup = (d.weight_drop > 0.f && NL > 1) ? (float*)take((size_t)(NL - 1) * 4 * d.n * d.n) : nullptr;
    w.ln_xhat = w.ln_rstd = w.ln_part = nullptr; w.ln_nslots = 0;
    if (ln) {
        w.ln_nslots = ln_slots((int)N);
        w.ln_xhat = (float*)take((size_t)NL * T1 * N * 5 * d.n); w.ln_rstd = (float*)take((size_t)NL * T1 * N * 5);
        w.ln_part = (float*)take((size_t)NL * w.ln_nslots * 10 * d.n);
    }
    w.total = off;
    return w;
}

int check_dims(const sat_decoder_dims* d) {
    SAT_REQUIRE(d, "decoder: null dims");
    SAT_REQUIRE(d->B > 0 && d->R > 0 && d->T >= 2 && d->L > 0 && d->D > 0 && d->A > 0 && d->m > 0 && d->n > 0 && d->V > 0,
                "decoder: non-positive dimension (B=%d R=%d T=%d L=%d D=%d A=%d m=%d n=%d V=%d)", d->B, d->R, d->T, d->L, d->D, d->A, d->m, d->n, d->V);
    SAT_REQUIRE(d->P >= 0 && (long)d->P <= (long)d->B * d->R * (d->T - 1), "decoder: packed token count %d out of range", d->P);
    SAT_REQUIRE(d->layers >= 1 && d->layers <= SAT_MAX_LSTM_LAYERS, "decoder: layers=%d outside 1..%d", d->layers, SAT_MAX_LSTM_LAYERS);
    SAT_REQUIRE(d->dropout >= 0.f && d->dropout < 1.f && d->embedding_dropout >= 0.f && d->embedding_dropout < 1.f, "decoder: dropout must lie in [0,1)");
    SAT_REQUIRE(d->weight_drop >= 0.f && d->weight_drop < 1.f, "decoder: weight_drop=%g must lie in [0,1)", (double)d->weight_drop);
    return SAT_OK;
}

// ------------------------------------------------------------------ small launch helpers
thread_local int t_bf16_mfma = 0;             // decoder_step.h; set per call from sat_decoder_dims.precision

// fp32 -> bf16 copy of n elements (n % 4 == 0)
static int cast_bf16(hipStream_t st, const float* src, __bf16* dst, long n) {
    hipLaunchKernelGGL(cast_bf16_kernel, dim3(cdiv(n / 4, 256)), dim3(256), 0, st, src, dst, n / 4);
    return launch_ok("cast_bf16");
}
// C (fp32) = A (bf16, rows x K) * B^T (bf16, N x K): both operands bf16 in HBM -> gemm_glds.hip
static int gemm_bb_nt(hipStream_t st, const __bf16* A, long lda, const __bf16* B, long ldb, float* C, long ldc, int M, int N, int K, int epi, const float* bias,
                      int acc = 0, int c0 = 0, int c1 = 0) {
    GemmArgs g;
    g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.amode = A_ROW; g.bmode = B_ROW; g.epi = epi; g.bias = bias; g.a_bf16 = g.b_bf16 = 1; g.c_bf16 = 0; g.bf16_mfma = 1;
    g.accumulate = acc; g.c0 = c0; g.c1 = c1;
    return launch_gemm(g, st);
}

// C (fp32) (+)= A (bf16, rows x K, row stride lda) * B (bf16, K x N k-major): data gradients of the per-step products
static int gemm_bb_nn(hipStream_t st, const __bf16* A, long lda, const __bf16* B, long ldb, float* C, long ldc, int M, int N, int K, int acc, float* slab, long slab_elems) {
    GemmArgs g;
    g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.amode = A_ROW; g.bmode = B_KMAJOR; g.a_bf16 = g.b_bf16 = 1; g.c_bf16 = 0; g.bf16_mfma = 1; g.accumulate = acc; g.slab = slab; g.slab_elems = slab_elems;
    return launch_gemm(g, st);
}

static int colsum(hipStream_t st, const Ws& w, const float* x, long ld, int rows, int cols, float* out, int accumulate = 0, float scale = 1.f) {
    if (cols <= 0) return SAT_OK;
    if (rows <= 0) { if (!accumulate) SAT_TRY(dev_fill_bytes(st, out, 0, (size_t)cols * 4)); return SAT_OK; }
    int nparts = cdiv(rows, 256);
    if (cols % 4 == 0 && ld % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0)
        hipLaunchKernelGGL(colsum_part4_kernel, dim3(cdiv(cols / 4, 128), nparts), dim3(128), 0, st, x, ld, rows, cols / 4, 256, w.colpart);
    else
        hipLaunchKernelGGL(colsum_part_kernel, dim3(cdiv(cols, 256), nparts), dim3(256), 0, st, x, ld, rows, cols, 256, w.colpart);
    SAT_TRY(launch_ok("colsum_part"));
    hipLaunchKernelGGL(colsum_finish_kernel, dim3(cdiv(cols, 256)), dim3(256), 0, st, w.colpart, nparts, cols, out, accumulate, scale);
    return launch_ok("colsum_finish");
}

// weight-drop: `layers` matrices of `per` elements, dst[l] = src[l] * mask layer (layer0 + l); one launch
int weight_drop(const float* const* src, float* const* dst, __bf16* const* dstb, int layers, long per, int layer0, float p, unsigned long long seed, hipStream_t st) {
    SAT_REQUIRE(layers >= 1 && layers <= SAT_MAX_LSTM_LAYERS && layer0 >= 0 && per > 0, "weight_drop: layers=%d (1..%d) layer0=%d per=%ld", layers, SAT_MAX_LSTM_LAYERS, layer0, per);
    WeightDropLayers w = {};
    for (int l = 0; l < layers; ++l) { w.src[l] = src[l]; w.dst[l] = dst[l]; w.dstb[l] = dstb ? dstb[l] : nullptr; }
    hipLaunchKernelGGL(weight_drop_kernel, dim3(cdiv(layers * per, 256)), dim3(256), 0, st, w, layers, per, layer0, p, seed);
    return launch_ok("weight_drop");
}

// ------------------------------------------------------------------ what the caption searches share with the train loop (decoder_step.h)
int pack_step_weights(const sat_decoder_dims& d, const sat_decoder_params& p, float* Wcat, __bf16* Wcat_b, float* bcat, float* bup, hipStream_t st,
                      float weight_drop_p, unsigned long long seed) {
    const int n = d.n, HCW = d.A + d.D + 4 * n;
    hipLaunchKernelGGL(pack_wcat_kernel, dim3(cdiv((long)HCW * n + HCW, 256)), dim3(256), 0, st, p.att_dec, p.beta_w, p.w_hh, p.beta_b, p.b_ih, p.b_hh, Wcat, Wcat_b,
                       bcat, d.A, d.D, n, weight_drop_p, seed);
    SAT_TRY(launch_ok("pack Wcat"));
    for (int l = 1; l < d.layers; ++l) {
        hipLaunchKernelGGL(add_kernel, dim3(cdiv(4 * n, 256)), dim3(256), 0, st, bup + (long)(l - 1) * 4 * n, p.up_b_ih[l - 1], p.up_b_hh[l - 1], (long)4 * n);
        SAT_TRY(launch_ok("bias add (stacked layer)"));
    }
    return SAT_OK;
}
int pack_weights_public(const sat_decoder_dims& d, const sat_decoder_params& p, float* wcat, void* wcat_b, float* bcat, hipStream_t st) {
    sat_decoder_dims d0 = d; d0.layers = 1;          // the stacked layers' bias sums are not part of the packing launch
    return pack_step_weights(d0, p, wcat, (__bf16*)wcat_b, bcat, nullptr, st, d.weight_drop, (unsigned long long)d.dropout_seed);
}
int image_begin(const sat_decoder_dims& d, const sat_decoder_params& p, const float* ann, int images, float* U, float* mean, float* f, float* init_img,
                hipStream_t st) {
    const int n2 = 2 * d.n * d.layers;
    // att_enc, hoisted (model.py:100): U = ann * W_e^T once per image
    SAT_TRY(gemm(st, A_ROW, B_ROW, ann, d.D, p.att_enc, d.D, U, d.A, images * d.L, d.A, d.D));
    hipLaunchKernelGGL(ann_mean_kernel, dim3(images), dim3(256), 0, st, ann, mean, d.L, d.D);
    SAT_TRY(launch_ok("ann_mean"));
    if (!f) return SAT_OK;
    // InitLSTM (model.py:76-81) on the images; the caller expands the rows (the raw reshape, F3)
    SAT_TRY(gemm(st, A_ROW, B_ROW, mean, d.D, p.init_f_w, d.D, f, d.m, images, d.m, d.D, 0, EPI_BIAS, p.init_f_b));
    return gemm(st, A_ROW, B_ROW, f, d.m, p.init_i_w, d.m, init_img, n2, images, n2, d.m, 0, EPI_BIAS, p.init_i_b);
}
int lstm_cell_pointwise(float* gates, int g_ld, const float* c_prev, const float* h_prev, float* c_new, float* h_new, const int* live, int rows, int n,
                        hipStream_t st, const LnCell* ln) {
    if (ln) return lstm_ln_cell_fwd(gates, g_ld, nullptr, c_prev, h_prev, c_new, h_new, live, 0, rows, n, nullptr, *ln, nullptr, nullptr, st);
    hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3(cdiv((long)rows * n, 256)), dim3(256), 0, st, gates, g_ld, (const float*)nullptr, c_prev, h_prev, c_new, h_new, live,
                       0, rows, n, (__bf16*)nullptr);
    return launch_ok("lstm_cell_fwd");
}

// the plain pair on caller-supplied gates (sat_lstm_cell_pointwise_fwd / _bwd): the launches of the time loops, for tools that time them
int lstm_cell_plain_fwd(float* gates, int g_ld, const float* gy, const float* c_prev, const float* h_prev, float* c_new, float* h_new, const int* lengths, int step,
                        int rows, int n, void* hb_new, hipStream_t st) {
    hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3(cdiv((long)rows * n, 256)), dim3(256), 0, st, gates, g_ld, gy, c_prev, h_prev, c_new, h_new, lengths, step, rows, n,
                       reinterpret_cast<__bf16*>(hb_new));
    return launch_ok("lstm_cell_fwd");
}
int lstm_cell_plain_bwd(const float* gates, int g_ld, const float* c_prev, const float* c_new, const float* dh_out, float* dh_carry, float* dc_carry, float* dgates,
                        int dg_ld, const int* lengths, int step, int rows, int n, void* dgb, hipStream_t st) {
    hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3(cdiv((long)rows * n, 256)), dim3(256), 0, st, gates, g_ld, c_prev, c_new, dh_out, dh_carry, dc_carry, dgates, dg_ld,
                       lengths, step, rows, n, reinterpret_cast<__bf16*>(dgb));
    return launch_ok("lstm_cell_bwd");
}

static int ensure_dynamic_lds(const void* kernel, size_t bytes);
// ------------------------------------------------------------------ layer-normalised cell: launch forms
// One block per row up to LN_MAX_SLOTS blocks (the backward's partial-sum slots), rows beyond that strided over the blocks; 64, 128 or 256
// threads by the width of a gate; the row (5n floats) and the cross-wave partials in dynamic LDS.
int ln_slots(int rows) { return rows < LN_MAX_SLOTS ? (rows < 1 ? 1 : rows) : LN_MAX_SLOTS; }
static int ln_threads(int n) { return n <= 64 ? 64 : n <= 128 ? 128 : 256; }
static size_t ln_lds(int n) { return (size_t)(LN_RED + 5L * n) * 4; }
int lstm_ln_cell_fwd(float* gates, int g_ld, const float* gy, const float* c_prev, const float* h_prev, float* c_new, float* h_new, const int* lengths, int step,
                     int rows, int n, void* hb_new, const LnCell& ln, float* xhat, float* rstd, hipStream_t st) {
    const size_t lds = ln_lds(n);
    SAT_REQUIRE(lds <= 160 * 1024, "lstm_ln_cell_fwd: n=%d needs %zu B of LDS (> 160 KiB)", n, lds);
    SAT_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(lstm_ln_cell_fwd_kernel), lds));
    hipLaunchKernelGGL(lstm_ln_cell_fwd_kernel, dim3(ln_slots(rows)), dim3(ln_threads(n)), lds, st, gates, g_ld, gy, c_prev, h_prev, c_new, h_new, lengths, step, rows, n,
                       reinterpret_cast<__bf16*>(hb_new), ln.gate_w, ln.gate_b, ln.cell_w, ln.cell_b, xhat, rstd);
    return launch_ok("lstm_ln_cell_fwd");
}
int lstm_ln_cell_bwd(const float* gates, int g_ld, const float* c_prev, const float* xhat, const float* rstd, const float* dh_out, float* dh_carry, float* dc_carry,
                     float* dgates, int dg_ld, const int* lengths, int step, int rows, int n, void* dgb, const LnCell& ln, float* part, hipStream_t st) {
    const size_t lds = ln_lds(n);
    SAT_REQUIRE(lds <= 160 * 1024, "lstm_ln_cell_bwd: n=%d needs %zu B of LDS (> 160 KiB)", n, lds);
    SAT_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(lstm_ln_cell_bwd_kernel), lds));
    hipLaunchKernelGGL(lstm_ln_cell_bwd_kernel, dim3(ln_slots(rows)), dim3(ln_threads(n)), lds, st, gates, g_ld, c_prev, xhat, rstd, dh_out, dh_carry, dc_carry, dgates,
                       dg_ld, lengths, step, rows, n, reinterpret_cast<__bf16*>(dgb), ln.gate_w, ln.cell_w, ln.cell_b, part);
    return launch_ok("lstm_ln_cell_bwd");
}

static int live_steps(const sat_decoder_dims& d, const sat_decoder_batch& b) {
    const int T1 = d.T - 1; int ts = 0;
    for (int t = 0; t < T1; ++t) if (b.step_offsets_host[t + 1] > b.step_offsets_host[t]) ts = t + 1;
    return ts;
}

static size_t att_fwd_lds(int L, int A, int vw) { return (size_t)(ATT_RMAX * L + ATT_RMAX * A + A + ATT_RMAX * ATT_THREADS * vw) * 4; }
static size_t att_bwd_lds(int L, int A, int D) { return (size_t)(2 * ATT_RMAX * L + ATT_RMAX * A + A + ATT_RMAX * D + ATTB_WAVES * ATT_RMAX * A + ATTB_WAVES * A) * 4; }

// The one place where the launch form of the attention step is decided.  launch_attention_fwd, launch_attention_bwd, attention_context_bwd
// and the query sat_attention_step_plan all read it from here.
//   forward  split : scores + context kernels.  Needs the score scratch, D, A and hc_ld multiples of 4 (float4 reads of the gate and of the
//                    annotations, float4 stores of Z / XZ) and ann, hc, Z, XZ on 16-byte boundaries.
//            single: attention_fwd_kernel<VW, RN>; VW = 4 (256-wide chunks of D) when D % 4 == 0 and ann is 16-byte aligned, else VW = 1 (64-wide).
//   backward split : dalpha + tanh kernels.  The dalpha kernel walks D in 16-byte vectors of ann and of its dz rows in LDS: D % 4 == 0 and
//                    ann on a 16-byte boundary (its bf16 copy on an 8-byte one).  The tanh kernel is scalar in A, L and every pointer.
//            single: attention_bwd_kernel<RN>, scalar throughout: any D, A, alignment.
//   context bwd    : dann_from_context_kernel<NQ>, scalar in D; NQ float4 of a (zero-padded) alphas row per slab.
// The bf16 copies (annotation stream in, gated context / dhc out) exist in the split kernels only.
int attention_plan(int op, int R, int L, int D, int A, int hc_ld, int T1, unsigned flags, AttPlan& p, const char* who) {
    p = AttPlan();
    SAT_REQUIRE(op >= ATT_OP_FWD && op <= ATT_OP_CONTEXT_BWD, "%s: op=%d (0 forward, 1 backward, 2 context backward)", who, op);
    SAT_REQUIRE(R >= 1 && L >= 1 && D >= 1 && T1 >= 1 && (op == ATT_OP_CONTEXT_BWD || (A >= 1 && hc_ld >= A + D)),
                "%s: bad shape (R=%d L=%d D=%d A=%d hc_ld=%d T1=%d)", who, R, L, D, A, hc_ld, T1);
    const bool scratch = flags & ATT_HAS_SCRATCH, ann_al = flags & ATT_ANN_ALIGNED, rows_al = flags & ATT_ROWS_ALIGNED;
    p.rn = R < ATT_RMAX ? R : ATT_RMAX;            // rows per pass, compile-time in the kernels
    p.passes = cdiv(R, p.rn);
    const int RN = p.rn;
    if (op == ATT_OP_FWD) {
        if (scratch && D % 4 == 0 && A % 4 == 0 && hc_ld % 4 == 0 && ann_al && rows_al) {
            p.form = ATT_FORM_SPLIT; p.vw = 4; p.dchunk = ATTC_DCH;
            p.lds0 = (size_t)(RN * A + A) * 4;                                                   // scores: [RN][A] q, [A] w
            p.lds1 = (size_t)((RN * L + 3) & ~3) * 4 + (size_t)16 * RN * 16 * 16;                // context: [RN][L] alpha, [16][RN][16] float4
        } else {
            p.form = ATT_FORM_SINGLE;
            const bool vec = D % 4 == 0 && ann_al;
            p.vw = vec ? 4 : 1;
            p.dchunk = vec ? 256 : 64;
            if (p.dchunk > D) p.dchunk = D;
            p.lds0 = att_fwd_lds(L, A, p.vw);
        }
    } else if (op == ATT_OP_BWD) {
        if (scratch && D % 4 == 0 && ann_al) {
            p.form = ATT_FORM_SPLIT; p.vw = 4;
            p.lds0 = (size_t)RN * D * 4;                                                         // dalpha: [RN][D] dz
            p.lds1 = (size_t)(RN * L + RN * ATTB_KCH + 32 * (RN + 1) * ATTB_KCH) * 4;            // tanh: [RN][L] ds, [RN][32] q, [32][RN + 1][32]
        } else {
            p.form = ATT_FORM_SINGLE; p.vw = 1;
            p.lds0 = att_bwd_lds(L, A, D);
        }
    } else {
        // location slab = NQ float4 per LDS row: 13 covers L <= 52 (7x7 maps) in one pass, 16 the 8x8 / 14x14 maps
        const int lq4 = (L + 3) / 4;
        p.form = ATT_FORM_SINGLE; p.rn = R; p.passes = 1; p.vw = 1;
        p.nq = (lq4 <= 13) ? 13 : 16;
        p.lq = (lq4 + p.nq - 1) / p.nq * p.nq;
        p.lds0 = (size_t)R * T1 * p.lq * 16;
    }
    if ((flags & ATT_HAS_BF16) && p.form != ATT_FORM_SPLIT) { p = AttPlan(); SAT_REQUIRE(false, "%s: the bf16 copies need the split kernels (aligned shapes)", who); }
    if (p.lds0 > 160 * 1024 || p.lds1 > 160 * 1024) {
        const size_t need = p.lds0 > p.lds1 ? p.lds0 : p.lds1;
        p = AttPlan();
        SAT_REQUIRE(false, "%s: R=%d L=%d D=%d A=%d T1=%d need %zu B of LDS (> 160 KiB)", who, R, L, D, A, T1, need);
    }
    return SAT_OK;
}
static bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// hipFuncAttributeMaxDynamicSharedMemorySize is a per-kernel maximum that stays set: raise it when a launch needs more than any launch of that
// kernel on this device did before, not at every time step (four host calls a step, ~170 per train step otherwise)
static int ensure_dynamic_lds(const void* kernel, size_t bytes) {
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, size_t> granted;
    int dev = 0;
    SAT_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    size_t& have = granted[std::make_pair(dev, kernel)];
    if (bytes <= have) return SAT_OK;
    SAT_CHECK_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    have = bytes;
    return SAT_OK;
}
static bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

static bool ann_bf16_enabled() { static const bool off = getenv("SAT_ANN_BF16") && !atoi(getenv("SAT_ANN_BF16")); return !off; }      // dev switch
static bool attention_split_enabled() {
    static const int no_split = getenv("SAT_ATT_FUSED") ? atoi(getenv("SAT_ATT_FUSED")) : 0;
    return !no_split;
}
template <int RN, typename TA>
static int attention_fwd_split(hipStream_t st, const TA* ann, const float* U, const float* hc, int hc_ld, const float* wf, const int* lengths, int step,
                               float* alphas, int T1, float* Z, float* XZ, int B, int R, int L, int D, int A, float* sc, __bf16* xzb, const AttPlan& pl) {
    const size_t lds_s = pl.lds0, lds_c = pl.lds1;
    SAT_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(attention_scores_kernel<RN>), lds_s));
    SAT_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(attention_context_kernel<RN, TA>), lds_c));
    // algorithmic bytes (per image-step): scores read att_enc U (L x A fp32) and the R query rows, write R x L raw scores; context streams the
    // image's annotations (L x D) ONCE for its R captions, reads scores + gates, writes alphas, z and the gated context
    const double N = (double)B * R;
    {
        ProfScope prof("attention_scores", 2.0 * N * L * A, 4.0 * ((double)B * L * A + N * (A + L)), st);
        hipLaunchKernelGGL(attention_scores_kernel<RN>, dim3(B, cdiv(L, ATTS_WAVES)), dim3(ATTS_WAVES * 64), lds_s, st, U, hc, hc_ld, wf, sc, R, L, A);
        SAT_TRY(launch_ok("attention_scores"));
    }
    ProfScope prof("attention_context", 2.0 * N * L * D, (double)sizeof(TA) * B * L * D + 4.0 * N * (2.0 * L + 3.0 * D), st);
    hipLaunchKernelGGL((attention_context_kernel<RN, TA>), dim3(B, cdiv(D, ATTC_DCH)), dim3(256), lds_c, st, ann, sc, hc, hc_ld, lengths, step, alphas, T1, Z, XZ, R, L, D, A, xzb);
    return launch_ok("attention_context");
}

int launch_attention_fwd(hipStream_t st, const float* ann, const float* U, const float* hc, int hc_ld, const float* wf,
                                const int* lengths, int step, float* alphas, int T1, float* Z, float* XZ, int B, int R, int L, int D, int A, float* sc, void* xzb_v,
                                const void* annb_v) {
    __bf16* xzb = reinterpret_cast<__bf16*>(xzb_v);
    const __bf16* annb = reinterpret_cast<const __bf16*>(annb_v);          // bf16 copy of ann for the context stream (split kernels only), or NULL
    static const int no_split = getenv("SAT_ATT_FUSED") ? atoi(getenv("SAT_ATT_FUSED")) : 0;
    const unsigned flags = (sc && !no_split ? ATT_HAS_SCRATCH : 0u) | (al16(ann) && (!annb || al8(annb)) ? ATT_ANN_ALIGNED : 0u) |
                           (al16(hc) && al16(Z) && al16(XZ) ? ATT_ROWS_ALIGNED : 0u) | (xzb || annb ? ATT_HAS_BF16 : 0u);
    AttPlan pl;
    SAT_TRY(attention_plan(ATT_OP_FWD, R, L, D, A, hc_ld, T1, flags, pl, "attention_fwd"));
    if (pl.form == ATT_FORM_SPLIT) {
        // scores and context as two chip-wide launches (scratch: raw scores (B*R, L))
        switch (pl.rn) {
            case 1: return annb ? attention_fwd_split<1, __bf16>(st, annb, U, hc, hc_ld, wf, lengths, step, alphas, T1, Z, XZ, B, R, L, D, A, sc, xzb, pl)
                                : attention_fwd_split<1, float>(st, ann, U, hc, hc_ld, wf, lengths, step, alphas, T1, Z, XZ, B, R, L, D, A, sc, xzb, pl);
            case 2: return annb ? attention_fwd_split<2, __bf16>(st, annb, U, hc, hc_ld, wf, lengths, step, alphas, T1, Z, XZ, B, R, L, D, A, sc, xzb, pl)
                                : attention_fwd_split<2, float>(st, ann, U, hc, hc_ld, wf, lengths, step, alphas, T1, Z, XZ, B, R, L, D, A, sc, xzb, pl);
            case 3: return annb ? attention_fwd_split<3, __bf16>(st, annb, U, hc, hc_ld, wf, lengths, step, alphas, T1, Z, XZ, B, R, L, D, A, sc, xzb, pl)
                                : attention_fwd_split<3, float>(st, ann, U, hc, hc_ld, wf, lengths, step, alphas, T1, Z, XZ, B, R, L, D, A, sc, xzb, pl);
            case 4: return annb ? attention_fwd_split<4, __bf16>(st, annb, U, hc, hc_ld, wf, lengths, step, alphas, T1, Z, XZ, B, R, L, D, A, sc, xzb, pl)
                                : attention_fwd_split<4, float>(st, ann, U, hc, hc_ld, wf, lengths, step, alphas, T1, Z, XZ, B, R, L, D, A, sc, xzb, pl);
            case 5: return annb ? attention_fwd_split<5, __bf16>(st, annb, U, hc, hc_ld, wf, lengths, step, alphas, T1, Z, XZ, B, R, L, D, A, sc, xzb, pl)
                                : attention_fwd_split<5, float>(st, ann, U, hc, hc_ld, wf, lengths, step, alphas, T1, Z, XZ, B, R, L, D, A, sc, xzb, pl);
            case 6: return annb ? attention_fwd_split<6, __bf16>(st, annb, U, hc, hc_ld, wf, lengths, step, alphas, T1, Z, XZ, B, R, L, D, A, sc, xzb, pl)
                                : attention_fwd_split<6, float>(st, ann, U, hc, hc_ld, wf, lengths, step, alphas, T1, Z, XZ, B, R, L, D, A, sc, xzb, pl);
            case 7: return annb ? attention_fwd_split<7, __bf16>(st, annb, U, hc, hc_ld, wf, lengths, step, alphas, T1, Z, XZ, B, R, L, D, A, sc, xzb, pl)
                                : attention_fwd_split<7, float>(st, ann, U, hc, hc_ld, wf, lengths, step, alphas, T1, Z, XZ, B, R, L, D, A, sc, xzb, pl);
            default: return annb ? attention_fwd_split<8, __bf16>(st, annb, U, hc, hc_ld, wf, lengths, step, alphas, T1, Z, XZ, B, R, L, D, A, sc, xzb, pl)
                                 : attention_fwd_split<8, float>(st, ann, U, hc, hc_ld, wf, lengths, step, alphas, T1, Z, XZ, B, R, L, D, A, sc, xzb, pl);
        }
    }
    const bool vec = pl.vw == 4;
    const int dchunk = pl.dchunk;
    const size_t lds = pl.lds0;
    dim3 grid(B, cdiv(D, dchunk));
    const int RN = pl.rn;
#define SAT_ATTF(VWV, RNV)                                                                                                                  \
    case RNV:                                                                                                                               \
        SAT_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(attention_fwd_kernel<VWV, RNV>), lds)); \
        hipLaunchKernelGGL((attention_fwd_kernel<VWV, RNV>), grid, dim3(ATTF_THREADS), lds, st, ann, U, hc, hc_ld, wf, lengths, step, alphas, T1, Z, XZ, R, L, D, A, dchunk); \
        break;
    if (vec) {
        switch (RN) { SAT_ATTF(4, 1) SAT_ATTF(4, 2) SAT_ATTF(4, 3) SAT_ATTF(4, 4) SAT_ATTF(4, 5) SAT_ATTF(4, 6) SAT_ATTF(4, 7) SAT_ATTF(4, 8) default: break; }
    } else {
        switch (RN) { SAT_ATTF(1, 1) SAT_ATTF(1, 2) SAT_ATTF(1, 3) SAT_ATTF(1, 4) SAT_ATTF(1, 5) SAT_ATTF(1, 6) SAT_ATTF(1, 7) SAT_ATTF(1, 8) default: break; }
    }
#undef SAT_ATTF
    return launch_ok("attention_fwd");
}

template <int RN, typename TA>
static int attention_bwd_split_t(hipStream_t st, const TA* ann, const float* U, const float* hc, int hc_ld, const float* wf, const int* lengths, int step,
                                 const float* alphas, const float* dalphas, int T1, const float* Zs, const float* dZ_out, const float* dXZ, float* DZ, float* dhc,
                                 int dhc_ld, float* dU, float* dwf_part, float* da, int B, int R, int L, int D, int A, __bf16* dhcb, const AttPlan& pl) {
    const size_t lds_a = pl.lds0, lds_t = pl.lds1;
    SAT_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(attention_bwd_dalpha_kernel<RN, TA>), lds_a));
    SAT_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(attention_bwd_tanh_kernel<RN>), lds_t));
    // algorithmic bytes: dalpha streams the annotations once per image, reads the R gradient rows of z / gated z / the gate (3 x D) and z, writes dz and
    // d(alpha); tanh reads att_enc and d(alpha), alphas, the queries, and adds into dU (read + write)
    const double N = (double)B * R;
    {
        ProfScope prof("attention_bwd_dalpha", 2.0 * N * L * D, (double)sizeof(TA) * B * L * D + 4.0 * N * (5.0 * D + 2.0 * L), st);
        hipLaunchKernelGGL((attention_bwd_dalpha_kernel<RN, TA>), dim3(B, cdiv(L, 16)), dim3(1024), lds_a, st, ann, hc, hc_ld, lengths, step, dalphas, T1, Zs, dZ_out, dXZ, DZ, dhc,
                           dhc_ld, da, R, L, D, A, dhcb);
        SAT_TRY(launch_ok("attention_bwd_dalpha"));
    }
    ProfScope prof("attention_bwd_tanh", 4.0 * N * L * A, 4.0 * (3.0 * B * L * A + N * (2.0 * A + 2.0 * L)), st);
    hipLaunchKernelGGL(attention_bwd_tanh_kernel<RN>, dim3(B, cdiv(A, ATTB_KCH)), dim3(1024), lds_t, st, U, hc, hc_ld, wf, lengths, step, alphas, T1, da, dhc, dhc_ld, dU,
                       dwf_part, R, L, A, dhcb);
    return launch_ok("attention_bwd_tanh");
}
// One attention backward step in the form attention_plan decides; `da` ((B*R, L) floats, or NULL) is the split pair's scratch.
int launch_attention_bwd(hipStream_t st, const float* ann, const float* U, const float* hc, int hc_ld, const float* wf, const int* lengths, int step,
                         const float* alphas, const float* dalphas, int T1, const float* Zs, const float* dZ_out, const float* dXZ, float* DZ, float* dhc,
                         int dhc_ld, float* dU, float* dwf_part, float* da, int B, int R, int L, int D, int A, void* dhcb_v, const void* annb_v) {
    __bf16* dhcb = reinterpret_cast<__bf16*>(dhcb_v);
    const __bf16* annb = reinterpret_cast<const __bf16*>(annb_v);
    const unsigned flags = (da ? ATT_HAS_SCRATCH : 0u) | (al16(ann) && (!annb || al8(annb)) ? ATT_ANN_ALIGNED : 0u) | (dhcb || annb ? ATT_HAS_BF16 : 0u);
    AttPlan pl;
    SAT_TRY(attention_plan(ATT_OP_BWD, R, L, D, A, hc_ld, T1, flags, pl, "attention_bwd"));
    SAT_REQUIRE(dhc_ld >= A + D, "attention_bwd: dhc_ld %d < A+D", dhc_ld);
    if (pl.form == ATT_FORM_SPLIT) {
#define SAT_ATTB(RNV) case RNV: return annb ? attention_bwd_split_t<RNV, __bf16>(st, annb, U, hc, hc_ld, wf, lengths, step, alphas, dalphas, T1, Zs, dZ_out, dXZ, DZ, dhc, dhc_ld, dU, dwf_part, da, B, R, L, D, A, dhcb, pl) \
                                            : attention_bwd_split_t<RNV, float>(st, ann, U, hc, hc_ld, wf, lengths, step, alphas, dalphas, T1, Zs, dZ_out, dXZ, DZ, dhc, dhc_ld, dU, dwf_part, da, B, R, L, D, A, dhcb, pl);
        switch (pl.rn) { SAT_ATTB(1) SAT_ATTB(2) SAT_ATTB(3) SAT_ATTB(4) SAT_ATTB(5) SAT_ATTB(6) SAT_ATTB(7) default: SAT_ATTB(8) }
#undef SAT_ATTB
    }
    // one block per image, scalar in D and A: the shapes and views the vector loads of the dalpha kernel cannot take (and the dev switch)
    typedef void (*attb_fn)(const float*, const float*, const float*, int, const float*, const int*, int, const float*, const float*, int, const float*,
                            const float*, const float*, float*, float*, int, float*, float*, int, int, int, int);
    attb_fn attb = nullptr;
    switch (pl.rn) {
        case 1: attb = attention_bwd_kernel<1>; break; case 2: attb = attention_bwd_kernel<2>; break; case 3: attb = attention_bwd_kernel<3>; break;
        case 4: attb = attention_bwd_kernel<4>; break; case 5: attb = attention_bwd_kernel<5>; break; case 6: attb = attention_bwd_kernel<6>; break;
        case 7: attb = attention_bwd_kernel<7>; break; default: attb = attention_bwd_kernel<8>; break;
    }
    SAT_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(attb), pl.lds0));
    hipLaunchKernelGGL(attb, dim3(B), dim3(ATTB_THREADS), pl.lds0, st, ann, U, hc, hc_ld, wf, lengths, step, alphas, dalphas, T1, Zs, dZ_out, dXZ, DZ, dhc, dhc_ld,
                       dU, dwf_part, R, L, D, A);
    return launch_ok("attention_bwd");
}

// ------------------------------------------------------------------ output stage for packed rows [p0, p1)
static int flush_outputs(hipStream_t st, const sat_decoder_dims& d, const sat_decoder_params& p, const sat_decoder_batch& b,
                         const Ws& w, float* logits, int p0, int p1) {
    const int rows = p1 - p0;
    if (rows <= 0) return SAT_OK;
    const long N = (long)d.B * d.R;
    const float* H1 = w.H_all + ((long)(d.layers - 1) * d.T + 1) * N * d.n;   // top layer's hidden state AFTER each step (F8: the new h)
    float* u = w.Uact + (long)p0 * d.m;
    const int* rows_map = b.src_row + p0;
    if (d.deep_output) {
        SAT_TRY(gemm(st, A_ROW, B_ROW, H1, d.n, p.out_hidden, d.n, u, d.m, rows, d.m, d.n, 0, EPI_NONE, nullptr, rows_map));
        SAT_TRY(gemm(st, A_ROW, B_ROW, w.Z, d.D, p.out_context, d.D, u, d.m, rows, d.m, d.D, 1, EPI_ADD_TANH, nullptr, rows_map, nullptr, w.Y, d.m));
    } else {
        SAT_TRY(gemm(st, A_ROW, B_ROW, H1, d.n, p.out_hidden, d.n, u, d.m, rows, d.m, d.n, 0, EPI_NONE, nullptr, rows_map));
    }
    const float* uin = u;
    if (d.dropout > 0.f) {                       // DeepOutput.dropout (model.py:130) on the packed rows
        float* ud = w.Udrop + (long)p0 * d.m;
        hipLaunchKernelGGL(dropout_rows_kernel, dim3(cdiv((long)rows * d.m, 256)), dim3(256), 0, st, u, ud, (long)rows * d.m, d.m, d.dropout,
                           (unsigned long long)d.dropout_seed, 2u, (long)p0, d.variational_dropout ? b.src_row : (const int*)nullptr, d.variational_dropout ? (int)N : 0);
        SAT_TRY(launch_ok("output dropout"));
        uin = ud;
    }
    if (w.Wb_out) {          // bf16 mode: vocabulary projection on bf16 copies of both operands.  The weight copy is made at the first flush of a
                             // forward pass (p0 == 0) and again at every later one only under weight tying with max-norm renormalisation: the
                             // embedding table IS the output weight then and is edited during the loop (scheduled sampling flushes every step)
        if (p0 == 0 || (p.out_w == p.embedding && d.embed_max_norm > 0.f)) SAT_TRY(cast_bf16(st, p.out_w, w.Wb_out, (long)d.V * d.m));
        SAT_TRY(cast_bf16(st, uin, w.Ub + (long)p0 * d.m, (long)rows * d.m));
        return gemm_bb_nt(st, w.Ub + (long)p0 * d.m, d.m, w.Wb_out, d.m, logits + (long)p0 * d.V, d.V, rows, d.V, d.m, p.out_b ? EPI_BIAS : EPI_NONE, p.out_b);
    }
    return gemm(st, A_ROW, B_ROW, uin, d.m, p.out_w, d.m, logits + (long)p0 * d.V, d.V, rows, d.V, d.m, 0,
                p.out_b ? EPI_BIAS : EPI_NONE, p.out_b);
}

int decoder_fwd(const sat_decoder_dims& d, const sat_decoder_params& p, const sat_decoder_batch& b, float* logits, float* alphas,
                       char* ws, size_t ws_bytes, hipStream_t st) {
    const bool ln = ln_on(p);
    Ws w = layout(d, ws, ln);
    t_bf16_mfma = d.precision ? 1 : 0;
    SAT_REQUIRE(ws_bytes >= w.total, "decoder_fwd: workspace %zu < %zu bytes", ws_bytes, w.total);
    SAT_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "decoder: workspace must be 256-byte aligned");
    const int N = d.B * d.R, T1 = d.T - 1, HCW = d.A + d.D + 4 * d.n, n = d.n, A = d.A, D = d.D, m = d.m;
    const int NL = d.layers, top = NL - 1;
    const long LS = (long)(T1 + 1) * N * n;                                   // layer stride of H_all / C_all
    auto Hs = [&](int t, int l) { return w.H_all + l * LS + (long)t * N * n; };
    auto Cs = [&](int t, int l) { return w.C_all + l * LS + (long)t * N * n; };
    auto GUs = [&](int t, int l) { return w.GU + ((long)(l - 1) * T1 + t) * N * 4 * n; };
    auto LnX = [&](int t, int l) { return w.ln_xhat + ((long)l * T1 + t) * N * 5 * n; };       // layer-normalised cell: saved for the backward
    auto LnR = [&](int t, int l) { return w.ln_rstd + ((long)l * T1 + t) * N * 5; };
    const int ts = live_steps(d, b);
    SAT_REQUIRE(b.step_offsets_host[T1] == d.P, "decoder: step_offsets[T-1]=%d != P=%d", b.step_offsets_host[T1], d.P);
    for (int t = 0; t < ts; ++t) SAT_REQUIRE(b.teacher_host[t] || t > 0, "decoder: step 0 must be teacher forced");

    // packed parameters: Wcat = [W_d ; W_beta ; W_hh] (HCW, n), bcat = [0 ; b_beta ; b_ih + b_hh]
    const bool use_b = w.Hb != nullptr && attention_split_enabled();
    SAT_TRY(pack_step_weights(d, p, w.Wcat, use_b ? w.Wcat_b : (__bf16*)nullptr, w.bcat, w.bup, st, d.weight_drop, (unsigned long long)d.dropout_seed));
    // weight-drop on the stacked layers: masked fp32 copies for this call, one launch (layer 0's mask went into Wcat above)
    const float* up_w_hh[SAT_MAX_LSTM_LAYERS] = {};
    for (int l = 1; l < NL; ++l) up_w_hh[l - 1] = w.Wup ? w.Wup + (long)(l - 1) * 4 * n * n : p.up_w_hh[l - 1];
    if (w.Wup) {
        float* dst[SAT_MAX_LSTM_LAYERS] = {};
        for (int l = 1; l < NL; ++l) dst[l - 1] = w.Wup + (long)(l - 1) * 4 * n * n;
        SAT_TRY(weight_drop(p.up_w_hh, dst, nullptr, NL - 1, 4L * n * n, 1, d.weight_drop, (unsigned long long)d.dropout_seed, st));
    }
    const int vper = d.variational_dropout ? N : 0;         // variational dropout: one embedding / output mask row per caption (mask_row)

    // att_enc and the annotation mean; without dropout InitLSTM (model.py:76-81) on the B images, then the raw reshape over the repeated rows (F3)
    SAT_TRY(image_begin(d, p, b.ann, d.B, w.U, w.mean, d.dropout > 0.f ? nullptr : w.f, w.init_img, st));
    if (d.dropout > 0.f) {
        // dropout acts on the mean of the repeated annotations: every caption row has its own mask, so run the
        // two Linears on N rows; the (N, 2n) result IS the (2, N, n) state buffer (raw reshape, F3)
        hipLaunchKernelGGL(init_mean_rows_kernel, dim3(cdiv((long)N * D, 256)), dim3(256), 0, st, w.mean, w.mean_rows, N, d.R, D, d.dropout, (unsigned long long)d.dropout_seed);
        SAT_TRY(launch_ok("init_mean_rows"));
        SAT_TRY(gemm(st, A_ROW, B_ROW, w.mean_rows, D, p.init_f_w, D, w.f_rows, m, N, m, D, 0, EPI_BIAS, p.init_f_b));
        SAT_TRY(gemm(st, A_ROW, B_ROW, w.f_rows, m, p.init_i_w, m, w.init_rows, 2 * n * NL, N, 2 * n * NL, m, 0, EPI_BIAS, p.init_i_b));
        for (int l = 0; l < NL; ++l) {
            SAT_TRY(dev_copy_bytes(st, Hs(0, l), w.init_rows + (long)l * N * n, (size_t)N * n * 4));
            SAT_TRY(dev_copy_bytes(st, Cs(0, l), w.init_rows + (long)(NL + l) * N * n, (size_t)N * n * 4));
        }
    } else {
        hipLaunchKernelGGL(init_expand_kernel, dim3(cdiv(2L * NL * N * n, 256)), dim3(256), 0, st, w.init_img, w.H_all, w.C_all, N, d.R, n, NL, LS);
        SAT_TRY(launch_ok("init_expand"));
    }

    // bf16 mode, one layer: the per-step GEMMs read bf16 copies (state written by the cell kernel, gated context by the attention
    // kernel, weights cast here once) through the direct-to-LDS kernel instead of rounding fp32 operands in registers every step
    const __bf16* annb = (w.annb && attention_split_enabled() && ann_bf16_enabled() && al16(b.ann)) ? w.annb : nullptr;
    if (annb) SAT_TRY(cast_bf16(st, b.ann, w.annb, (long)d.B * d.L * D));
    if (use_b) {
        hipLaunchKernelGGL(cast_block_bf16_kernel, dim3(cdiv((long)4 * n * (D / 4), 256)), dim3(256), 0, st, p.w_ih + m, (long)(m + D), w.Wz_b, 4 * n, D);
        SAT_TRY(launch_ok("cast W_ih[:, m:]"));
        SAT_TRY(cast_bf16(st, Hs(0, 0), w.Hb, (long)N * n));
    }
    // alphas of steps that never run stay zero (model.py:506)
    if (ts < T1) SAT_TRY(dev_fill_bytes(st, alphas, 0, (size_t)N * T1 * d.L * 4));

    // tokens + embeddings + the embedding half of the LSTM input GEMM for every teacher-forced step, in one batch
    SAT_TRY(dev_fill_bytes(st, w.Tok, 0xFF, (size_t)T1 * N * 4));       // -1: no token
    for (int t = 0; t < ts;) {          // one launch per run of teacher-forced steps (the whole caption when epsilon = 1)
        if (!b.teacher_host[t]) { ++t; continue; }
        int t1 = t + 1;
        while (t1 < ts && b.teacher_host[t1]) ++t1;
        hipLaunchKernelGGL(teacher_tokens_kernel, dim3(cdiv(N, 256), t1 - t), dim3(256), 0, st, b.caps, b.lengths, w.Tok + (long)t * N, N, d.T, t);
        SAT_TRY(launch_ok("teacher_tokens"));
        t = t1;
    }
    auto renorm = [&](const int* tok, int count) -> int {
        if (!(d.embed_max_norm > 0.f)) return SAT_OK;
        hipLaunchKernelGGL(embedding_mark_kernel, dim3(cdiv(count, 256)), dim3(256), 0, st, tok, count, w.flags, d.V);
        SAT_TRY(launch_ok("embedding_mark"));
        hipLaunchKernelGGL(embedding_renorm_kernel, dim3(d.V), dim3(64), 0, st, p.embedding, w.flags, m, d.embed_max_norm);
        return launch_ok("embedding_renorm");
    };
    if (d.embed_max_norm > 0.f) SAT_TRY(dev_fill_bytes(st, w.flags, 0, (size_t)d.V * 4));
    if (ts > 0) {
        SAT_TRY(renorm(w.Tok, ts * N));
        hipLaunchKernelGGL(gather_rows_kernel, dim3(ts * N), dim3(64), 0, st, p.embedding, w.Tok, w.Y, ts * N, m, d.V, d.embedding_dropout, (unsigned long long)d.dropout_seed, 0L, vper);
        SAT_TRY(launch_ok("embedding gather"));
        SAT_TRY(gemm(st, A_ROW, B_ROW, w.Y, m, p.w_ih, m + D, w.GY, 4 * n, ts * N, 4 * n, m));
    }

    int pending = 0;
    for (int t = 0; t < ts; ++t) {
        float* hc = w.HC + (long)t * N * HCW;
        if (!b.teacher_host[t]) {
            // scheduled sampling (model.py:521-523): feed argmax of the previous step's logits
            SAT_TRY(flush_outputs(st, d, p, b, w, logits, b.step_offsets_host[pending], b.step_offsets_host[t]));
            pending = t;
            if (d.embed_max_norm > 0.f) {       // the chosen rows are renormalised in place between the decision and the gather (model.py:158-164)
                hipLaunchKernelGGL(argmax_tokens_kernel, dim3(N), dim3(256), 0, st, logits, b.prow + (long)(t - 1) * N, b.lengths, w.Tok + (long)t * N, d.V, t);
                SAT_TRY(launch_ok("argmax_tokens"));
                SAT_TRY(renorm(w.Tok + (long)t * N, N));
                hipLaunchKernelGGL(gather_rows_kernel, dim3(N), dim3(64), 0, st, p.embedding, w.Tok + (long)t * N, w.Y + (long)t * N * m, N, m, d.V, d.embedding_dropout, (unsigned long long)d.dropout_seed, (long)t * N, vper);
                SAT_TRY(launch_ok("embedding gather"));
            } else {                            // decision + embedding row in one launch
                hipLaunchKernelGGL(argmax_gather_kernel, dim3(N), dim3(256), 0, st, logits, b.prow + (long)(t - 1) * N, b.lengths, w.Tok + (long)t * N, d.V, t, p.embedding,
                                   w.Y + (long)t * N * m, m, d.embedding_dropout, (unsigned long long)d.dropout_seed, (long)t * N, vper);
                SAT_TRY(launch_ok("argmax + embedding gather"));
            }
            SAT_TRY(gemm(st, A_ROW, B_ROW, w.Y + (long)t * N * m, m, p.w_ih, m + D, w.GY + (long)t * N * 4 * n, 4 * n, N, 4 * n, m));
        }
        // [q | beta | gates_h] = h_{t-1} * Wcat^T + bcat, sigmoid on the beta columns.  Attention and the gate read the TOP
        // layer's state (h[-1], model.py:533,538); the recurrent term of layer 0 reads layer 0's.
        if (use_b) {
            SAT_TRY(gemm_bb_nt(st, w.Hb + (long)t * N * n, n, w.Wcat_b, n, hc, HCW, N, HCW, n, EPI_BIAS_SIGMOID_RANGE, w.bcat, 0, A, A + D));
        } else if (NL == 1) {
            SAT_TRY(gemm(st, A_ROW, B_ROW, Hs(t, 0), n, w.Wcat, n, hc, HCW, N, HCW, n, 0, EPI_BIAS_SIGMOID_RANGE, w.bcat,
                         nullptr, nullptr, nullptr, 0, A, A + D));
        } else {
            SAT_TRY(gemm(st, A_ROW, B_ROW, Hs(t, top), n, w.Wcat, n, hc, HCW, N, A + D, n, 0, EPI_BIAS_SIGMOID_RANGE, w.bcat,
                         nullptr, nullptr, nullptr, 0, A, A + D));
            SAT_TRY(gemm(st, A_ROW, B_ROW, Hs(t, 0), n, w.Wcat + (long)(A + D) * n, n, hc + A + D, HCW, N, 4 * n, n, 0, EPI_BIAS, w.bcat + A + D));
        }
        SAT_TRY(launch_attention_fwd(st, b.ann, w.U, hc, HCW, p.att_f, b.lengths, t, alphas, T1, w.Z + (long)t * N * D, w.XZ + (long)t * N * D,
                                     d.B, d.R, d.L, D, A, w.SC, use_b ? w.XZb : nullptr, annb));
        // gates += (beta*z) * W_ih[:, m:]^T
        if (use_b) SAT_TRY(gemm_bb_nt(st, w.XZb, D, w.Wz_b, D, hc + A + D, HCW, N, 4 * n, D, EPI_NONE, nullptr, 1));
        else SAT_TRY(gemm(st, A_ROW, B_ROW, w.XZ + (long)t * N * D, D, p.w_ih + m, m + D, hc + A + D, HCW, N, 4 * n, D, 1));
        if (ln) {       // the layer-normalised cell: the same single launch in the step
            SAT_TRY(lstm_ln_cell_fwd(hc + A + D, HCW, w.GY + (long)t * N * 4 * n, Cs(t, 0), Hs(t, 0), Cs(t + 1, 0), Hs(t + 1, 0), b.lengths, t, N, n,
                                     use_b ? w.Hb + (long)(t + 1) * N * n : (__bf16*)nullptr, ln_layer(p, 0), LnX(t, 0), LnR(t, 0), st));
        } else {
            hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3(cdiv((long)N * n, 256)), dim3(256), 0, st, hc + A + D, HCW, w.GY + (long)t * N * 4 * n,
                               Cs(t, 0), Hs(t, 0), Cs(t + 1, 0), Hs(t + 1, 0), b.lengths, t, N, n, use_b ? w.Hb + (long)(t + 1) * N * n : (__bf16*)nullptr);
            SAT_TRY(launch_ok("lstm_cell_fwd"));
        }
        for (int l = 1; l < NL; ++l) {          // stacked layers: input = the layer below's new h (nn.LSTM, no inter-layer dropout: model.py:175-180)
            float* gu = GUs(t, l);
            SAT_TRY(gemm(st, A_ROW, B_ROW, Hs(t + 1, l - 1), n, p.up_w_ih[l - 1], n, gu, 4 * n, N, 4 * n, n, 0, EPI_BIAS, w.bup + (long)(l - 1) * 4 * n));
            SAT_TRY(gemm(st, A_ROW, B_ROW, Hs(t, l), n, up_w_hh[l - 1], n, gu, 4 * n, N, 4 * n, n, 1));
            if (ln) {
                SAT_TRY(lstm_ln_cell_fwd(gu, 4 * n, nullptr, Cs(t, l), Hs(t, l), Cs(t + 1, l), Hs(t + 1, l), b.lengths, t, N, n, nullptr, ln_layer(p, l), LnX(t, l),
                                         LnR(t, l), st));
                continue;
            }
            hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3(cdiv((long)N * n, 256)), dim3(256), 0, st, gu, 4 * n, (const float*)nullptr,
                               Cs(t, l), Hs(t, l), Cs(t + 1, l), Hs(t + 1, l), b.lengths, t, N, n);
            SAT_TRY(launch_ok("lstm_cell_fwd (stacked layer)"));
        }
    }
    return flush_outputs(st, d, p, b, w, logits, b.step_offsets_host[pending], b.step_offsets_host[ts]);
}

// Q of the activation regularisers: the (t - 1, t) pairs of live steps = P minus the captions that run at step 0
static long reg_pairs(const sat_decoder_batch& b, long P) { return P - (b.step_offsets_host[1] - b.step_offsets_host[0]); }

int decoder_reg_fwd(const sat_decoder_dims& d, const sat_decoder_batch& b, char* ws, size_t ws_bytes, void* scratch, float* out, hipStream_t st) {
    Ws w = layout(d, ws);
    SAT_REQUIRE(ws_bytes >= w.total, "decoder_reg_fwd: workspace %zu < %zu bytes", ws_bytes, w.total);
    const int N = d.B * d.R, T1 = d.T - 1;
    SAT_REQUIRE(b.step_offsets_host[T1] == d.P, "decoder_reg_fwd: step_offsets[T-1]=%d != P=%d", b.step_offsets_host[T1], d.P);
    const float* H1 = w.H_all + ((long)(d.layers - 1) * d.T + 1) * N * d.n;    // top layer's hidden state after each step, as flush_outputs reads it
    return activation_reg_fwd(H1, b.lengths, N, T1, d.n, d.P, reg_pairs(b, d.P), scratch, out, st);
}

int decoder_bwd(const sat_decoder_dims& d, const sat_decoder_params& p, const sat_decoder_batch& b, const float* dlogits,
                       const float* alphas, const float* dalphas, const sat_decoder_params& g, float* dann, char* ws, size_t ws_bytes, hipStream_t st,
                       hipStream_t side, hipEvent_t fork_event, const float* reg_gscale) {
    const bool ln = ln_on(p);
    SAT_REQUIRE(ln == ln_on(g), "decoder_bwd: the layer-norm tensors are %s in the parameters and %s in the gradients", ln ? "set" : "NULL", ln ? "NULL" : "set");
    Ws w = layout(d, ws, ln);
    t_bf16_mfma = d.precision ? 1 : 0;
    SAT_REQUIRE(ws_bytes >= w.total, "decoder_bwd: workspace %zu < %zu bytes", ws_bytes, w.total);
    SAT_REQUIRE(!side || fork_event, "decoder_bwd: side stream without event");
    // Everything after the time loop is either CRITICAL (on the way to dann, which the encoder backward waits for: dU * att_enc, the
    // attention context backward, the InitLSTM data gradients down to dmean, dann_add_mean) or LEAF (writes a parameter gradient in g.* and
    // feeds nothing else: the k-major weight-gradient products, the column sums, dY and the embedding gradient, the bias copies; also the
    // output layer's three parameter gradients, whose operands are complete before the loop).  Without a side stream both run interleaved
    // on `st`, as they always have.  With one, the critical part is issued first on `st`, `fork_event` is recorded on `st` behind the last
    // kernel whose output the leaf part reads (the InitLSTM df product), `side` waits for it once, and the leaf part is issued on `side` in
    // its old order with a scratch set of its own.  The call does not join: the caller makes `st` wait for `side` before g.* is read.
    // What the leaf part reads, and why nothing on `st` can change it between the fork and the caller's join:
    //   dlogits, Uact / Udrop, H_all, Z, Y, XZ, Tok, ann, f / mean (f_rows / mean_rows), parameters   written by the forward pass or the caller only
    //   dY      scattered dA before the loop (on st); from then on read and written by leaf launches only
    //   DHC, DGU  written by the time loop; read by leaf products only
    //   dU, dwf_part  accumulated by the time loop; dU is read by both parts (dann and g.att_enc), written by neither
    //   dinit_img, df (init_rows, df_rows)  written by the critical InitLSTM chain BEFORE the event, never again
    //   mean_rows  the critical chain used to put d(mean rows) back into it while g.init_f_w still wants the forward's values: it has a
    //              buffer of its own now (dmean_rows)
    //   emb_count / emb_offset / emb_cursor / emb_list, colpart2, slab2   leaf scratch; st keeps colpart and slab
    //   ln_part   (layer-normalised cell) zeroed before and accumulated by the time loop; read by the leaf sums over its slots only
    // The critical launches after the event write dmean, dmean_rows and dann only.
    const bool fork = side != nullptr;
    const hipStream_t ls = fork ? side : st;                    // where the leaf part goes
    Ws wl = w;                                                  // ... and the scratch its column sums and split-K products use
    if (fork) { wl.colpart = w.colpart2; wl.slab = w.slab2; }
    const int N = d.B * d.R, T1 = d.T - 1, HCW = d.A + d.D + 4 * d.n, n = d.n, A = d.A, D = d.D, m = d.m, V = d.V, P = d.P;
    const int ts = live_steps(d, b);
    const int KR = ts * N;                              // rows of the time-major padded buffers that were touched
    const int NL = d.layers, top = NL - 1;
    const long LS = (long)(T1 + 1) * N * n;
    auto Hs = [&](int t, int l) { return w.H_all + l * LS + (long)t * N * n; };
    auto Cs = [&](int t, int l) { return w.C_all + l * LS + (long)t * N * n; };
    auto GUs = [&](int t, int l) { return w.GU + ((long)(l - 1) * T1 + t) * N * 4 * n; };
    auto DGUs = [&](int t, int l) { return w.DGU + ((long)(l - 1) * T1 + t) * N * 4 * n; };
    auto dHcs = [&](int l) { return w.dHc + (long)l * N * n; };
    auto dCcs = [&](int l) { return w.dCc + (long)l * N * n; };
    auto LnX = [&](int t, int l) { return w.ln_xhat + ((long)l * T1 + t) * N * 5 * n; };
    auto LnR = [&](int t, int l) { return w.ln_rstd + ((long)l * T1 + t) * N * 5; };
    auto LnP = [&](int l) { return w.ln_part + (long)l * w.ln_nslots * 10 * n; };
    float* const slab = w.slab; const long se = w.slab_elems;
    // weight-drop: the state gradients flow through the masked matrices the forward left in the workspace (Wcat, Wup)
    const float* up_w_hh[SAT_MAX_LSTM_LAYERS] = {};
    for (int l = 1; l < NL; ++l) up_w_hh[l - 1] = w.Wup ? w.Wup + (long)(l - 1) * 4 * n * n : p.up_w_hh[l - 1];

    SAT_TRY(dev_fill_bytes(st, w.zero_begin, 0, (size_t)(w.zero_end - w.zero_begin)));       // dHout, dZout, dHc, dCc, dU, dwf_part
    if (NL > 1 && KR < T1 * N) SAT_TRY(dev_fill_bytes(st, w.DGU, 0, (size_t)(NL - 1) * T1 * N * 4 * n * 4));
    if (ln) SAT_TRY(dev_fill_bytes(st, w.ln_part, 0, (size_t)NL * w.ln_nslots * 10 * n * 4));

    // ---- output layer, all packed rows at once (DeepOutput backward)
    float* const lslab = wl.slab;
    // leaf: output.output.weight / bias
    auto leaf_out_w = [&]() -> int {
        if (P > 0) {
            SAT_TRY(gemm(ls, A_KMAJOR, B_KMAJOR, dlogits, V, d.dropout > 0.f ? w.Udrop : w.Uact, m, g.out_w, m, V, m, P, 0, EPI_NONE, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, lslab, se));
            if (g.out_b) SAT_TRY(colsum(ls, wl, dlogits, V, P, V, g.out_b));
        } else {
            SAT_TRY(dev_fill_bytes(ls, g.out_w, 0, (size_t)V * m * 4));
            if (g.out_b) SAT_TRY(dev_fill_bytes(ls, g.out_b, 0, (size_t)V * 4));
        }
        return SAT_OK;
    };
    // leaf: output.hidden.weight / output.context.weight from the scattered dA; dY then becomes the embedding gradient's accumulator
    auto leaf_out_hidden = [&]() -> int {
        const float* H1 = Hs(1, top);
        SAT_TRY(gemm(ls, A_KMAJOR, B_KMAJOR, w.dY, m, H1, n, g.out_hidden, n, m, n, KR, 0, EPI_NONE, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, lslab, se));
        if (d.deep_output)
            SAT_TRY(gemm(ls, A_KMAJOR, B_KMAJOR, w.dY, m, w.Z, D, g.out_context, D, m, D, KR, 0, EPI_NONE, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, lslab, se));
        else
            SAT_TRY(dev_fill_bytes(ls, w.dY, 0, (size_t)T1 * N * m * 4));     // shallow output does not see the embedding
        return SAT_OK;
    };
    if (P > 0) {
        SAT_TRY(gemm(st, A_ROW, B_KMAJOR, dlogits, V, p.out_w, m, w.dA, m, P, m, V, 0, d.deep_output ? EPI_MUL_DTANH : EPI_NONE, nullptr,
                     nullptr, nullptr, w.Uact, m, 0, 0, slab, se));           // few output tiles, long reduction over the vocabulary: split-K
        if (d.dropout > 0.f) {
            hipLaunchKernelGGL(dropout_rows_kernel, dim3(cdiv((long)P * m, 256)), dim3(256), 0, st, w.dA, w.dA, (long)P * m, m, d.dropout,
                               (unsigned long long)d.dropout_seed, 2u, 0L, d.variational_dropout ? b.src_row : (const int*)nullptr, d.variational_dropout ? N : 0);
            SAT_TRY(launch_ok("output dropout bwd"));
        }
    }
    if (!fork) SAT_TRY(leaf_out_w());
    if (P > 0) {
        SAT_TRY(gemm(st, A_ROW, B_KMAJOR, w.dA, m, p.out_hidden, n, w.dHout, n, P, n, m, 0, EPI_NONE, nullptr, nullptr, b.src_row));
        if (d.deep_output)
            SAT_TRY(gemm(st, A_ROW, B_KMAJOR, w.dA, m, p.out_context, D, w.dZout, D, P, D, m, 0, EPI_NONE, nullptr, nullptr, b.src_row));
    }
    // AR / TAR: their direct gradient with respect to the top-layer states joins the output layer's in dHout; the time loop carries it on
    if (reg_gscale && P > 0) SAT_TRY(activation_reg_bwd(Hs(1, top), b.lengths, N, T1, n, P, reg_pairs(b, P), reg_gscale, w.dHout, st));
    // dA in time-major padded rows (zeros for finished captions): operand of the weight-grad GEMMs and of dY
    hipLaunchKernelGGL(scatter_rows_kernel, dim3(T1 * N), dim3(64), 0, st, w.dA, b.prow, w.dY, T1 * N, m);
    SAT_TRY(launch_ok("scatter dA"));
    if (!fork) SAT_TRY(leaf_out_hidden());

    // ---- back through time
    static const int att_fused = getenv("SAT_ATT_FUSED") ? atoi(getenv("SAT_ATT_FUSED")) : 0;
    const bool use_b = w.Hb != nullptr && !att_fused;           // bf16 operand copies (the forward cast the weights into Wcat_b / Wz_b)
    const __bf16* annb = (w.annb && !att_fused && ann_bf16_enabled() && al16(b.ann)) ? w.annb : nullptr;      // the forward left the bf16 annotations there
    for (int t = ts - 1; t >= 0; --t) {
        const float* hc = w.HC + (long)t * N * HCW;
        float* dhc = w.DHC + (long)t * N * HCW;
        for (int l = top; l >= 1; --l) {        // stacked layers, top down: gate grads, then into the layer below and the own past
            float* dgu = DGUs(t, l);
            if (ln) {
                SAT_TRY(lstm_ln_cell_bwd(GUs(t, l), 4 * n, Cs(t, l), LnX(t, l), LnR(t, l), l == top ? w.dHout + (long)t * N * n : (const float*)nullptr, dHcs(l),
                                         dCcs(l), dgu, 4 * n, b.lengths, t, N, n, nullptr, ln_layer(p, l), LnP(l), st));
            } else {
                hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3(cdiv((long)N * n, 256)), dim3(256), 0, st, GUs(t, l), 4 * n, Cs(t, l), Cs(t + 1, l),
                                   l == top ? w.dHout + (long)t * N * n : (const float*)nullptr, dHcs(l), dCcs(l), dgu, 4 * n, b.lengths, t, N, n);
                SAT_TRY(launch_ok("lstm_cell_bwd (stacked layer)"));
            }
            SAT_TRY(gemm(st, A_ROW, B_KMAJOR, dgu, 4 * n, p.up_w_ih[l - 1], n, dHcs(l - 1), n, N, n, 4 * n, 1, EPI_NONE, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, slab, se));
            SAT_TRY(gemm(st, A_ROW, B_KMAJOR, dgu, 4 * n, up_w_hh[l - 1], n, dHcs(l), n, N, n, 4 * n, 1, EPI_NONE, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, slab, se));
        }
        if (ln) {
            SAT_TRY(lstm_ln_cell_bwd(hc + A + D, HCW, Cs(t, 0), LnX(t, 0), LnR(t, 0), top == 0 ? w.dHout + (long)t * N * n : (const float*)nullptr, dHcs(0), dCcs(0),
                                     dhc + A + D, HCW, b.lengths, t, N, n, use_b ? w.DHCb + A + D : (__bf16*)nullptr, ln_layer(p, 0), LnP(0), st));
        } else {
            hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3(cdiv((long)N * n, 256)), dim3(256), 0, st, hc + A + D, HCW, Cs(t, 0),
                               Cs(t + 1, 0), top == 0 ? w.dHout + (long)t * N * n : (const float*)nullptr, dHcs(0), dCcs(0), dhc + A + D, HCW, b.lengths, t, N, n,
                               use_b ? w.DHCb + A + D : (__bf16*)nullptr);
            SAT_TRY(launch_ok("lstm_cell_bwd"));
        }
        // d(beta*z) = dG * W_ih[:, m:]
        if (use_b) SAT_TRY(gemm_bb_nn(st, w.DHCb + A + D, HCW, w.Wz_b, D, w.dXZ, D, N, D, 4 * n, 0, slab, se));
        else SAT_TRY(gemm(st, A_ROW, B_KMAJOR, dhc + A + D, HCW, p.w_ih + m, m + D, w.dXZ, D, N, D, 4 * n, 0, EPI_NONE, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, slab, se));
        // the dev switch withholds the scratch: the single-launch form
        SAT_TRY(launch_attention_bwd(st, b.ann, w.U, hc, HCW, p.att_f, b.lengths, t, alphas, dalphas, T1, w.Z + (long)t * N * D, w.dZout + (long)t * N * D, w.dXZ,
                                     w.DZ + (long)t * N * D, dhc, HCW, w.dU, w.dwf_part, att_fused ? nullptr : w.DA, d.B, d.R, d.L, D, A,
                                     use_b ? w.DHCb : nullptr, annb));
        // dh_{t-1} += [dq | dbeta_pre | dG] * Wcat
        if (use_b) {
            SAT_TRY(gemm_bb_nn(st, w.DHCb, HCW, w.Wcat_b, n, w.dHc, n, N, n, HCW, 1, slab, se));
        } else if (NL == 1) {
            SAT_TRY(gemm(st, A_ROW, B_KMAJOR, dhc, HCW, w.Wcat, n, w.dHc, n, N, n, HCW, 1, EPI_NONE, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, slab, se));
        } else {
            SAT_TRY(gemm(st, A_ROW, B_KMAJOR, dhc, HCW, w.Wcat, n, dHcs(top), n, N, n, A + D, 1, EPI_NONE, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, slab, se));
            SAT_TRY(gemm(st, A_ROW, B_KMAJOR, dhc + A + D, HCW, w.Wcat + (long)(A + D) * n, n, dHcs(0), n, N, n, 4 * n, 1, EPI_NONE, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, slab, se));
        }
    }
    // now dHc = dL/dh0 and dCc = dL/dc0

    // ---- weight gradients, batched over every executed step (reduction length KR = ts*N)
    auto wgrad = [&](const float* dy, long ldy, const float* x, long ldx, float* out, long ldo, int M, int Nn) {
        return gemm(ls, A_KMAJOR, B_KMAJOR, dy, ldy, x, ldx, out, ldo, M, Nn, KR, 0, EPI_NONE, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, lslab, se);
    };
    const float* dG = w.DHC + A + D;
    // leaf: the parameters of the time loop, the embedding table, the attention parameters
    auto leaf_loop_params = [&]() -> int {
        SAT_TRY(wgrad(w.DHC, HCW, Hs(0, top), n, g.att_dec, n, A, n));
        SAT_TRY(wgrad(w.DHC + A, HCW, Hs(0, top), n, g.beta_w, n, D, n));
        SAT_TRY(wgrad(dG, HCW, Hs(0, 0), n, g.w_hh, n, 4 * n, n));
        for (int l = 1; l < NL; ++l) {
            const float* dgu = DGUs(0, l);
            SAT_TRY(wgrad(dgu, 4 * n, Hs(1, l - 1), n, g.up_w_ih[l - 1], n, 4 * n, n));
            SAT_TRY(wgrad(dgu, 4 * n, Hs(0, l), n, g.up_w_hh[l - 1], n, 4 * n, n));
            SAT_TRY(colsum(ls, wl, dgu, 4 * n, KR, 4 * n, g.up_b_ih[l - 1]));
            SAT_TRY(dev_copy_bytes(ls, g.up_b_hh[l - 1], g.up_b_ih[l - 1], (size_t)4 * n * 4));
        }
        if (d.weight_drop > 0.f) {      // the products above are gradients w.r.t. the MASKED matrices: times the same mask, all layers in one launch
            float* gw[SAT_MAX_LSTM_LAYERS] = {g.w_hh};
            for (int l = 1; l < NL; ++l) gw[l] = g.up_w_hh[l - 1];
            SAT_TRY(weight_drop(gw, gw, nullptr, NL, 4L * n * n, 0, d.weight_drop, (unsigned long long)d.dropout_seed, ls));
        }
        // layer-normalised cell: the sum over the slots of the time loop's partials, per layer (leaf work)
        for (int l = 0; ln && l < NL; ++l)
            SAT_TRY(ln_param_grads(LnP(l), w.ln_nslots, n, g.ln_gate_w[l], g.ln_gate_b[l], g.ln_cell_w[l], g.ln_cell_b[l], wl.colpart, ls));
        SAT_TRY(colsum(ls, wl, w.DHC + A, HCW, KR, D, g.beta_b));
        SAT_TRY(colsum(ls, wl, dG, HCW, KR, 4 * n, g.b_ih));
        SAT_TRY(dev_copy_bytes(ls, g.b_hh, g.b_ih, (size_t)4 * n * 4));
        SAT_TRY(wgrad(dG, HCW, w.Y, m, g.w_ih, m + D, 4 * n, m));
        SAT_TRY(wgrad(dG, HCW, w.XZ, D, g.w_ih + m, m + D, 4 * n, D));
        // embedding: dY = dA (deep output) + dG * W_ih[:, :m], scattered into the table (padding row skipped)
        SAT_TRY(gemm(ls, A_ROW, B_KMAJOR, dG, HCW, p.w_ih, m + D, w.dY, m, KR, m, 4 * n, 1));
        if (d.embedding_dropout > 0.f && KR > 0) {
            hipLaunchKernelGGL(dropout_rows_kernel, dim3(cdiv((long)KR * m, 256)), dim3(256), 0, ls, w.dY, w.dY, (long)KR * m, m, d.embedding_dropout,
                               (unsigned long long)d.dropout_seed, 1u, 0L, (const int*)nullptr, d.variational_dropout ? N : 0);
            SAT_TRY(launch_ok("embedding dropout bwd"));
        }
        if (KR > 0) {
            SAT_TRY(dev_fill_bytes(ls, w.emb_count, 0, (size_t)V * 4));
            hipLaunchKernelGGL(embedding_count_kernel, dim3(cdiv(KR, 256)), dim3(256), 0, ls, w.Tok, KR, V, d.padding_idx, w.emb_count);
            hipLaunchKernelGGL(embedding_scan_kernel, dim3(1), dim3(1024), 0, ls, w.emb_count, V, w.emb_offset, w.emb_cursor);
            hipLaunchKernelGGL(embedding_place_kernel, dim3(cdiv(KR, 256)), dim3(256), 0, ls, w.Tok, KR, V, d.padding_idx, w.emb_offset, w.emb_cursor, w.emb_list);
            hipLaunchKernelGGL(embedding_sum_kernel, dim3(V), dim3(256), 0, ls, w.dY, w.Tok, w.emb_offset, w.emb_list, g.embedding, KR, m, d.padding_idx);
            SAT_TRY(launch_ok("embedding gradient"));
        } else SAT_TRY(dev_fill_bytes(ls, g.embedding, 0, (size_t)V * m * 4));
        SAT_TRY(colsum(ls, wl, w.dwf_part, A, d.B, A, g.att_f));
        return gemm(ls, A_KMAJOR, B_KMAJOR, w.dU, A, b.ann, D, g.att_enc, D, A, D, d.B * d.L, 0, EPI_NONE, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, lslab, se);
    };
    // critical: the annotation gradient through att_enc and through the context
    auto crit_dann = [&]() -> int {
        SAT_TRY(gemm(st, A_ROW, B_KMAJOR, w.dU, A, p.att_enc, D, dann, D, d.B * d.L, D, A));
        return attention_context_bwd(alphas, w.DZ, b.lengths, dann, 1, d.B, d.R, T1, d.L, D, st);
    };
    // InitLSTM backward (the raw reshape is a reinterpretation: gradients of the repeated rows add up per image).  dropout > 0: the
    // per-caption-row path (see decoder_fwd); else one row per image.  dinit -> df -> dmean is critical, the four parameter gradients are leaf.
    const bool rows = d.dropout > 0.f;
    const int n2 = 2 * n * NL, IR = rows ? N : d.B;
    const float* dinit = rows ? w.init_rows : w.dinit_img;
    float* dfp = rows ? w.df_rows : w.df;
    auto crit_dinit = [&]() -> int {
        if (rows) {
            SAT_TRY(dev_copy_bytes(st, w.init_rows, w.dHc, (size_t)NL * N * n * 4));
            return dev_copy_bytes(st, w.init_rows + (long)NL * N * n, w.dCc, (size_t)NL * N * n * 4);
        }
        hipLaunchKernelGGL(init_expand_bwd_kernel, dim3(cdiv((long)d.B * n2, 256)), dim3(256), 0, st, w.dHc, w.dCc, w.dinit_img, d.B, d.R, n * NL);
        return launch_ok("init_expand_bwd");
    };
    auto leaf_init_i = [&]() -> int {
        SAT_TRY(gemm(ls, A_KMAJOR, B_KMAJOR, dinit, n2, rows ? w.f_rows : w.f, m, g.init_i_w, m, n2, m, IR));
        return colsum(ls, wl, dinit, n2, IR, n2, g.init_i_b);
    };
    auto crit_df = [&]() -> int { return gemm(st, A_ROW, B_KMAJOR, dinit, n2, p.init_i_w, m, dfp, m, IR, m, n2); };
    auto leaf_init_f = [&]() -> int {
        SAT_TRY(gemm(ls, A_KMAJOR, B_KMAJOR, dfp, m, rows ? w.mean_rows : w.mean, D, g.init_f_w, D, m, D, IR));
        return colsum(ls, wl, dfp, m, IR, m, g.init_f_b);
    };
    auto crit_dmean = [&]() -> int {
        if (rows) {
            SAT_TRY(gemm(st, A_ROW, B_KMAJOR, w.df_rows, m, p.init_f_w, D, w.dmean_rows, D, N, D, m));          // d(mean rows)
            hipLaunchKernelGGL(init_mean_rows_bwd_kernel, dim3(cdiv((long)d.B * D, 256)), dim3(256), 0, st, w.dmean_rows, w.dmean, d.B, d.R, D, d.dropout,
                               (unsigned long long)d.dropout_seed);
            SAT_TRY(launch_ok("init_mean_rows_bwd"));
        } else {
            SAT_TRY(gemm(st, A_ROW, B_KMAJOR, w.df, m, p.init_f_w, D, w.dmean, D, d.B, D, m));
        }
        const long tot = (long)d.B * d.L * D;
        hipLaunchKernelGGL(dann_add_mean_kernel, dim3(cdiv(tot, 256)), dim3(256), 0, st, dann, w.dmean, d.L, D, tot);
        return launch_ok("dann_add_mean");
    };
    if (!fork) {          // one stream: the two parts interleaved, each launch where it has always been
        SAT_TRY(leaf_loop_params());
        SAT_TRY(crit_dann());
        SAT_TRY(crit_dinit());
        SAT_TRY(leaf_init_i());
        SAT_TRY(crit_df());
        SAT_TRY(leaf_init_f());
        return crit_dmean();
    }
    SAT_TRY(crit_dann());
    SAT_TRY(crit_dinit());
    SAT_TRY(crit_df());
    SAT_CHECK_HIP(hipEventRecord(fork_event, st));              // df is the last thing the leaf part reads that st writes
    SAT_TRY(crit_dmean());
    SAT_CHECK_HIP(hipStreamWaitEvent(side, fork_event, 0));
    SAT_TRY(leaf_out_w());
    SAT_TRY(leaf_out_hidden());
    SAT_TRY(leaf_loop_params());
    SAT_TRY(leaf_init_i());
    return leaf_init_f();
}


int colsum_public(const float* x, long ld, long rows, int cols, float* out, float* scratch, hipStream_t st) {
    Ws w; w.colpart = scratch;
    return colsum(st, w, x, ld, (int)rows, cols, out);
}

size_t decoder_workspace_bytes(const sat_decoder_dims& d, bool ln) { return layout(d, nullptr, ln).total; }
int ln_param_grads(const float* part, int slots, int n, float* dgate_w, float* dgate_b, float* dcell_w, float* dcell_b, float* scratch, hipStream_t st) {
    Ws w; w.colpart = scratch;
    SAT_TRY(colsum(st, w, part, 10L * n, slots, 4 * n, dgate_w));
    SAT_TRY(colsum(st, w, part + 4L * n, 10L * n, slots, 4 * n, dgate_b));
    SAT_TRY(colsum(st, w, part + 8L * n, 10L * n, slots, n, dcell_w));
    return colsum(st, w, part + 9L * n, 10L * n, slots, n, dcell_b);
}


// ------------------------------------------------------------------ sub-module step entry points (SURVEY 8b minimum set)
// The reference's sub-modules called on their own (model.py:76-81, 94-109, 125-131, 175-180 / 326, 544): the same kernels and GEMMs
// as the train loop above, for N independent rows, exact fp32 MFMA.  Scratch comes from the caller (sizes in include/sat_hip.h).
static int fill_f(hipStream_t st, float* p, long n, float v) {
    if (n <= 0) return SAT_OK;
    hipLaunchKernelGGL(fill_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, p, n, v);
    return launch_ok("fill");
}

int attention_context_bwd(const float* alphas, const float* DZ, const int* lengths, float* dann, int accumulate, int B, int R, int T1, int L, int D, hipStream_t st) {
    AttPlan pl;
    SAT_TRY(attention_plan(ATT_OP_CONTEXT_BWD, R, L, D, 0, 0, T1, 0u, pl, "attention_context_bwd"));
    const size_t lds = pl.lds0;
    if (pl.nq == 13) {
        SAT_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(dann_from_context_kernel<13>), lds));
        hipLaunchKernelGGL(dann_from_context_kernel<13>, dim3(B, cdiv(D, 256)), dim3(256), lds, st, alphas, DZ, lengths, dann, accumulate, R, B * R, T1, L, D);
    } else {
        SAT_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(dann_from_context_kernel<16>), lds));
        hipLaunchKernelGGL(dann_from_context_kernel<16>, dim3(B, cdiv(D, 256)), dim3(256), lds, st, alphas, DZ, lengths, dann, accumulate, R, B * R, T1, L, D);
    }
    return launch_ok("dann_from_context");
}

// nn.LSTM, one layer, one time step (model.py:175-180; calls at 326, 544): gates = x W_ih^T + b_ih + h W_hh^T + b_hh, i,f,g,o
int lstm_cell_fwd(const float* x, int in, const float* h_prev, const float* c_prev, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                  float* gates, float* h_new, float* c_new, float* bias_scratch, int N, int n, hipStream_t st) {
    t_bf16_mfma = 0;
    hipLaunchKernelGGL(add_kernel, dim3(cdiv(4 * n, 256)), dim3(256), 0, st, bias_scratch, b_ih, b_hh, (long)4 * n);
    SAT_TRY(launch_ok("bias add"));
    SAT_TRY(gemm(st, A_ROW, B_ROW, x, in, w_ih, in, gates, 4 * n, N, 4 * n, in, 0, EPI_BIAS, bias_scratch));
    SAT_TRY(gemm(st, A_ROW, B_ROW, h_prev, n, w_hh, n, gates, 4 * n, N, 4 * n, n, 1));
    return lstm_cell_pointwise(gates, 4 * n, c_prev, h_prev, c_new, h_new, nullptr, N, n, st);
}

int lstm_cell_bwd(const float* x, int in, const float* h_prev, const float* c_prev, const float* c_new, const float* gates, const float* dh_new, const float* dc_new,
                  const float* w_ih, const float* w_hh, float* dx, float* dh_prev, float* dc_prev, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh,
                  float* dgates, float* scratch, int N, int n, hipStream_t st) {
    t_bf16_mfma = 0;
    // the cell kernel adds its `carry` inputs and leaves dc_prev in the cell carry: start them from the incoming cell gradient / zero
    if (dc_new) SAT_TRY(dev_copy_bytes(st, dc_prev, dc_new, (size_t)N * n * 4));
    else SAT_TRY(fill_f(st, dc_prev, (long)N * n, 0.f));
    SAT_TRY(fill_f(st, dh_prev, (long)N * n, 0.f));
    hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3(cdiv((long)N * n, 256)), dim3(256), 0, st, gates, 4 * n, c_prev, c_new, dh_new, dh_prev, dc_prev, dgates, 4 * n,
                       (const int*)nullptr, 0, N, n, (__bf16*)nullptr);
    SAT_TRY(launch_ok("lstm_cell_bwd"));
    SAT_TRY(gemm(st, A_ROW, B_KMAJOR, dgates, 4 * n, w_ih, in, dx, in, N, in, 4 * n));
    SAT_TRY(gemm(st, A_ROW, B_KMAJOR, dgates, 4 * n, w_hh, n, dh_prev, n, N, n, 4 * n));
    SAT_TRY(gemm(st, A_KMAJOR, B_KMAJOR, dgates, 4 * n, x, in, dw_ih, in, 4 * n, in, N));
    SAT_TRY(gemm(st, A_KMAJOR, B_KMAJOR, dgates, 4 * n, h_prev, n, dw_hh, n, 4 * n, n, N));
    Ws w; w.colpart = scratch;
    SAT_TRY(colsum(st, w, dgates, 4 * n, N, 4 * n, db_ih));
    SAT_TRY(dev_copy_bytes(st, db_hh, db_ih, (size_t)4 * n * 4));
    return SAT_OK;
}

// DeepOutput.forward (model.py:125-131)
int deep_output_fwd(const float* prev_embed, const float* hidden, const float* context, const float* w_hidden, const float* w_context, const float* w_out,
                    const float* b_out, float dropout, unsigned long long seed, float* u, float* udrop, float* logits, int N, int m, int n, int D, int V, hipStream_t st) {
    t_bf16_mfma = 0;
    if (context) {
        SAT_TRY(gemm(st, A_ROW, B_ROW, hidden, n, w_hidden, n, u, m, N, m, n));
        SAT_TRY(gemm(st, A_ROW, B_ROW, context, D, w_context, D, u, m, N, m, D, 1, EPI_ADD_TANH, nullptr, nullptr, nullptr, prev_embed, m));
    } else {
        SAT_TRY(gemm(st, A_ROW, B_ROW, hidden, n, w_hidden, n, u, m, N, m, n));
    }
    const float* uin = u;
    if (dropout > 0.f) {
        hipLaunchKernelGGL(dropout_rows_kernel, dim3(cdiv((long)N * m, 256)), dim3(256), 0, st, u, udrop, (long)N * m, m, dropout, seed, 2u, 0L, (const int*)nullptr, 0);
        SAT_TRY(launch_ok("output dropout"));
        uin = udrop;
    }
    return gemm(st, A_ROW, B_ROW, uin, m, w_out, m, logits, V, N, V, m, 0, b_out ? EPI_BIAS : EPI_NONE, b_out);
}

int deep_output_bwd(const float* dlogits, const float* hidden, const float* context, const float* u, const float* udrop, const float* w_hidden, const float* w_context,
                    const float* w_out, float dropout, unsigned long long seed, float* d_prev_embed, float* d_hidden, float* d_context, float* dw_hidden,
                    float* dw_context, float* dw_out, float* db_out, float* scratch, int N, int m, int n, int D, int V, hipStream_t st) {
    t_bf16_mfma = 0;
    const bool deep = context != nullptr;
    float* du = d_prev_embed;                 // gradient of the pre-tanh sum = gradient of the embedding input (deep); scratch of the same shape (shallow)
    if (dropout > 0.f) {
        SAT_TRY(gemm(st, A_ROW, B_KMAJOR, dlogits, V, w_out, m, du, m, N, m, V));
        hipLaunchKernelGGL(dropout_rows_kernel, dim3(cdiv((long)N * m, 256)), dim3(256), 0, st, du, du, (long)N * m, m, dropout, seed, 2u, 0L, (const int*)nullptr, 0);
        SAT_TRY(launch_ok("output dropout bwd"));
        if (deep) {
            hipLaunchKernelGGL(mul_dtanh_kernel, dim3(cdiv((long)N * m, 256)), dim3(256), 0, st, du, u, (long)N * m);
            SAT_TRY(launch_ok("tanh bwd"));
        }
    } else {
        SAT_TRY(gemm(st, A_ROW, B_KMAJOR, dlogits, V, w_out, m, du, m, N, m, V, 0, deep ? EPI_MUL_DTANH : EPI_NONE, nullptr, nullptr, nullptr, u, m));
    }
    SAT_TRY(gemm(st, A_KMAJOR, B_KMAJOR, dlogits, V, dropout > 0.f ? udrop : u, m, dw_out, m, V, m, N));
    Ws w; w.colpart = scratch;
    if (db_out) SAT_TRY(colsum(st, w, dlogits, V, N, V, db_out));
    SAT_TRY(gemm(st, A_ROW, B_KMAJOR, du, m, w_hidden, n, d_hidden, n, N, n, m));
    SAT_TRY(gemm(st, A_KMAJOR, B_KMAJOR, du, m, hidden, n, dw_hidden, n, m, n, N));
    if (deep) {
        SAT_TRY(gemm(st, A_ROW, B_KMAJOR, du, m, w_context, D, d_context, D, N, D, m));
        SAT_TRY(gemm(st, A_KMAJOR, B_KMAJOR, du, m, context, D, dw_context, D, m, D, N));
    }
    return SAT_OK;
}

// InitLSTM.forward (model.py:76-81) on N rows; `init` (N, n2) row-major IS the (2*layers, N, n) buffer of the raw reshape (F3)
int init_lstm_fwd(const float* ann, const float* w_f, const float* b_f, const float* w_i, const float* b_i, float dropout, unsigned long long seed, float* mean,
                  float* f, float* init, int N, int L, int D, int m, int n2, hipStream_t st) {
    t_bf16_mfma = 0;
    hipLaunchKernelGGL(ann_mean_kernel, dim3(N), dim3(256), 0, st, ann, mean, L, D);
    SAT_TRY(launch_ok("ann_mean"));
    if (dropout > 0.f) {
        hipLaunchKernelGGL(init_mean_rows_kernel, dim3(cdiv((long)N * D, 256)), dim3(256), 0, st, mean, mean, N, 1, D, dropout, seed);
        SAT_TRY(launch_ok("init_mean_rows"));
    }
    SAT_TRY(gemm(st, A_ROW, B_ROW, mean, D, w_f, D, f, m, N, m, D, 0, EPI_BIAS, b_f));
    return gemm(st, A_ROW, B_ROW, f, m, w_i, m, init, n2, N, n2, m, 0, EPI_BIAS, b_i);
}

int init_lstm_bwd(const float* dinit, const float* mean, const float* f, const float* w_f, const float* w_i, float dropout, unsigned long long seed, float* dw_f,
                  float* db_f, float* dw_i, float* db_i, float* dann, float* df, float* dmean, float* scratch, int N, int L, int D, int m, int n2, hipStream_t st) {
    t_bf16_mfma = 0;
    Ws w; w.colpart = scratch;
    SAT_TRY(gemm(st, A_KMAJOR, B_KMAJOR, dinit, n2, f, m, dw_i, m, n2, m, N));
    SAT_TRY(colsum(st, w, dinit, n2, N, n2, db_i));
    SAT_TRY(gemm(st, A_ROW, B_KMAJOR, dinit, n2, w_i, m, df, m, N, m, n2));
    SAT_TRY(gemm(st, A_KMAJOR, B_KMAJOR, df, m, mean, D, dw_f, D, m, D, N));
    SAT_TRY(colsum(st, w, df, m, N, m, db_f));
    SAT_TRY(gemm(st, A_ROW, B_KMAJOR, df, m, w_f, D, dmean, D, N, D, m));
    if (dropout > 0.f) {
        hipLaunchKernelGGL(init_mean_rows_bwd_kernel, dim3(cdiv((long)N * D, 256)), dim3(256), 0, st, dmean, dmean, N, 1, D, dropout, seed);
        SAT_TRY(launch_ok("init_mean_rows_bwd"));
    }
    const long tot = (long)N * L * D;
    SAT_TRY(fill_f(st, dann, tot, 0.f));
    hipLaunchKernelGGL(dann_add_mean_kernel, dim3(cdiv(tot, 256)), dim3(256), 0, st, dann, dmean, L, D, tot);
    return launch_ok("dann_add_mean");
}

// nn.Embedding forward (model.py:158-164, use at 298, 526): optional in-place max-norm renormalisation of the rows used, then the gather
int embedding_fwd(float* table, const int* tokens, float* out, int rows, int V, int m, float max_norm, int* flags, hipStream_t st) {
    if (max_norm > 0.f) {
        SAT_TRY(dev_fill_bytes(st, flags, 0, (size_t)V * 4));
        hipLaunchKernelGGL(embedding_mark_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, st, tokens, rows, flags, V);
        SAT_TRY(launch_ok("embedding_mark"));
        hipLaunchKernelGGL(embedding_renorm_kernel, dim3(V), dim3(64), 0, st, table, flags, m, max_norm);
        SAT_TRY(launch_ok("embedding_renorm"));
    }
    hipLaunchKernelGGL(gather_rows_kernel, dim3(rows), dim3(64), 0, st, table, tokens, out, rows, m, V, 0.f, 0ull, 0L, 0);
    return launch_ok("embedding gather");
}
// its gradient: rows of dY added into the table rows of their tokens in increasing row order (no floating-point atomics); padding row zero
int embedding_bwd(const float* dY, const int* tokens, float* dtable, int rows, int V, int m, int padding_idx, int* scratch, hipStream_t st) {
    int* count = scratch; int* offset = count + V; int* cursor = offset + V + 1; int* list = cursor + V;
    SAT_TRY(dev_fill_bytes(st, count, 0, (size_t)V * 4));
    hipLaunchKernelGGL(embedding_count_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, st, tokens, rows, V, padding_idx, count);
    hipLaunchKernelGGL(embedding_scan_kernel, dim3(1), dim3(1024), 0, st, count, V, offset, cursor);
    hipLaunchKernelGGL(embedding_place_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, st, tokens, rows, V, padding_idx, offset, cursor, list);
    hipLaunchKernelGGL(embedding_sum_kernel, dim3(V), dim3(256), 0, st, dY, tokens, offset, list, dtable, rows, m, padding_idx);
    return launch_ok("embedding gradient");
}
// backward of y = sigmoid(pre): dpre = dy * y * (1 - y)   (the beta gate, model.py:187-192)
int sigmoid_bwd(const float* dy, const float* y, float* dpre, long n, hipStream_t st) {
    hipLaunchKernelGGL(sigmoid_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, dy, y, dpre, n);
    return launch_ok("sigmoid_bwd");
}

}  // namespace sat
