// extern "C" surface of libsat_hip.so (declared in include/sat_hip.h).
#include <stdarg.h>

#include "../../include/sat_hip.h"
#include "decoder.h"
#include "decoder_step.h"
#include "gemm.h"
#include "gemm_bf16_common.h"
#include "temperature.h"
#include "caption_score.h"

namespace sat {
static thread_local char g_err[512] = {0};
int& dev_switch(int which) {
    static int v[SW_COUNT] = {0 /* (ticket-based BatchNorm reduce: removed in round 3, measured slower) */, getenv("SAT_NO_WGRAD3X3") ? !atoi(getenv("SAT_NO_WGRAD3X3")) : 1,
                              getenv("SAT_REDUCE_Z16") ? atoi(getenv("SAT_REDUCE_Z16")) : 1, getenv("SAT_WIDE_TILES") ? atoi(getenv("SAT_WIDE_TILES")) : 0,
                              getenv("SAT_BN_ONEPASS") ? atoi(getenv("SAT_BN_ONEPASS")) : 1,
                              getenv("SAT_BN_VPT") ? atoi(getenv("SAT_BN_VPT")) : 2,
                              getenv("SAT_ACC_PREFETCH") ? atoi(getenv("SAT_ACC_PREFETCH")) : 0};
    return v[which];
}
int& trace_launches() { static int on = getenv("SAT_TRACE_LAUNCH") ? 1 : 0; return on; }
char* last_error_buf() { return g_err; }
int fail(int code, const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
    return code;
}
}  // namespace sat

using namespace sat;

extern "C" {

int sat_abi_version(void) { return SAT_HIP_ABI_VERSION; }
int sat_debug_trace_launches(int32_t on) { sat::trace_launches() = on ? 1 : 0; return SAT_OK; }
int sat_debug_option(const char* name, int32_t value) {
    if (!name) return fail(SAT_EINVAL, "debug_option: null name");
    if (!strcmp(name, "wgrad3x3")) { dev_switch(SW_WGRAD3X3) = value; return SAT_OK; }
    if (!strcmp(name, "reduce_z16")) { dev_switch(SW_REDUCE_Z16) = value; return SAT_OK; }
    if (!strcmp(name, "acc_prefetch")) { dev_switch(SW_ACC_PREFETCH) = value; return SAT_OK; }
    if (!strcmp(name, "bn_vpt")) { dev_switch(SW_BN_VPT) = value; return SAT_OK; }
    if (!strcmp(name, "bn_onepass")) { dev_switch(SW_BN_ONEPASS) = value; return SAT_OK; }
    if (!strcmp(name, "wide_tiles")) { dev_switch(SW_WIDE_TILES) = value; return SAT_OK; }
    if (!strcmp(name, "glds_tile")) { glds_force_tile() = value; return SAT_OK; }
    if (!strcmp(name, "glds_stages")) { glds_force_stages() = value; return SAT_OK; }
    if (!strcmp(name, "glds_stages_tr_bf16")) { glds_stages_tr_bf16() = value; return SAT_OK; }
    if (!strcmp(name, "glds_stages_f32")) { glds_stages_f32() = value; return SAT_OK; }
    if (!strcmp(name, "w3_stages")) { w3_stages() = value; return SAT_OK; }
    if (!strcmp(name, "glds_stages8")) { glds_stages8() = value; return SAT_OK; }
    if (!strcmp(name, "glds_tall_k")) { glds_tall_k() = value; return SAT_OK; }
    if (!strcmp(name, "glds_tall_conv")) { glds_tall_conv() = value; return SAT_OK; }
    if (!strcmp(name, "tile_override")) { gemm_tile_override() = value; return SAT_OK; }
    return fail(SAT_EINVAL, "debug_option: unknown option %s", name);
}
const char* sat_last_error(void) { return last_error_buf(); }

static int gemm_from_desc(const sat_gemm_desc* d, const sat_gemm_types* t, void* stream);
int sat_gemm_f32(const sat_gemm_desc* d, void* stream) { return gemm_from_desc(d, nullptr, stream); }
int sat_gemm_ex(const sat_gemm_desc* d, const sat_gemm_types* t, void* stream) {
    if (!t) return fail(SAT_EINVAL, "sat_gemm_ex: null type descriptor");
    return gemm_from_desc(d, t, stream);
}
static int gemm_from_desc(const sat_gemm_desc* d, const sat_gemm_types* t, void* stream) {
    if (!d) return fail(SAT_EINVAL, "sat_gemm_f32: null descriptor");
    if (d->amode != A_ROW && d->amode != A_KMAJOR) return fail(SAT_EINVAL, "sat_gemm_f32: amode %d (dense modes only)", d->amode);
    if (d->bmode != B_ROW && d->bmode != B_KMAJOR) return fail(SAT_EINVAL, "sat_gemm_f32: bmode %d (dense modes only)", d->bmode);
    GemmArgs g;
    g.A = d->A; g.lda = d->lda; g.a_rows = d->a_rows; g.B = d->B; g.ldb = d->ldb; g.C = d->C; g.ldc = d->ldc; g.c_rows = d->c_rows;
    g.M = d->M; g.N = d->N; g.K = d->K; g.amode = d->amode; g.bmode = d->bmode; g.accumulate = d->accumulate; g.epi = d->epi;
    g.bias = d->bias; g.e0 = d->e0; g.lde0 = d->lde0; g.c0 = d->c0; g.c1 = d->c1; g.slab = d->slab; g.slab_elems = d->slab_elems;
    if (t) { g.a_bf16 = t->a_bf16; g.b_bf16 = t->b_bf16; g.c_bf16 = t->c_bf16; g.bf16_mfma = t->bf16_mfma; }
    return launch_gemm(g, (hipStream_t)stream);
}

size_t sat_decoder_workspace_bytes(const sat_decoder_dims* d) {
    if (check_dims(d) != SAT_OK) return 0;
    return decoder_workspace_bytes(*d);
}

size_t sat_decoder_workspace_bytes_ln(const sat_decoder_dims* d, const sat_decoder_params* w) {
    if (check_dims(d) != SAT_OK) return 0;
    return decoder_workspace_bytes(*d, w && ln_on(*w));
}

static int check_params(const sat_decoder_dims* d, const sat_decoder_params* w, const char* what) {
    if (!w) return fail(SAT_EINVAL, "%s: null parameter struct", what);
    if (!w->embedding || !w->init_f_w || !w->init_f_b || !w->init_i_w || !w->init_i_b || !w->w_ih || !w->w_hh || !w->b_ih || !w->b_hh ||
        !w->att_enc || !w->att_dec || !w->att_f || !w->beta_w || !w->beta_b || !w->out_hidden || !w->out_w)
        return fail(SAT_EINVAL, "%s: null tensor in parameter struct", what);
    if (d->deep_output && !w->out_context) return fail(SAT_EINVAL, "%s: deep output needs output.context.weight", what);
    for (int l = 1; l < d->layers; ++l)
        if (!w->up_w_ih[l - 1] || !w->up_w_hh[l - 1] || !w->up_b_ih[l - 1] || !w->up_b_hh[l - 1])
            return fail(SAT_EINVAL, "%s: null tensor for LSTM layer %d", what, l);
    // the layer-norm tensors are the switch of the normalised cell: all of them for the layers in use, or none
    int ln_set = 0;
    for (int l = 0; l < d->layers; ++l) ln_set += (w->ln_gate_w[l] != nullptr) + (w->ln_gate_b[l] != nullptr) + (w->ln_cell_w[l] != nullptr) + (w->ln_cell_b[l] != nullptr);
    if (ln_set != 0 && ln_set != 4 * d->layers)
        return fail(SAT_EINVAL, "%s: %d of the %d layer-norm tensors (ln_gate_w / ln_gate_b / ln_cell_w / ln_cell_b of %d layers) are set: all or none", what, ln_set,
                    4 * d->layers, d->layers);
    return SAT_OK;
}
static int check_batch(const sat_decoder_batch* b) {
    if (!b || !b->ann || !b->caps || !b->lengths || !b->prow || !b->src_row || !b->step_offsets_host || !b->teacher_host)
        return fail(SAT_EINVAL, "decoder: null field in batch struct");
    return SAT_OK;
}

int sat_decoder_train_fwd(const sat_decoder_dims* d, const sat_decoder_params* w, const sat_decoder_batch* b, float* logits_packed,
                          float* alphas, void* workspace, size_t workspace_bytes, void* stream) {
    SAT_TRY(check_dims(d)); SAT_TRY(check_params(d, w, "decoder_train_fwd")); SAT_TRY(check_batch(b));
    if (!alphas || !workspace || (d->P > 0 && !logits_packed)) return fail(SAT_EINVAL, "decoder_train_fwd: null output/workspace");
    return decoder_fwd(*d, *w, *b, logits_packed, alphas, (char*)workspace, workspace_bytes, (hipStream_t)stream);
}

int sat_decoder_train_bwd(const sat_decoder_dims* d, const sat_decoder_params* w, const sat_decoder_batch* b, const float* dlogits_packed,
                          const float* alphas, const float* dalphas, const sat_decoder_params* g, float* dann, void* workspace,
                          size_t workspace_bytes, void* stream) {
    SAT_TRY(check_dims(d)); SAT_TRY(check_params(d, w, "decoder_train_bwd")); SAT_TRY(check_params(d, g, "decoder_train_bwd(grads)")); SAT_TRY(check_batch(b));
    if (!alphas || !dann || !workspace || (d->P > 0 && !dlogits_packed)) return fail(SAT_EINVAL, "decoder_train_bwd: null input/output/workspace");
    return decoder_bwd(*d, *w, *b, dlogits_packed, alphas, dalphas, *g, dann, (char*)workspace, workspace_bytes, (hipStream_t)stream);
}

int sat_decoder_train_bwd_fork(const sat_decoder_dims* d, const sat_decoder_params* w, const sat_decoder_batch* b, const float* dlogits_packed,
                               const float* alphas, const float* dalphas, const sat_decoder_params* g, float* dann, void* workspace,
                               size_t workspace_bytes, void* side_stream, void* event, void* stream) {
    SAT_TRY(check_dims(d)); SAT_TRY(check_params(d, w, "decoder_train_bwd_fork")); SAT_TRY(check_params(d, g, "decoder_train_bwd_fork(grads)")); SAT_TRY(check_batch(b));
    if (!alphas || !dann || !workspace || (d->P > 0 && !dlogits_packed)) return fail(SAT_EINVAL, "decoder_train_bwd_fork: null input/output/workspace");
    if ((side_stream != nullptr) != (event != nullptr)) return fail(SAT_EINVAL, "decoder_train_bwd_fork: side stream and event go together (got %s only)", side_stream ? "a stream" : "an event");
    if (side_stream && side_stream == stream) return fail(SAT_EINVAL, "decoder_train_bwd_fork: the side stream is the caller's stream");
    if (workspace_bytes < decoder_workspace_bytes(*d))
        return fail(SAT_EINVAL, "decoder_train_bwd_fork: workspace %zu < %zu bytes", workspace_bytes, decoder_workspace_bytes(*d));
    return decoder_bwd(*d, *w, *b, dlogits_packed, alphas, dalphas, *g, dann, (char*)workspace, workspace_bytes, (hipStream_t)stream, (hipStream_t)side_stream,
                       (hipEvent_t)event);
}

int sat_decoder_train_bwd_reg(const sat_decoder_dims* d, const sat_decoder_params* w, const sat_decoder_batch* b, const float* dlogits_packed,
                              const float* alphas, const float* dalphas, const sat_decoder_params* g, float* dann, void* workspace,
                              size_t workspace_bytes, void* side_stream, void* event, void* stream, const float* reg_gscale) {
    if (!reg_gscale)
        return sat_decoder_train_bwd_fork(d, w, b, dlogits_packed, alphas, dalphas, g, dann, workspace, workspace_bytes, side_stream, event, stream);
    SAT_TRY(check_dims(d)); SAT_TRY(check_params(d, w, "decoder_train_bwd_reg")); SAT_TRY(check_params(d, g, "decoder_train_bwd_reg(grads)")); SAT_TRY(check_batch(b));
    if (!alphas || !dann || !workspace || (d->P > 0 && !dlogits_packed)) return fail(SAT_EINVAL, "decoder_train_bwd_reg: null input/output/workspace");
    if ((side_stream != nullptr) != (event != nullptr)) return fail(SAT_EINVAL, "decoder_train_bwd_reg: side stream and event go together (got %s only)", side_stream ? "a stream" : "an event");
    if (side_stream && side_stream == stream) return fail(SAT_EINVAL, "decoder_train_bwd_reg: the side stream is the caller's stream");
    if (workspace_bytes < decoder_workspace_bytes(*d))
        return fail(SAT_EINVAL, "decoder_train_bwd_reg: workspace %zu < %zu bytes", workspace_bytes, decoder_workspace_bytes(*d));
    return decoder_bwd(*d, *w, *b, dlogits_packed, alphas, dalphas, *g, dann, (char*)workspace, workspace_bytes, (hipStream_t)stream, (hipStream_t)side_stream,
                       (hipEvent_t)event, reg_gscale);
}

int sat_decoder_train_reg_fwd(const sat_decoder_dims* d, const sat_decoder_batch* b, void* workspace, size_t workspace_bytes, void* scratch, float* out,
                              void* stream) {
    SAT_TRY(check_dims(d)); SAT_TRY(check_batch(b));
    if (!workspace || !scratch || !out) return fail(SAT_EINVAL, "decoder_train_reg_fwd: null workspace/scratch/out");
    if (workspace_bytes < decoder_workspace_bytes(*d))
        return fail(SAT_EINVAL, "decoder_train_reg_fwd: workspace %zu < %zu bytes", workspace_bytes, decoder_workspace_bytes(*d));
    return decoder_reg_fwd(*d, *b, (char*)workspace, workspace_bytes, scratch, out, (hipStream_t)stream);
}

static int weight_drop_public(const char* what, const float* src, float* dst, void* dstb, int32_t layers, int32_t rows, int32_t cols, float p, uint64_t seed,
                              void* stream) {
    if (!src || !dst) return fail(SAT_EINVAL, "%s: null pointer", what);
    if (layers < 1 || layers > SAT_MAX_LSTM_LAYERS || rows <= 0 || cols <= 0)
        return fail(SAT_EINVAL, "%s: layers=%d (1..%d) rows=%d cols=%d", what, layers, SAT_MAX_LSTM_LAYERS, rows, cols);
    if (!(p >= 0.f && p < 1.f)) return fail(SAT_EINVAL, "%s: p=%g must lie in [0,1)", what, (double)p);
    const long per = (long)rows * cols;
    const float* s[SAT_MAX_LSTM_LAYERS] = {}; float* o[SAT_MAX_LSTM_LAYERS] = {}; __bf16* ob[SAT_MAX_LSTM_LAYERS] = {};
    for (int l = 0; l < layers; ++l) { s[l] = src + l * per; o[l] = dst + l * per; ob[l] = dstb ? (__bf16*)dstb + l * per : nullptr; }
    return weight_drop(s, o, ob, layers, per, 0, p, (unsigned long long)seed, (hipStream_t)stream);
}
int sat_weight_drop(const float* w, float* out_f32, void* out_bf16, int32_t layers, int32_t rows, int32_t cols, float p, uint64_t seed, void* stream) {
    return weight_drop_public("weight_drop", w, out_f32, out_bf16, layers, rows, cols, p, seed, stream);
}
int sat_weight_drop_grad(float* g, int32_t layers, int32_t rows, int32_t cols, float p, uint64_t seed, void* stream) {
    return weight_drop_public("weight_drop_grad", g, g, nullptr, layers, rows, cols, p, seed, stream);
}

int sat_lstm_cell_pointwise_fwd(float* gates, int32_t g_ld, const float* gy, const float* c_prev, const float* h_prev, float* c_new, float* h_new,
                                const int32_t* live, void* h_bf16, int32_t rows, int32_t n, void* stream) {
    if (!gates || !c_prev || !h_prev || !c_new || !h_new) return fail(SAT_EINVAL, "lstm_cell_pointwise_fwd: null pointer");
    if (rows < 1 || n < 1 || g_ld < 4 * (int64_t)n) return fail(SAT_EINVAL, "lstm_cell_pointwise_fwd: bad shape (rows=%d n=%d g_ld=%d)", rows, n, g_ld);
    return lstm_cell_plain_fwd(gates, g_ld, gy, c_prev, h_prev, c_new, h_new, live, 0, rows, n, h_bf16, (hipStream_t)stream);
}
int sat_lstm_cell_pointwise_bwd(const float* gates, int32_t g_ld, const float* c_prev, const float* c_new, const float* dh_out, float* dh_carry, float* dc_carry,
                                float* dgates, int32_t dg_ld, const int32_t* live, void* dgates_bf16, int32_t rows, int32_t n, void* stream) {
    if (!gates || !c_prev || !c_new || !dh_carry || !dc_carry || !dgates) return fail(SAT_EINVAL, "lstm_cell_pointwise_bwd: null pointer");
    if (rows < 1 || n < 1 || g_ld < 4 * (int64_t)n || dg_ld < 4 * (int64_t)n)
        return fail(SAT_EINVAL, "lstm_cell_pointwise_bwd: bad shape (rows=%d n=%d g_ld=%d dg_ld=%d)", rows, n, g_ld, dg_ld);
    return lstm_cell_plain_bwd(gates, g_ld, c_prev, c_new, dh_out, dh_carry, dc_carry, dgates, dg_ld, live, 0, rows, n, dgates_bf16, (hipStream_t)stream);
}
int32_t sat_lstm_ln_slots(int32_t rows) { return ln_slots(rows); }
int sat_lstm_ln_cell_fwd(float* gates, int32_t g_ld, const float* gy, const float* c_prev, const float* h_prev, float* c_new, float* h_new, const int32_t* live,
                         void* h_bf16, const float* ln_gate_w, const float* ln_gate_b, const float* ln_cell_w, const float* ln_cell_b, float* xhat, float* rstd,
                         int32_t rows, int32_t n, void* stream) {
    if (!gates || !c_prev || !h_prev || !c_new || !h_new || !ln_gate_w || !ln_gate_b || !ln_cell_w || !ln_cell_b) return fail(SAT_EINVAL, "lstm_ln_cell_fwd: null pointer");
    if ((xhat != nullptr) != (rstd != nullptr)) return fail(SAT_EINVAL, "lstm_ln_cell_fwd: xhat and rstd go together");
    if (rows < 1 || n < 1 || g_ld < 4 * (int64_t)n) return fail(SAT_EINVAL, "lstm_ln_cell_fwd: bad shape (rows=%d n=%d g_ld=%d)", rows, n, g_ld);
    const LnCell ln{ln_gate_w, ln_gate_b, ln_cell_w, ln_cell_b};
    return lstm_ln_cell_fwd(gates, g_ld, gy, c_prev, h_prev, c_new, h_new, live, 0, rows, n, h_bf16, ln, xhat, rstd, (hipStream_t)stream);
}
int sat_lstm_ln_cell_bwd(const float* gates, int32_t g_ld, const float* c_prev, const float* xhat, const float* rstd, const float* dh_out, float* dh_carry,
                         float* dc_carry, float* dgates, int32_t dg_ld, const int32_t* live, void* dgates_bf16, const float* ln_gate_w, const float* ln_cell_w,
                         const float* ln_cell_b, float* part, int32_t rows, int32_t n, void* stream) {
    if (!gates || !c_prev || !xhat || !rstd || !dh_carry || !dc_carry || !dgates || !ln_gate_w || !ln_cell_w || !ln_cell_b)
        return fail(SAT_EINVAL, "lstm_ln_cell_bwd: null pointer");
    if (rows < 1 || n < 1 || g_ld < 4 * (int64_t)n || dg_ld < 4 * (int64_t)n)
        return fail(SAT_EINVAL, "lstm_ln_cell_bwd: bad shape (rows=%d n=%d g_ld=%d dg_ld=%d)", rows, n, g_ld, dg_ld);
    const LnCell ln{ln_gate_w, nullptr, ln_cell_w, ln_cell_b};
    return lstm_ln_cell_bwd(gates, g_ld, c_prev, xhat, rstd, dh_out, dh_carry, dc_carry, dgates, dg_ld, live, 0, rows, n, dgates_bf16, ln, part, (hipStream_t)stream);
}
int sat_lstm_ln_param_grads(const float* part, int32_t slots, int32_t n, float* d_gate_w, float* d_gate_b, float* d_cell_w, float* d_cell_b, float* scratch,
                            void* stream) {
    if (!part || !d_gate_w || !d_gate_b || !d_cell_w || !d_cell_b || !scratch) return fail(SAT_EINVAL, "lstm_ln_param_grads: null pointer");
    if (slots < 1 || slots > sat_lstm_ln_slots(slots) || n < 1) return fail(SAT_EINVAL, "lstm_ln_param_grads: bad shape (slots=%d n=%d)", slots, n);
    return ln_param_grads(part, slots, n, d_gate_w, d_gate_b, d_cell_w, d_cell_b, scratch, (hipStream_t)stream);
}

int sat_decoder_pack_weights(const sat_decoder_dims* d, const sat_decoder_params* w, float* wcat, void* wcat_bf16, float* bcat, void* stream) {
    SAT_TRY(check_dims(d));
    if (!w || !w->att_dec || !w->beta_w || !w->w_hh || !w->beta_b || !w->b_ih || !w->b_hh || !wcat || !bcat)
        return fail(SAT_EINVAL, "decoder_pack_weights: null tensor or output");
    return pack_weights_public(*d, *w, wcat, wcat_bf16, bcat, (hipStream_t)stream);
}

static int check_activation_reg(const char* what, const void* hidden, const void* lengths, const void* p2, const char* n2, const void* p3, const char* n3,
                                int32_t N, int32_t T1, int32_t n, int64_t P, int64_t Q) {
    if (!hidden || !lengths || !p2 || !p3)
        return fail(SAT_EINVAL, "%s: null pointer (%s)", what, !hidden ? "hidden" : !lengths ? "lengths" : !p2 ? n2 : n3);
    if (N <= 0 || T1 <= 0 || n <= 0) return fail(SAT_EINVAL, "%s: non-positive size (N=%d T1=%d n=%d)", what, N, T1, n);
    if (P < 0 || Q < 0 || Q > P || P > (int64_t)N * T1)
        return fail(SAT_EINVAL, "%s: live counts P=%lld Q=%lld outside 0 <= Q <= P <= N*T1=%lld", what, (long long)P, (long long)Q, (long long)N * T1);
    return SAT_OK;
}
size_t sat_activation_reg_scratch_bytes(int32_t N, int32_t T1, int32_t n) {
    if (N <= 0 || T1 <= 0 || n <= 0) { fail(SAT_EINVAL, "activation_reg_scratch_bytes: non-positive size (N=%d T1=%d n=%d)", N, T1, n); return 0; }
    return activation_reg_scratch_bytes(N, T1, n);
}
int sat_activation_reg_fwd(const float* hidden, const int32_t* lengths, int32_t N, int32_t T1, int32_t n, int64_t P, int64_t Q, void* scratch, float* out,
                           void* stream) {
    SAT_TRY(check_activation_reg("activation_reg_fwd", hidden, lengths, scratch, "scratch", out, "out", N, T1, n, P, Q));
    return activation_reg_fwd(hidden, lengths, N, T1, n, (long)P, (long)Q, scratch, out, (hipStream_t)stream);
}
int sat_activation_reg_bwd(const float* hidden, const int32_t* lengths, int32_t N, int32_t T1, int32_t n, int64_t P, int64_t Q, const float* gscale, float* dH,
                           void* stream) {
    SAT_TRY(check_activation_reg("activation_reg_bwd", hidden, lengths, gscale, "gscale", dH, "dH", N, T1, n, P, Q));
    return activation_reg_bwd(hidden, lengths, N, T1, n, (long)P, (long)Q, gscale, dH, (hipStream_t)stream);
}

int sat_ce_label_smooth_fwd(const float* logits, const int32_t* targets, int32_t P, int32_t V, float smoothing, float* lse_rows,
                            float* loss_rows, int32_t* correct_rows, float* out, void* stream) {
    if (!logits || !targets || !lse_rows || !loss_rows || !correct_rows || !out) return fail(SAT_EINVAL, "ce_label_smooth_fwd: null pointer");
    return ce_fwd(logits, targets, P, V, smoothing, lse_rows, loss_rows, correct_rows, out, (hipStream_t)stream);
}
int sat_ce_label_smooth_bwd(const float* logits, const int32_t* targets, const float* lse_rows, int32_t P, int32_t V, float smoothing,
                            const float* gscale, float* dlogits, void* stream) {
    if (!logits || !targets || !lse_rows || !dlogits) return fail(SAT_EINVAL, "ce_label_smooth_bwd: null pointer");
    return ce_bwd(logits, targets, lse_rows, P, V, smoothing, gscale, dlogits, (hipStream_t)stream);
}
int sat_doubly_stochastic_fwd(const float* alphas, int32_t N, int32_t T1, int32_t L, float gamma, float* asum, float* part, float* out, void* stream) {
    if (!alphas || !asum || !part || !out) return fail(SAT_EINVAL, "doubly_stochastic_fwd: null pointer");
    return ds_fwd(alphas, N, T1, L, gamma, asum, part, out, (hipStream_t)stream);
}
int sat_doubly_stochastic_bwd(const float* asum, const float* gscale, int32_t N, int32_t T1, int32_t L, float gamma, float* dalphas, void* stream) {
    if (!asum || !dalphas) return fail(SAT_EINVAL, "doubly_stochastic_bwd: null pointer");
    return ds_bwd(asum, gscale, N, T1, L, gamma, dalphas, (hipStream_t)stream);
}

size_t sat_temperature_workspace_bytes(int32_t P, int32_t V) {
    if (P <= 0 || V <= 0) { fail(SAT_EINVAL, "temperature_workspace_bytes: non-positive size (P=%d V=%d)", P, V); return 0; }
    return temperature_workspace_bytes(P, V);
}
int sat_temperature_nll(const float* logits, const int32_t* targets, int32_t P, int32_t V, const float* temperatures, int32_t n_temperatures,
                        float* loss_out, float* grad_out, void* workspace, void* stream) {
    if (!logits || !targets || !temperatures || !loss_out || !grad_out || !workspace) return fail(SAT_EINVAL, "temperature_nll: null pointer");
    if (P <= 0 || V <= 0) return fail(SAT_EINVAL, "temperature_nll: empty input (P=%d V=%d)", P, V);
    if (n_temperatures < 1 || n_temperatures > SAT_TEMPERATURE_MAX)
        return fail(SAT_EINVAL, "temperature_nll: %d temperatures (1..%d in one pass)", n_temperatures, SAT_TEMPERATURE_MAX);
    if ((uintptr_t)workspace % 16) return fail(SAT_EINVAL, "temperature_nll: workspace must be 16-byte aligned");
    return temperature_nll(logits, targets, P, V, temperatures, n_temperatures, loss_out, grad_out, (char*)workspace, (hipStream_t)stream);
}
int sat_temperature_fit(const float* logits, const int32_t* targets, int32_t P, int32_t V, float init, float lr, float momentum, int32_t nesterov,
                        int32_t iters, float* t_trace, float* loss_trace, void* workspace, void* stream) {
    if (!logits || !targets || !t_trace || !loss_trace || !workspace) return fail(SAT_EINVAL, "temperature_fit: null pointer");
    if (P <= 0 || V <= 0 || iters <= 0) return fail(SAT_EINVAL, "temperature_fit: non-positive size (P=%d V=%d iters=%d)", P, V, iters);
    if (!(init > 0.f) || !(init < INFINITY)) return fail(SAT_EINVAL, "temperature_fit: initial temperature %g is not a positive finite number", init);
    if (!(lr > 0.f)) return fail(SAT_EINVAL, "temperature_fit: learning rate %g is not positive", lr);
    if (!(momentum >= 0.f)) return fail(SAT_EINVAL, "temperature_fit: momentum %g is negative", momentum);
    if ((uintptr_t)workspace % 16) return fail(SAT_EINVAL, "temperature_fit: workspace must be 16-byte aligned");
    return temperature_fit(logits, targets, P, V, init, lr, momentum, nesterov ? 1 : 0, iters, t_trace, loss_trace, (char*)workspace, (hipStream_t)stream);
}

size_t sat_decoder_infer_workspace_bytes(const sat_decoder_dims* d, int32_t max_beams) {
    if (check_dims(d) != SAT_OK || max_beams < 1) return 0;
    return decoder_infer_workspace_bytes(*d, max_beams);
}
int sat_decoder_infer_begin(const sat_decoder_dims* d, const sat_decoder_params* w, const float* ann, int32_t beams, int32_t max_beams,
                            float* h, float* c, void* workspace, size_t workspace_bytes, void* stream) {
    SAT_TRY(check_dims(d)); SAT_TRY(check_params(d, w, "decoder_infer_begin"));
    if (!ann || !h || !c || !workspace) return fail(SAT_EINVAL, "decoder_infer_begin: null pointer");
    return decoder_infer_begin(*d, *w, ann, beams, max_beams, h, c, (char*)workspace, workspace_bytes, (hipStream_t)stream);
}
int sat_decoder_infer_step(const sat_decoder_dims* d, const sat_decoder_params* w, const float* ann, const int32_t* tokens, int32_t beams,
                           int32_t max_beams, float* h, float* c, float* logits, float* alpha, const float* h_noise, void* workspace,
                           size_t workspace_bytes, void* stream) {
    SAT_TRY(check_dims(d)); SAT_TRY(check_params(d, w, "decoder_infer_step"));
    if (!ann || !tokens || !h || !c || !logits || !alpha || !workspace) return fail(SAT_EINVAL, "decoder_infer_step: null pointer");
    return decoder_infer_step(*d, *w, ann, tokens, beams, max_beams, h, c, logits, alpha, h_noise, (char*)workspace, workspace_bytes, (hipStream_t)stream);
}
// ---- the batched search: one descriptor, one plan (decoder.hip: beam_plan), one entry point
static int check_ensemble(const sat_beam_ensemble* e, const char* what) {
    SAT_TRY(beam_ensemble_check(e, what));
    for (int i = 0; i < e->members; ++i) { SAT_TRY(check_dims(e->dims[i])); SAT_TRY(check_params(e->dims[i], e->params[i], what)); }
    return SAT_OK;
}
// what every search entry checks in front of the plan, under the caller's name; o == NULL: the workspace query, which has no outputs
static int check_search(const sat_beam_search_desc* s, const sat_beam_search_out* o, const void* workspace, const char* what) {
    if (s->ensemble) SAT_TRY(check_ensemble(s->ensemble, what));
    else { SAT_TRY(check_dims(s->d)); SAT_TRY(check_params(s->d, s->w, what)); }
    if ((!s->ensemble && !s->ann) || !s->temperatures_host || !s->special_ids_host ||
        (o && (!o->tok_in || !o->prev_row || !o->alpha_hist || !o->fin_count || !o->fin_step || !o->fin_row || !o->fin_score || !o->fin_mean || !workspace)))
        return fail(SAT_EINVAL, "%s: null pointer", what);
    for (int i = 0; i < s->n_temperatures; ++i) if (!(s->temperatures_host[i] > 0.f)) return fail(SAT_EINVAL, "%s: temperature %g", what, s->temperatures_host[i]);
    return SAT_OK;
}
static int search_as(const char* what, const sat_beam_search_desc& s, const sat_beam_search_out& o, void* workspace, size_t workspace_bytes, void* stream) {
    SAT_TRY(check_search(&s, &o, workspace, what));
    return beam_search(s, o, (char*)workspace, workspace_bytes, (hipStream_t)stream);
}
size_t sat_beam_search_desc_workspace_bytes(const sat_beam_search_desc* s) {
    size_t total = 0;
    if (!s) { fail(SAT_EINVAL, "beam_search_desc_workspace_bytes: null descriptor"); return 0; }
    if (check_search(s, nullptr, nullptr, "beam_search_desc_workspace_bytes") != SAT_OK || beam_search_workspace_bytes(*s, total) != SAT_OK) return 0;
    return total;
}
int sat_beam_search(const sat_beam_search_desc* s, const sat_beam_search_out* o, void* workspace, size_t workspace_bytes, void* stream) {
    if (!s) return fail(SAT_EINVAL, "beam_search: null descriptor");
    if (!o) return fail(SAT_EINVAL, "beam_search: null output struct");
    return search_as("beam_search", *s, *o, workspace, workspace_bytes, stream);
}
// ---- the entry points and queries from before the descriptor, kept for existing callers: each search fills a descriptor and runs the
// shared path under its own name; each query keeps its documented figure (an upper bound of the plan's for the features it names)
#define SAT_SINGLE_DESC(sampling, constraints, history, groups, required) \
    {d, w, ann, nullptr, beamk, max_gen_length, temperatures_host, n_temperatures, 0, special_ids_host, sampling, constraints, history, groups, required}
#define SAT_SEARCH_OUT(req_met) {tok_in, prev_row, alpha_hist, fin_count, fin_step, fin_row, fin_score, fin_mean, req_met}
size_t sat_beam_search_workspace_bytes(const sat_decoder_dims* d, int32_t beamk) {
    if (check_dims(d) != SAT_OK || beamk < 1) return 0;
    return decoder_beam_workspace_bytes(*d, beamk, 0, 0, 1);
}
int sat_beam_search_batched(const sat_decoder_dims* d, const sat_decoder_params* w, const float* ann, int32_t beamk, int32_t max_gen_length,
                            const float* temperatures_host, int32_t n_temperatures, const int32_t* special_ids_host, int32_t* tok_in, int32_t* prev_row,
                            float* alpha_hist, int32_t* fin_count, int32_t* fin_step, int32_t* fin_row, float* fin_score, float* fin_mean, void* workspace,
                            size_t workspace_bytes, void* stream) {
    const sat_beam_search_desc s = SAT_SINGLE_DESC(nullptr, nullptr, nullptr, nullptr, nullptr);
    return search_as("beam_search_batched", s, SAT_SEARCH_OUT(nullptr), workspace, workspace_bytes, stream);
}
int sat_beam_search_sampled(const sat_decoder_dims* d, const sat_decoder_params* w, const float* ann, int32_t beamk, int32_t max_gen_length,
                            const float* temperatures_host, int32_t n_temperatures, const int32_t* special_ids_host, const sat_beam_sampling* sampling,
                            int32_t* tok_in, int32_t* prev_row, float* alpha_hist, int32_t* fin_count, int32_t* fin_step, int32_t* fin_row, float* fin_score,
                            float* fin_mean, void* workspace, size_t workspace_bytes, void* stream) {
    const sat_beam_search_desc s = SAT_SINGLE_DESC(sampling, nullptr, nullptr, nullptr, nullptr);
    return search_as("beam_search_sampled", s, SAT_SEARCH_OUT(nullptr), workspace, workspace_bytes, stream);
}
size_t sat_beam_search_constrained_workspace_bytes(const sat_decoder_dims* d, int32_t beamk, int32_t topg) {
    if (check_dims(d) != SAT_OK || beamk < 1) return 0;
    if (topg < 0 || topg > d->V) { fail(SAT_EINVAL, "beam_search_constrained_workspace_bytes: topg %d outside 0..V=%d", topg, d->V); return 0; }
    return decoder_beam_workspace_bytes(*d, beamk, topg, 0, 1);
}
int sat_beam_search_constrained(const sat_decoder_dims* d, const sat_decoder_params* w, const float* ann, int32_t beamk, int32_t max_gen_length,
                                const float* temperatures_host, int32_t n_temperatures, const int32_t* special_ids_host, const sat_beam_sampling* sampling,
                                const sat_beam_constraints* constraints, int32_t* tok_in, int32_t* prev_row, float* alpha_hist, int32_t* fin_count,
                                int32_t* fin_step, int32_t* fin_row, float* fin_score, float* fin_mean, void* workspace, size_t workspace_bytes, void* stream) {
    const sat_beam_search_desc s = SAT_SINGLE_DESC(sampling, constraints, nullptr, nullptr, nullptr);
    return search_as("beam_search_constrained", s, SAT_SEARCH_OUT(nullptr), workspace, workspace_bytes, stream);
}
size_t sat_beam_search_history_workspace_bytes(const sat_decoder_dims* d, int32_t beamk, int32_t topg, int32_t max_gen_length) {
    if (check_dims(d) != SAT_OK || beamk < 1) return 0;
    if (topg < 0 || topg > d->V) { fail(SAT_EINVAL, "beam_search_history_workspace_bytes: topg %d outside 0..V=%d", topg, d->V); return 0; }
    if (max_gen_length < 0 || max_gen_length + 1 > SAT_CAPTION_MAX_LEN) {
        fail(SAT_EINVAL, "beam_search_history_workspace_bytes: max_gen_length %d outside 0..%d", max_gen_length, SAT_CAPTION_MAX_LEN - 1);
        return 0;
    }
    return decoder_beam_workspace_bytes(*d, beamk, topg, max_gen_length + 1, 1);
}
int sat_beam_search_history(const sat_decoder_dims* d, const sat_decoder_params* w, const float* ann, int32_t beamk, int32_t max_gen_length,
                            const float* temperatures_host, int32_t n_temperatures, const int32_t* special_ids_host, const sat_beam_sampling* sampling,
                            const sat_beam_constraints* constraints, const sat_beam_history* history, int32_t* tok_in, int32_t* prev_row, float* alpha_hist,
                            int32_t* fin_count, int32_t* fin_step, int32_t* fin_row, float* fin_score, float* fin_mean, void* workspace, size_t workspace_bytes,
                            void* stream) {
    const sat_beam_search_desc s = SAT_SINGLE_DESC(sampling, constraints, history, nullptr, nullptr);
    return search_as("beam_search_history", s, SAT_SEARCH_OUT(nullptr), workspace, workspace_bytes, stream);
}
size_t sat_beam_search_groups_workspace_bytes(const sat_decoder_dims* d, int32_t beamk, int32_t groups, int32_t max_gen_length) {
    if (check_dims(d) != SAT_OK || beamk < 1) return 0;
    if (groups < 0 || (groups > 1 && beamk % groups != 0)) {
        fail(SAT_EINVAL, "beam_search_groups_workspace_bytes: beamk %d is not a multiple of groups %d (0 or 1 = off)", beamk, groups);
        return 0;
    }
    if (max_gen_length < 0) { fail(SAT_EINVAL, "beam_search_groups_workspace_bytes: max_gen_length %d is negative", max_gen_length); return 0; }
    // room for the history tables too where the history rules can run at all (max_gen_length + 1 <= SAT_CAPTION_MAX_LEN)
    return decoder_beam_workspace_bytes(*d, beamk, 0, max_gen_length + 1 <= SAT_CAPTION_MAX_LEN ? max_gen_length + 1 : 0, groups);
}
int sat_beam_search_groups(const sat_decoder_dims* d, const sat_decoder_params* w, const float* ann, int32_t beamk, int32_t max_gen_length,
                           const float* temperatures_host, int32_t n_temperatures, const int32_t* special_ids_host, const sat_beam_sampling* sampling,
                           const sat_beam_constraints* constraints, const sat_beam_history* history, const sat_beam_groups* groups, int32_t* tok_in,
                           int32_t* prev_row, float* alpha_hist, int32_t* fin_count, int32_t* fin_step, int32_t* fin_row, float* fin_score, float* fin_mean,
                           void* workspace, size_t workspace_bytes, void* stream) {
    const sat_beam_search_desc s = SAT_SINGLE_DESC(sampling, constraints, history, groups, nullptr);
    return search_as("beam_search_groups", s, SAT_SEARCH_OUT(nullptr), workspace, workspace_bytes, stream);
}
size_t sat_beam_search_required_workspace_bytes(const sat_decoder_dims* d, int32_t beamk, int32_t max_gen_length, int32_t max_required) {
    if (check_dims(d) != SAT_OK || beamk < 1) return 0;
    if (max_gen_length < 0) { fail(SAT_EINVAL, "beam_search_required_workspace_bytes: max_gen_length %d is negative", max_gen_length); return 0; }
    const sat_beam_required shape = {max_required, 0, (const int32_t*)d, (const int32_t*)d};      // the sizes only: the pointers are not read
    if (beam_required_check(&shape, beamk, max_gen_length, "beam_search_required_workspace_bytes") != SAT_OK) return 0;
    // room for the history tables where they can exist at all (required words off and max_gen_length + 1 > SAT_CAPTION_MAX_LEN: none)
    return decoder_beam_workspace_bytes(*d, beamk, 0, max_gen_length + 1 <= SAT_CAPTION_MAX_LEN ? max_gen_length + 1 : 0, 1);
}
int sat_beam_search_required(const sat_decoder_dims* d, const sat_decoder_params* w, const float* ann, int32_t beamk, int32_t max_gen_length,
                             const float* temperatures_host, int32_t n_temperatures, const int32_t* special_ids_host, const sat_beam_sampling* sampling,
                             const sat_beam_constraints* constraints, const sat_beam_history* history, const sat_beam_required* required,
                             int32_t* tok_in, int32_t* prev_row, float* alpha_hist, int32_t* fin_count, int32_t* fin_step, int32_t* fin_row,
                             float* fin_score, float* fin_mean, int32_t* req_met, void* workspace, size_t workspace_bytes, void* stream) {
    const sat_beam_search_desc s = SAT_SINGLE_DESC(sampling, constraints, history, nullptr, required);
    return search_as("beam_search_required", s, SAT_SEARCH_OUT(req_met), workspace, workspace_bytes, stream);
}
size_t sat_beam_search_ensemble_workspace_bytes(const sat_beam_ensemble* ensemble, int32_t beamk, int32_t max_gen_length) {
    if (beam_ensemble_check(ensemble, "beam_search_ensemble_workspace_bytes") != SAT_OK) return 0;
    for (int i = 0; i < ensemble->members; ++i) if (check_dims(ensemble->dims[i]) != SAT_OK) return 0;
    if (beamk < 1 || max_gen_length < 0) { fail(SAT_EINVAL, "beam_search_ensemble_workspace_bytes: beamk %d, max_gen_length %d", beamk, max_gen_length); return 0; }
    return decoder_beam_ensemble_workspace_bytes(*ensemble, beamk, max_gen_length + 1 <= SAT_CAPTION_MAX_LEN ? max_gen_length + 1 : 0);
}
int sat_beam_search_ensemble(const sat_beam_ensemble* ensemble, int32_t beamk, int32_t max_gen_length, const float* temperatures_host,
                             int32_t n_temperatures, const int32_t* special_ids_host, const sat_beam_constraints* constraints,
                             const sat_beam_history* history, int32_t* tok_in, int32_t* prev_row, float* alpha_hist, int32_t* fin_count,
                             int32_t* fin_step, int32_t* fin_row, float* fin_score, float* fin_mean, void* workspace, size_t workspace_bytes,
                             void* stream) {
    if (!ensemble) return beam_ensemble_check(ensemble, "beam_search_ensemble");        // "null ensemble struct": a descriptor without one is a single-model search
    const sat_beam_search_desc s = {nullptr, nullptr, nullptr, ensemble, beamk, max_gen_length, temperatures_host, n_temperatures, 0, special_ids_host,
                                    nullptr, constraints, history, nullptr, nullptr};
    return search_as("beam_search_ensemble", s, SAT_SEARCH_OUT(nullptr), workspace, workspace_bytes, stream);
}
#undef SAT_SINGLE_DESC
#undef SAT_SEARCH_OUT
int sat_beam_required_select(const float* scores, const int32_t* klive, int32_t B, int32_t beamk, int32_t V, const int32_t* hist, int32_t hist_stride,
                             int32_t hist_len, int32_t first_step, const sat_beam_required* required, int32_t end_id, float* work, float* values,
                             int32_t* indices, void* stream) {
    if (!scores || !klive || !required || !work || !values || !indices) return fail(SAT_EINVAL, "beam_required_select: null pointer");
    return beam_required_select(scores, klive, B, beamk, V, hist, hist_stride, hist_len, first_step, *required, end_id, work, values, indices, (hipStream_t)stream);
}
int sat_beam_ensemble_scores(const float* const* logits, const float* weights, int32_t members, int32_t combine, int32_t rows, int32_t V,
                             float temperature, float* combined, void* stream) {
    if (!logits || !weights || !combined) return fail(SAT_EINVAL, "beam_ensemble_scores: null pointer");
    return beam_ensemble_scores(logits, weights, members, combine, rows, V, temperature, combined, (hipStream_t)stream);
}
int sat_beam_group_select(const float* scores, const int32_t* klive, int32_t B, int32_t beamk, int32_t groups, int32_t V, int32_t first_step,
                          float diversity_penalty, float* work, float* values, int32_t* indices, void* stream) {
    if (!scores || !klive || !work || !values || !indices) return fail(SAT_EINVAL, "beam_group_select: null pointer");
    return beam_group_select(scores, klive, B, beamk, groups, V, first_step, diversity_penalty, work, values, indices, (hipStream_t)stream);
}
int sat_beam_history_scores(const float* logits, int32_t rows, int32_t V, float temperature, const int32_t* masked_ids, int32_t n_masked,
                            const float* parent_scores, const int32_t* hist, const int32_t* hist_len, int32_t hist_stride, const sat_beam_history* rules,
                            int32_t step, int32_t end_id, float* scores, void* stream) {
    if (rows < 1 || V < 1) return fail(SAT_EINVAL, "beam_history_scores: non-positive size (rows=%d V=%d)", rows, V);
    if (!(temperature > 0.f)) return fail(SAT_EINVAL, "beam_history_scores: temperature %g", (double)temperature);
    if (hist_stride < 0 || hist_stride > SAT_CAPTION_MAX_LEN)
        return fail(SAT_EINVAL, "beam_history_scores: hist_stride %d outside 0..%d", hist_stride, SAT_CAPTION_MAX_LEN);
    if (!logits || !scores || !rules || !hist_len || (hist_stride > 0 && !hist) || (n_masked > 0 && !masked_ids))
        return fail(SAT_EINVAL, "beam_history_scores: null pointer");
    SAT_TRY(beam_history_check(rules, -1, "beam_history_scores"));
    return beam_history_scores(logits, rows, V, temperature, masked_ids, n_masked < 0 ? 0 : n_masked, parent_scores, hist, hist_len, hist_stride, *rules, step,
                               end_id, scores, (hipStream_t)stream);
}
int sat_beam_select(const int32_t* tok_in, const int32_t* prev_row, const int32_t* fin_count, const int32_t* fin_step, const int32_t* fin_row,
                    const float* fin_score, const float* fin_mean, const float* alpha_hist, int32_t B, int32_t beamk, int32_t max_gen_length, int32_t L,
                    int32_t rescore_method, float rescore_reward, int32_t pad_id, int32_t* cap_tokens, int32_t* cap_len, float* cap_score, float* cap_raw,
                    int32_t* cap_step, float* cap_alpha, void* stream) {
    if (!tok_in || !prev_row || !fin_count || !fin_step || !fin_row || !fin_score || !fin_mean || !cap_tokens || !cap_len || !cap_score || !cap_raw || !cap_step)
        return fail(SAT_EINVAL, "beam_select: null pointer");
    if (cap_alpha && !alpha_hist) return fail(SAT_EINVAL, "beam_select: cap_alpha asked for without alpha_hist (null pointer)");
    if (B < 1 || beamk < 1 || max_gen_length < 1 || (cap_alpha && L < 1))
        return fail(SAT_EINVAL, "beam_select: non-positive size (B=%d beamk=%d max_gen_length=%d L=%d)", B, beamk, max_gen_length, L);
    if (max_gen_length + 1 > SAT_CAPTION_MAX_LEN)
        return fail(SAT_EINVAL, "beam_select: max_gen_length %d is over the limit (max_gen_length + 1 <= %d)", max_gen_length, SAT_CAPTION_MAX_LEN);
    if (rescore_method < SAT_RESCORE_NONE || rescore_method > SAT_RESCORE_BAR) return fail(SAT_EINVAL, "beam_select: rescore_method %d (0..3)", rescore_method);
    return beam_select(tok_in, prev_row, fin_count, fin_step, fin_row, fin_score, fin_mean, alpha_hist, B, beamk, max_gen_length, L, rescore_method,
                       rescore_reward, pad_id, cap_tokens, cap_len, cap_score, cap_raw, cap_step, cap_alpha, (hipStream_t)stream);
}
int sat_beam_select_at(const int32_t* tok_in, const int32_t* prev_row, const int32_t* fin_count, const int32_t* fin_step, const int32_t* fin_row,
                       const float* fin_score, const float* alpha_hist, const int32_t* pick, const double* pick_score, int32_t B, int32_t beamk,
                       int32_t max_gen_length, int32_t L, int32_t pad_id, int32_t* cap_tokens, int32_t* cap_len, float* cap_score, float* cap_raw,
                       int32_t* cap_step, float* cap_alpha, void* stream) {
    if (!tok_in || !prev_row || !fin_count || !fin_step || !fin_row || !fin_score || !pick || !cap_tokens || !cap_len || !cap_score || !cap_raw || !cap_step)
        return fail(SAT_EINVAL, "beam_select_at: null pointer");
    if (cap_alpha && !alpha_hist) return fail(SAT_EINVAL, "beam_select_at: cap_alpha asked for without alpha_hist (null pointer)");
    if (B < 1 || beamk < 1 || max_gen_length < 1 || (cap_alpha && L < 1))
        return fail(SAT_EINVAL, "beam_select_at: non-positive size (B=%d beamk=%d max_gen_length=%d L=%d)", B, beamk, max_gen_length, L);
    if (max_gen_length + 1 > SAT_CAPTION_MAX_LEN)
        return fail(SAT_EINVAL, "beam_select_at: max_gen_length %d is over the limit (max_gen_length + 1 <= %d)", max_gen_length, SAT_CAPTION_MAX_LEN);
    return beam_select_at(tok_in, prev_row, fin_count, fin_step, fin_row, fin_score, alpha_hist, pick, pick_score, B, beamk, max_gen_length, L, pad_id,
                          cap_tokens, cap_len, cap_score, cap_raw, cap_step, cap_alpha, (hipStream_t)stream);
}
int sat_beam_hypotheses(const int32_t* tok_in, const int32_t* prev_row, const int32_t* fin_count, const int32_t* fin_step, const int32_t* fin_row, int32_t B,
                        int32_t beamk, int32_t max_gen_length, int32_t pad_id, int32_t* hyp_tokens, int32_t* hyp_len, void* stream) {
    if (!tok_in || !prev_row || !fin_count || !fin_step || !fin_row || !hyp_tokens || !hyp_len) return fail(SAT_EINVAL, "beam_hypotheses: null pointer");
    if (B < 1 || beamk < 1 || max_gen_length < 1)
        return fail(SAT_EINVAL, "beam_hypotheses: non-positive size (B=%d beamk=%d max_gen_length=%d)", B, beamk, max_gen_length);
    if (max_gen_length + 1 > SAT_CAPTION_MAX_LEN)
        return fail(SAT_EINVAL, "beam_hypotheses: max_gen_length %d is over the limit (max_gen_length + 1 <= %d)", max_gen_length, SAT_CAPTION_MAX_LEN);
    return beam_hypotheses(tok_in, prev_row, fin_count, fin_step, fin_row, B, beamk, max_gen_length, pad_id, hyp_tokens, hyp_len, (hipStream_t)stream);
}
static int check_caption_sizes(const char* what, int32_t cap_width, int32_t B, int32_t R, int32_t T) {
    if (B < 1 || R < 1 || T < 1 || cap_width < 1) return fail(SAT_EINVAL, "%s: non-positive size (B=%d R=%d T=%d cap_width=%d)", what, B, R, T, cap_width);
    if (R > SAT_CAPTION_MAX_REFS || T > SAT_CAPTION_MAX_LEN || cap_width > SAT_CAPTION_MAX_LEN)
        return fail(SAT_EINVAL, "%s: over the limits (R=%d <= %d, T=%d <= %d, cap_width=%d <= %d)", what, R, SAT_CAPTION_MAX_REFS, T, SAT_CAPTION_MAX_LEN,
                    cap_width, SAT_CAPTION_MAX_LEN);
    return SAT_OK;
}
int sat_caption_stats(const int32_t* cap_tokens, const int32_t* cap_len, int32_t cap_width, const int32_t* refs, const int32_t* ref_lengths, int32_t B,
                      int32_t R, int32_t T, int32_t* stats, void* stream) {
    if (!cap_tokens || !cap_len || !refs || !ref_lengths || !stats) return fail(SAT_EINVAL, "caption_stats: null pointer");
    SAT_TRY(check_caption_sizes("caption_stats", cap_width, B, R, T));
    return caption_stats(cap_tokens, cap_len, cap_width, refs, ref_lengths, B, R, T, stats, (hipStream_t)stream);
}
int sat_caption_cosine(const int32_t* cap_tokens, const int32_t* cap_len, int32_t cap_width, const int32_t* refs, const int32_t* ref_lengths, int32_t B,
                       int32_t R, int32_t T, const float* embedding, int32_t V, int32_t m, float* best_cosine, void* stream) {
    if (!cap_tokens || !cap_len || !refs || !ref_lengths || !embedding || !best_cosine) return fail(SAT_EINVAL, "caption_cosine: null pointer");
    SAT_TRY(check_caption_sizes("caption_cosine", cap_width, B, R, T));
    if (V < 1 || m < 1) return fail(SAT_EINVAL, "caption_cosine: non-positive size (V=%d m=%d)", V, m);
    if (m > SAT_CAPTION_MAX_EMBED) return fail(SAT_EINVAL, "caption_cosine: embedding width %d is over the limit %d", m, SAT_CAPTION_MAX_EMBED);
    return caption_cosine(cap_tokens, cap_len, cap_width, refs, ref_lengths, B, R, T, embedding, V, m, best_cosine, (hipStream_t)stream);
}
size_t sat_ngram_table_bytes(int64_t capacity) {
    if (capacity < 1 || (capacity & (capacity - 1)) || capacity > SAT_NGRAM_TABLE_MAX_CAPACITY) {
        fail(SAT_EINVAL, "ngram_table_bytes: capacity %lld is not a power of two in [1, 2^%d]", (long long)capacity, 36);
        return 0;
    }
    return ngram_table_bytes((long)capacity);
}
static int check_table(const char* what, const void* table, int64_t capacity) {
    if (!table) return fail(SAT_EINVAL, "%s: null pointer", what);
    if (capacity < 1 || (capacity & (capacity - 1)) || capacity > SAT_NGRAM_TABLE_MAX_CAPACITY)
        return fail(SAT_EINVAL, "%s: capacity %lld is not a power of two in [1, 2^%d]", what, (long long)capacity, 36);
    return SAT_OK;
}
int sat_ngram_table_clear(void* table, int64_t capacity, void* stream) {
    SAT_TRY(check_table("ngram_table_clear", table, capacity));
    return ngram_table_clear(table, (long)capacity, (hipStream_t)stream);
}
int sat_ngram_table_add(const int32_t* refs, const int32_t* ref_lengths, int32_t B, int32_t R, int32_t T, void* table, int64_t capacity,
                        int32_t* error_flag, void* stream) {
    if (!refs || !ref_lengths || !error_flag) return fail(SAT_EINVAL, "ngram_table_add: null pointer");
    SAT_TRY(check_table("ngram_table_add", table, capacity));
    SAT_TRY(check_caption_sizes("ngram_table_add", 1, B, R, T));
    return ngram_table_add(refs, ref_lengths, B, R, T, table, (long)capacity, error_flag, (hipStream_t)stream);
}
int sat_caption_consensus(const int32_t* cap_tokens, const int32_t* cap_len, int32_t cap_width, const int32_t* refs, const int32_t* ref_lengths,
                          int32_t B, int32_t R, int32_t T, const void* table, int64_t capacity, int64_t n_images, double sigma, double* scores,
                          void* stream) {
    if (!cap_tokens || !cap_len || !refs || !ref_lengths || !scores) return fail(SAT_EINVAL, "caption_consensus: null pointer");
    SAT_TRY(check_table("caption_consensus", table, capacity));
    SAT_TRY(check_caption_sizes("caption_consensus", cap_width, B, R, T));
    if (n_images < 1) return fail(SAT_EINVAL, "caption_consensus: n_images %lld (the table holds no image)", (long long)n_images);
    if (!(sigma > 0.0)) return fail(SAT_EINVAL, "caption_consensus: sigma %g is not positive", sigma);
    return caption_consensus(cap_tokens, cap_len, cap_width, refs, ref_lengths, B, R, T, table, (long)capacity, (long)n_images, sigma, scores,
                             (hipStream_t)stream);
}
int sat_caption_mbr(const int32_t* hyp_tokens, const int32_t* hyp_len, const int32_t* hyp_count, const float* hyp_logp, int32_t B, int32_t K, int32_t width,
                    const void* table, int64_t capacity, int64_t n_images, double sigma, double w_cider, double w_rouge, double alpha, double* utilities,
                    int32_t* winner, void* stream) {
    const double finite_max = 1.79769313486231570815e308;
    if (!hyp_tokens || !hyp_len || !hyp_count || !utilities || !winner) return fail(SAT_EINVAL, "caption_mbr: null pointer");
    SAT_TRY(check_table("caption_mbr", table, capacity));
    if (B < 1 || K < 1 || width < 1) return fail(SAT_EINVAL, "caption_mbr: non-positive size (B=%d K=%d width=%d)", B, K, width);
    if (K > SAT_MBR_MAX_HYPS || width > SAT_CAPTION_MAX_LEN)
        return fail(SAT_EINVAL, "caption_mbr: over the limits (K=%d <= %d, width=%d <= %d)", K, SAT_MBR_MAX_HYPS, width, SAT_CAPTION_MAX_LEN);
    if (n_images < 1) return fail(SAT_EINVAL, "caption_mbr: n_images %lld (the table holds no image)", (long long)n_images);
    if (!(sigma > 0.0)) return fail(SAT_EINVAL, "caption_mbr: sigma %g is not positive", sigma);
    if (!(w_cider >= 0.0) || w_cider > finite_max || !(w_rouge >= 0.0) || w_rouge > finite_max)
        return fail(SAT_EINVAL, "caption_mbr: weights (%g, %g) are not finite numbers >= 0", w_cider, w_rouge);
    if (w_cider == 0.0 && w_rouge == 0.0) return fail(SAT_EINVAL, "caption_mbr: both weights are 0 (nothing to agree on)");
    if (!(alpha >= 0.0) || alpha > finite_max) return fail(SAT_EINVAL, "caption_mbr: alpha %g is not a finite number >= 0", alpha);
    if (alpha != 0.0 && !hyp_logp) return fail(SAT_EINVAL, "caption_mbr: alpha %g needs hyp_logp (null pointer)", alpha);
    return caption_mbr(hyp_tokens, hyp_len, hyp_count, hyp_logp, B, K, width, table, (long)capacity, (long)n_images, sigma, w_cider, w_rouge, alpha,
                       utilities, winner, (hipStream_t)stream);
}
int sat_caption_diversity(const int32_t* hyp_tokens, const int32_t* hyp_len, const int32_t* hyp_count, int32_t B, int32_t K, int32_t width, int32_t* stats,
                          int32_t* per_hyp, void* stream) {
    if (!hyp_tokens || !hyp_len || !hyp_count || !stats) return fail(SAT_EINVAL, "caption_diversity: null pointer");
    if (B < 0 || K < 1 || width < 1) return fail(SAT_EINVAL, "caption_diversity: bad size (B=%d >= 0, K=%d >= 1, width=%d >= 1)", B, K, width);
    if (K > SAT_MBR_MAX_HYPS || width > SAT_CAPTION_MAX_LEN)
        return fail(SAT_EINVAL, "caption_diversity: over the limits (K=%d <= %d, width=%d <= %d)", K, SAT_MBR_MAX_HYPS, width, SAT_CAPTION_MAX_LEN);
    if (B == 0) return SAT_OK;
    return caption_diversity(hyp_tokens, hyp_len, hyp_count, B, K, width, stats, per_hyp, (hipStream_t)stream);
}
int sat_caption_vocab_usage(const int32_t* cap_tokens, const int32_t* cap_len, int32_t cap_width, int32_t B, int32_t V, int32_t* counts, void* stream) {
    if (!cap_tokens || !cap_len || !counts) return fail(SAT_EINVAL, "caption_vocab_usage: null pointer");
    if (B < 0 || V < 1) return fail(SAT_EINVAL, "caption_vocab_usage: bad size (B=%d >= 0, V=%d >= 1)", B, V);
    if (cap_width < 1 || cap_width > SAT_CAPTION_MAX_LEN)
        return fail(SAT_EINVAL, "caption_vocab_usage: cap_width %d outside 1..%d", cap_width, SAT_CAPTION_MAX_LEN);
    if (B == 0) return SAT_OK;
    return caption_vocab_usage(cap_tokens, cap_len, cap_width, B, V, counts, (hipStream_t)stream);
}
int sat_caption_chrf(const int32_t* cap_tokens, const int32_t* cap_len, int32_t cap_width, const int32_t* refs, const int32_t* ref_lengths, int32_t B,
                     int32_t R, int32_t T, const int32_t* word_offsets, const int32_t* word_chars, int32_t V, int32_t max_word_chars, double beta,
                     double* scores, int32_t* stats, void* stream) {
    if (!cap_tokens || !cap_len || !refs || !ref_lengths || !word_offsets || !word_chars || !scores) return fail(SAT_EINVAL, "caption_chrf: null pointer");
    SAT_TRY(check_caption_sizes("caption_chrf", cap_width, B, R, T));
    if (V < 1 || max_word_chars < 0) return fail(SAT_EINVAL, "caption_chrf: V=%d (>= 1), max_word_chars=%d (>= 0)", V, max_word_chars);
    if ((int64_t)cap_width * max_word_chars > SAT_CHRF_MAX_CHARS || (int64_t)(T - 1) * max_word_chars > SAT_CHRF_MAX_CHARS)
        return fail(SAT_EINVAL, "caption_chrf: a sentence could exceed %d characters (cap_width=%d, T - 1=%d tokens of up to max_word_chars=%d)",
                    SAT_CHRF_MAX_CHARS, cap_width, T - 1, max_word_chars);
    if (!(beta > 0.0) || beta > 1.79769313486231570815e308) return fail(SAT_EINVAL, "caption_chrf: beta %g is not a positive finite number", beta);
    return caption_chrf(cap_tokens, cap_len, cap_width, refs, ref_lengths, B, R, T, word_offsets, word_chars, V, max_word_chars, beta, scores, stats,
                        (hipStream_t)stream);
}
int sat_beam_scores(const float* logits, int32_t beams, int32_t V, float temperature, const int32_t* masked_ids, int32_t n_masked,
                    const float* parent_scores, float* scores, void* stream) {
    if (!logits || !scores || (n_masked > 0 && !masked_ids)) return fail(SAT_EINVAL, "beam_scores: null pointer");
    return beam_scores(logits, beams, V, temperature, masked_ids, n_masked, parent_scores, scores, (hipStream_t)stream);
}
int sat_topk(const float* x, float* work, int64_t n, int32_t k, float* values, int32_t* indices, void* stream) {
    if (!x || !work || !values || !indices) return fail(SAT_EINVAL, "topk: null pointer");
    return topk(x, work, n, k, values, indices, (hipStream_t)stream);
}
int sat_nucleus_keys(const float* scores, int32_t rows, int32_t V, float topp, float step, uint64_t seed, uint64_t stream, const float* gumbel, float* keys,
                     int32_t* nucleus_size, void* stream_handle) {
    if (rows <= 0 || V <= 0) return fail(SAT_EINVAL, "nucleus_keys: non-positive size (rows=%d V=%d)", rows, V);
    if (!(topp > 0.f && topp <= 1.f)) return fail(SAT_EINVAL, "nucleus_keys: topp %g outside (0, 1]", (double)topp);
    if (!(step > 0.f && step < INFINITY)) return fail(SAT_EINVAL, "nucleus_keys: step %g is not a positive finite number", (double)step);
    if (!scores || !keys) return fail(SAT_EINVAL, "nucleus_keys: null pointer");
    return nucleus_keys(scores, rows, V, topp, step, seed, stream, gumbel, keys, nucleus_size, (hipStream_t)stream_handle);
}

int sat_colsum(const float* x, int64_t ld, int64_t rows, int32_t cols, float* out, float* scratch, void* stream) {
    if (!x || !out || !scratch) return fail(SAT_EINVAL, "colsum: null pointer");
    if (rows <= 0 || cols <= 0 || ld < cols) return fail(SAT_EINVAL, "colsum: bad shape");
    return colsum_public(x, ld, rows, cols, out, scratch, (hipStream_t)stream);
}

int sat_attention_precompute(const float* ann, const float* att_enc_w, float* U, int32_t B, int32_t L, int32_t D, int32_t A, void* stream) {
    if (!ann || !att_enc_w || !U) return fail(SAT_EINVAL, "attention_precompute: null pointer");
    GemmArgs g; g.A = ann; g.lda = D; g.B = att_enc_w; g.ldb = D; g.C = U; g.ldc = A; g.M = B * L; g.N = A; g.K = D;
    return launch_gemm(g, (hipStream_t)stream);
}
int sat_attention_step_fwd_ex(const float* ann, const float* U, const float* hc, int32_t hc_ld, const float* att_f, const int32_t* lengths,
                              int32_t step, float* alphas, int32_t T1, float* Z, float* XZ, int32_t B, int32_t R, int32_t L, int32_t D, int32_t A,
                              float* scores_scratch, const void* ann_bf16, void* xz_bf16, void* stream) {
    if (!ann || !U || !hc || !att_f || !lengths || !alphas || !Z || !XZ) return fail(SAT_EINVAL, "attention_step_fwd: null pointer");
    if (B < 1 || R < 1 || L < 1 || D < 1 || A < 1 || T1 < 1 || step < 0 || step >= T1) return fail(SAT_EINVAL, "attention_step_fwd: bad shape");
    if (hc_ld < A + D) return fail(SAT_EINVAL, "attention_step_fwd: hc_ld %d < A+D", hc_ld);
    return launch_attention_fwd((hipStream_t)stream, ann, U, hc, hc_ld, att_f, lengths, step, alphas, T1, Z, XZ, B, R, L, D, A, scores_scratch, xz_bf16, ann_bf16);
}
int sat_attention_step_fwd(const float* ann, const float* U, const float* hc, int32_t hc_ld, const float* att_f, const int32_t* lengths,
                           int32_t step, float* alphas, int32_t T1, float* Z, float* XZ, int32_t B, int32_t R, int32_t L, int32_t D, int32_t A, void* stream) {
    return sat_attention_step_fwd_ex(ann, U, hc, hc_ld, att_f, lengths, step, alphas, T1, Z, XZ, B, R, L, D, A, nullptr, nullptr, nullptr, stream);
}

int sat_attention_step_bwd_ex(const float* ann, const float* U, const float* hc, int32_t hc_ld, const float* att_f, const int32_t* lengths, int32_t step,
                              const float* alphas, const float* dalphas, int32_t T1, const float* Z, const float* dZ, const float* dXZ, float* DZ, float* dhc,
                              int32_t dhc_ld, float* dU, float* dwf_part, float* da_scratch, int32_t B, int32_t R, int32_t L, int32_t D, int32_t A,
                              const void* ann_bf16, void* dhc_bf16, void* stream) {
    if (!ann || !U || !hc || !att_f || !lengths || !alphas || !Z || !dZ || !dXZ || !DZ || !dhc || !dU || !dwf_part || !da_scratch)
        return fail(SAT_EINVAL, "attention_step_bwd: null pointer");
    if (hc_ld < A + D || dhc_ld < A + D) return fail(SAT_EINVAL, "attention_step_bwd: hc_ld %d / dhc_ld %d < A+D", hc_ld, dhc_ld);
    if (B < 1 || R < 1 || L < 1 || D < 1 || A < 1 || T1 < 1 || step < 0 || step >= T1) return fail(SAT_EINVAL, "attention_step_bwd: bad shape");
    return launch_attention_bwd((hipStream_t)stream, ann, U, hc, hc_ld, att_f, lengths, step, alphas, dalphas, T1, Z, dZ, dXZ, DZ, dhc, dhc_ld, dU, dwf_part,
                                da_scratch, B, R, L, D, A, dhc_bf16, ann_bf16);
}
int sat_attention_step_bwd(const float* ann, const float* U, const float* hc, int32_t hc_ld, const float* att_f, const int32_t* lengths, int32_t step,
                           const float* alphas, const float* dalphas, int32_t T1, const float* Z, const float* dZ, const float* dXZ, float* DZ, float* dhc,
                           int32_t dhc_ld, float* dU, float* dwf_part, float* da_scratch, int32_t B, int32_t R, int32_t L, int32_t D, int32_t A, void* stream) {
    return sat_attention_step_bwd_ex(ann, U, hc, hc_ld, att_f, lengths, step, alphas, dalphas, T1, Z, dZ, dXZ, DZ, dhc, dhc_ld, dU, dwf_part, da_scratch,
                                     B, R, L, D, A, nullptr, nullptr, stream);
}
int sat_attention_step_plan(int32_t op, int32_t B, int32_t R, int32_t L, int32_t D, int32_t A, int32_t hc_ld, int32_t T1, int32_t flags, int32_t out[9]) {
    if (!out) return fail(SAT_EINVAL, "attention_step_plan: null pointer");
    for (int i = 0; i < 9; ++i) out[i] = 0;
    if (B < 1) return fail(SAT_EINVAL, "attention_step_plan: B=%d", B);
    if (flags < 0 || flags > 15) return fail(SAT_EINVAL, "attention_step_plan: flags=%d outside 0..15", flags);
    AttPlan p;
    SAT_TRY(attention_plan(op, R, L, D, A, hc_ld, T1, (unsigned)flags, p, "attention_step_plan"));
    out[0] = p.form; out[1] = p.rn; out[2] = p.passes; out[3] = p.vw; out[4] = p.dchunk; out[5] = p.nq; out[6] = p.lq; out[7] = (int32_t)p.lds0; out[8] = (int32_t)p.lds1;
    return SAT_OK;
}
int sat_attention_context_bwd(const float* alphas, const float* DZ, const int32_t* lengths, float* dann, int32_t accumulate, int32_t B, int32_t R, int32_t T1,
                              int32_t L, int32_t D, void* stream) {
    if (!alphas || !DZ || !lengths || !dann) return fail(SAT_EINVAL, "attention_context_bwd: null pointer");
    if (B < 1 || R < 1 || L < 1 || D < 1 || T1 < 1) return fail(SAT_EINVAL, "attention_context_bwd: bad shape");
    return attention_context_bwd(alphas, DZ, lengths, dann, accumulate, B, R, T1, L, D, (hipStream_t)stream);
}
int sat_lstm_cell_fwd(const float* x, int32_t in, const float* h_prev, const float* c_prev, const float* w_ih, const float* w_hh, const float* b_ih,
                      const float* b_hh, float* gates, float* h_new, float* c_new, float* bias_scratch, int32_t N, int32_t n, void* stream) {
    if (!x || !h_prev || !c_prev || !w_ih || !w_hh || !b_ih || !b_hh || !gates || !h_new || !c_new || !bias_scratch) return fail(SAT_EINVAL, "lstm_cell_fwd: null pointer");
    if (N < 1 || n < 1 || in < 1) return fail(SAT_EINVAL, "lstm_cell_fwd: bad shape (N=%d n=%d in=%d)", N, n, in);
    return lstm_cell_fwd(x, in, h_prev, c_prev, w_ih, w_hh, b_ih, b_hh, gates, h_new, c_new, bias_scratch, N, n, (hipStream_t)stream);
}
int sat_lstm_cell_bwd(const float* x, int32_t in, const float* h_prev, const float* c_prev, const float* c_new, const float* gates, const float* dh_new,
                      const float* dc_new, const float* w_ih, const float* w_hh, float* dx, float* dh_prev, float* dc_prev, float* dw_ih, float* dw_hh,
                      float* db_ih, float* db_hh, float* dgates, float* scratch, int32_t N, int32_t n, void* stream) {
    if (!x || !h_prev || !c_prev || !c_new || !gates || !dh_new || !w_ih || !w_hh || !dx || !dh_prev || !dc_prev || !dw_ih || !dw_hh || !db_ih || !db_hh || !dgates || !scratch)
        return fail(SAT_EINVAL, "lstm_cell_bwd: null pointer");
    if (N < 1 || n < 1 || in < 1) return fail(SAT_EINVAL, "lstm_cell_bwd: bad shape (N=%d n=%d in=%d)", N, n, in);
    return lstm_cell_bwd(x, in, h_prev, c_prev, c_new, gates, dh_new, dc_new, w_ih, w_hh, dx, dh_prev, dc_prev, dw_ih, dw_hh, db_ih, db_hh, dgates, scratch, N, n,
                         (hipStream_t)stream);
}
int sat_deep_output_fwd(const float* prev_embed, const float* hidden, const float* context, const float* w_hidden, const float* w_context, const float* w_out,
                        const float* b_out, float dropout, uint64_t seed, float* u, float* udrop, float* logits, int32_t N, int32_t m, int32_t n, int32_t D,
                        int32_t V, void* stream) {
    if (!hidden || !w_hidden || !w_out || !u || !logits) return fail(SAT_EINVAL, "deep_output_fwd: null pointer");
    if (context && (!w_context || !prev_embed)) return fail(SAT_EINVAL, "deep_output_fwd: the deep form needs output.context.weight and the previous embedding");
    if (!(dropout >= 0.f && dropout < 1.f) || (dropout > 0.f && !udrop)) return fail(SAT_EINVAL, "deep_output_fwd: dropout %g needs a udrop buffer", dropout);
    if (N < 1 || m < 1 || n < 1 || V < 1 || (context && D < 1)) return fail(SAT_EINVAL, "deep_output_fwd: bad shape");
    return deep_output_fwd(prev_embed, hidden, context, w_hidden, w_context, w_out, b_out, dropout, seed, u, udrop, logits, N, m, n, D, V, (hipStream_t)stream);
}
int sat_deep_output_bwd(const float* dlogits, const float* hidden, const float* context, const float* u, const float* udrop, const float* w_hidden,
                        const float* w_context, const float* w_out, float dropout, uint64_t seed, float* d_prev_embed, float* d_hidden, float* d_context,
                        float* dw_hidden, float* dw_context, float* dw_out, float* db_out, float* scratch, int32_t N, int32_t m, int32_t n, int32_t D, int32_t V,
                        void* stream) {
    if (!dlogits || !hidden || !u || !w_hidden || !w_out || !d_prev_embed || !d_hidden || !dw_hidden || !dw_out || !scratch) return fail(SAT_EINVAL, "deep_output_bwd: null pointer");
    if (context && (!w_context || !d_context || !dw_context)) return fail(SAT_EINVAL, "deep_output_bwd: the deep form needs the context weight and gradient buffers");
    if (!(dropout >= 0.f && dropout < 1.f) || (dropout > 0.f && !udrop)) return fail(SAT_EINVAL, "deep_output_bwd: dropout %g needs the forward's udrop buffer", dropout);
    if (N < 1 || m < 1 || n < 1 || V < 1 || (context && D < 1)) return fail(SAT_EINVAL, "deep_output_bwd: bad shape");
    return deep_output_bwd(dlogits, hidden, context, u, udrop, w_hidden, w_context, w_out, dropout, seed, d_prev_embed, d_hidden, d_context, dw_hidden, dw_context,
                           dw_out, db_out, scratch, N, m, n, D, V, (hipStream_t)stream);
}
int sat_init_lstm_fwd(const float* ann, const float* w_f, const float* b_f, const float* w_i, const float* b_i, float dropout, uint64_t seed, float* mean, float* f,
                      float* init, int32_t N, int32_t L, int32_t D, int32_t m, int32_t n2, void* stream) {
    if (!ann || !w_f || !b_f || !w_i || !b_i || !mean || !f || !init) return fail(SAT_EINVAL, "init_lstm_fwd: null pointer");
    if (N < 1 || L < 1 || D < 1 || m < 1 || n2 < 2 || !(dropout >= 0.f && dropout < 1.f)) return fail(SAT_EINVAL, "init_lstm_fwd: bad shape / dropout");
    return init_lstm_fwd(ann, w_f, b_f, w_i, b_i, dropout, seed, mean, f, init, N, L, D, m, n2, (hipStream_t)stream);
}
int sat_init_lstm_bwd(const float* dinit, const float* mean, const float* f, const float* w_f, const float* w_i, float dropout, uint64_t seed, float* dw_f,
                      float* db_f, float* dw_i, float* db_i, float* dann, float* df, float* dmean, float* scratch, int32_t N, int32_t L, int32_t D, int32_t m,
                      int32_t n2, void* stream) {
    if (!dinit || !mean || !f || !w_f || !w_i || !dw_f || !db_f || !dw_i || !db_i || !dann || !df || !dmean || !scratch) return fail(SAT_EINVAL, "init_lstm_bwd: null pointer");
    if (N < 1 || L < 1 || D < 1 || m < 1 || n2 < 2 || !(dropout >= 0.f && dropout < 1.f)) return fail(SAT_EINVAL, "init_lstm_bwd: bad shape / dropout");
    return init_lstm_bwd(dinit, mean, f, w_f, w_i, dropout, seed, dw_f, db_f, dw_i, db_i, dann, df, dmean, scratch, N, L, D, m, n2, (hipStream_t)stream);
}

int sat_embedding_fwd(float* table, const int32_t* tokens, float* out, int32_t rows, int32_t V, int32_t m, float max_norm, int32_t* flags_scratch, void* stream) {
    if (!table || !tokens || !out || (max_norm > 0.f && !flags_scratch)) return fail(SAT_EINVAL, "embedding_fwd: null pointer");
    if (rows < 1 || V < 1 || m < 1) return fail(SAT_EINVAL, "embedding_fwd: bad shape");
    return embedding_fwd(table, tokens, out, rows, V, m, max_norm, flags_scratch, (hipStream_t)stream);
}
int sat_embedding_bwd(const float* dY, const int32_t* tokens, float* dtable, int32_t rows, int32_t V, int32_t m, int32_t padding_idx, int32_t* scratch, void* stream) {
    if (!dY || !tokens || !dtable || !scratch) return fail(SAT_EINVAL, "embedding_bwd: null pointer");
    if (rows < 1 || V < 1 || m < 1) return fail(SAT_EINVAL, "embedding_bwd: bad shape");
    return embedding_bwd(dY, tokens, dtable, rows, V, m, padding_idx, scratch, (hipStream_t)stream);
}
int sat_sigmoid_bwd(const float* dy, const float* y, float* dpre, int64_t n, void* stream) {
    if (!dy || !y || !dpre || n < 1) return fail(SAT_EINVAL, "sigmoid_bwd: null pointer / empty");
    return sigmoid_bwd(dy, y, dpre, n, (hipStream_t)stream);
}

}  // extern "C"
