// What decoder.hip (training, sub-module entry points) and decoder_search.hip (the caption searches) share: the GEMM wrapper with its
// precision flag, and the launchers of the decoder kernels (decoder_kernels.h, compiled into decoder.hip only) that both sides use.
#pragma once
#include "decoder.h"
#include "gemm.h"

namespace sat {

// 1: the GEMMs of this thread's call round their operands to bf16 (sat_decoder_dims.precision).  Every entry point sets it before its
// first product.  One definition, in decoder.hip.
extern thread_local int t_bf16_mfma;

inline int gemm(hipStream_t st, int amode, int bmode, const float* A, long lda, const float* B, long ldb, float* C, long ldc,
                int M, int N, int K, int acc = 0, int epi = EPI_NONE, const float* bias = nullptr, const int* a_rows = nullptr,
                const int* c_rows = nullptr, const float* e0 = nullptr, long lde0 = 0, int c0 = 0, int c1 = 0, float* slab = nullptr, long slab_elems = 0) {
    GemmArgs g;
    g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.amode = amode; g.bmode = bmode; g.accumulate = acc; g.epi = epi; g.bias = bias; g.a_rows = a_rows; g.c_rows = c_rows;
    g.e0 = e0; g.lde0 = lde0; g.c0 = c0; g.c1 = c1; g.slab = slab; g.slab_elems = slab_elems;
    g.bf16_mfma = t_bf16_mfma;
    return launch_gemm(g, st);
}

// The start-up every decoder shares, training forward and search alike (decoder.hip).
// Packed step weights in one launch: Wcat = [W_d ; W_beta ; W_hh] (A + D + 4n, n) with its bf16 copy (or NULL), bcat = [0 ; b_beta ;
// b_ih + b_hh]; then bup[l - 1] = b_ih + b_hh of every stacked layer l >= 1.  weight_drop_p > 0 (the train step only; the searches never
// pass it): the W_hh rows are written under the weight-drop mask of (seed, stream 3).
int pack_step_weights(const sat_decoder_dims& d, const sat_decoder_params& p, float* Wcat, __bf16* Wcat_b, float* bcat, float* bup, hipStream_t st,
                      float weight_drop_p = 0.f, unsigned long long seed = 0);
// Per image: U = ann * W_e^T (att_enc, hoisted out of the steps) and the annotation mean; with f != NULL also InitLSTM's two Linears
// on the `images` mean rows, f (images, m) and init_img (images, 2 * layers * n).
int image_begin(const sat_decoder_dims& d, const sat_decoder_params& p, const float* ann, int images, float* U, float* mean, float* f, float* init_img,
                hipStream_t st);
// The plain pair with every argument of its kernels (decoder.hip), for the entry points that run it on caller-supplied gates.
int lstm_cell_plain_fwd(float* gates, int g_ld, const float* gy, const float* c_prev, const float* h_prev, float* c_new, float* h_new, const int* lengths, int step,
                        int rows, int n, void* hb_new, hipStream_t st);
int lstm_cell_plain_bwd(const float* gates, int g_ld, const float* c_prev, const float* c_new, const float* dh_out, float* dh_carry, float* dc_carry, float* dgates,
                        int dg_ld, const int* lengths, int step, int rows, int n, void* dgb, hipStream_t st);
// The layer-norm parameters of one LSTM layer (sat_decoder_params.ln_*): gains / shifts of the four gates (4n) and of the cell (n).
struct LnCell { const float *gate_w, *gate_b, *cell_w, *cell_b; };
// The switch of the layer-normalised cell: the parameter struct carries the layer-norm tensors (the entry points refuse a mixture).
inline bool ln_on(const sat_decoder_params& p) { return p.ln_gate_w[0] != nullptr; }
inline LnCell ln_layer(const sat_decoder_params& p, int l) { return LnCell{p.ln_gate_w[l], p.ln_gate_b[l], p.ln_cell_w[l], p.ln_cell_b[l]}; }
// The pointwise LSTM cell on gates (rows, 4n; row stride g_ld) that hold every product already; rows with live[i] == 0 carry their state
// (live NULL: every row is live).  c_new / h_new may be c_prev / h_prev.  ln: the layer-normalised cell in the same single launch.
int lstm_cell_pointwise(float* gates, int g_ld, const float* c_prev, const float* h_prev, float* c_new, float* h_new, const int* live, int rows, int n,
                        hipStream_t st, const LnCell* ln = nullptr);
// The layer-normalised cell, one launch each (decoder_kernels.h: lstm_ln_cell_fwd_kernel / _bwd_kernel).  Forward: the contract of
// lstm_cell_fwd_kernel; xhat (rows, 5n) / rstd (rows, 5) are saved when not NULL.  Backward: the contract of lstm_cell_bwd_kernel; part
// (ln_slots(rows), 10n) or NULL receives the parameter-gradient partials (+=).
int ln_slots(int rows);
int lstm_ln_cell_fwd(float* gates, int g_ld, const float* gy, const float* c_prev, const float* h_prev, float* c_new, float* h_new, const int* lengths, int step,
                     int rows, int n, void* hb_new, const LnCell& ln, float* xhat, float* rstd, hipStream_t st);
int lstm_ln_cell_bwd(const float* gates, int g_ld, const float* c_prev, const float* xhat, const float* rstd, const float* dh_out, float* dh_carry, float* dc_carry,
                     float* dgates, int dg_ld, const int* lengths, int step, int rows, int n, void* dgb, const LnCell& ln, float* part, hipStream_t st);
// After the last backward launch: the sum over the slots, dgate_w / dgate_b (4n), dcell_w / dcell_b (n); scratch: 16n floats (four row blocks of 4n columns).
int ln_param_grads(const float* part, int slots, int n, float* dgate_w, float* dgate_b, float* dcell_w, float* dcell_b, float* scratch, hipStream_t st);

}  // namespace sat
