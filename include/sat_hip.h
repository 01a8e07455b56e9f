/* sat_hip.h -- C ABI of libsat_hip.so, the MI355X (gfx950) implementation of the
 * Show-Attend-and-Tell train-step hot path.
 *
 * The reference (Lukeasargen/Show-Attend-and-Tell-Pytorch-Lightning) is pure Python and
 * has no FFI: the boundary it offers is the Python surface of `class SAT`
 * (model.py:134) and its sub-modules.  Each entry point below replaces the stock
 * PyTorch ops behind one of those call sites (cited per function).  INTEGRATION.md
 * shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`;
 *   - fp32 tensors, int32 indices, row-major; Linear weights keep torch's (out,in)
 *     layout, conv weights are KRSC (torch channels_last memory), activations NHWC;
 *   - no allocation, no synchronisation, no ownership transfer: the caller provides
 *     outputs and a workspace (size from the *_workspace_bytes query) and a hipStream_t
 *     (passed as void*); calls are re-entrant per stream.  Stream capture (hipGraph): every entry point enqueues KERNEL
 *     launches only (clears and device-to-device copies are kernels too, csrc/devmem.hip), nothing reads host memory at
 *     execution time and nothing synchronises, so a captured stream is a chain of kernel nodes.  `_host` arrays
 *     (step_offsets_host, teacher_host) are read while ENQUEUEING: they shape the launch sequence, so a captured train step
 *     is valid for that packing plan and those teacher-forcing flags (sat_amd/graph.py keys its graphs by them).  Tested under
 *     capture + replay: sat_beam_search_batched / _sampled (tests/test_gpu_inference.py) and the whole train step - encoder,
 *     sat_decoder_train_fwd / _bwd, the losses, sat_optimizer_step_dev - bit-equal to the eager step (tests/test_gpu_graph.py),
 *     likewise with sat_optimizer_step_avg_dev as its last launch (averaged weights, tests/test_gpu_averaging.py);
 *   - return 0 on success, non-zero otherwise with text in sat_last_error()
 *     (thread-local).  Nothing throws, nothing exits.
 */
#ifndef SAT_HIP_H
#define SAT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAT_HIP_ABI_VERSION 23

int sat_abi_version(void);
/* dev aid: after every kernel launch wait for the device and print the launch's name to stderr (a device fault then points at the
 * launch after the last printed line).  Also switched on by SAT_TRACE_LAUNCH=1.  Not for captured streams. */
int sat_debug_trace_launches(int32_t on);
/* dev aid: tuning switches of the GEMM launcher by name ("glds_tile": force a tile form of csrc/gemm_glds.hip, -1 = automatic;
 * "glds_stages": LDS ring depth of every direct-to-LDS launch, 1 .. 4, 0 = automatic; "glds_stages8": the depth of its 8-wave forms; "tile_override": replace the launcher's own choice).  Not for production use. */
int sat_debug_option(const char* name, int32_t value);
const char* sat_last_error(void);

/* ------------------------------------------------------------------ kernel timing for the roofline report
 * Between start and stop every instrumented launch is bracketed by HIP events on its own stream; stop
 * synchronises them and returns one entry per kernel family (process-wide; measurement runs only). */
typedef struct sat_profile_entry {
    char name[96];
    int64_t launches;
    double total_ms;      /* sum of event-measured durations          */
    double flops;         /* algorithmic FLOPs of those launches       */
    double bytes;         /* algorithmic bytes of those launches       */
} sat_profile_entry;
int sat_profile_start(void);
/* the same, recording only the scopes of one family, or of every family with a common prefix when `name` ends in '*' */
int sat_profile_start_only(const char* name);
/* recording off (1) / on again (0) between start and stop, keeping what was recorded: bench.py instruments every n-th timed step */
int sat_profile_pause(int32_t paused);
int sat_profile_stop(sat_profile_entry* out, int32_t max_entries, int32_t* n_out);

/* ------------------------------------------------------------------ GEMM family
 * C[MxN] = op(A)[MxK] * op(B)[KxN] on v_mfma_f32_32x32x2_f32.  Replaces nn.Linear
 * (model.py:72-73, 90-92, 119-123, 188) and its autograd.  amode/bmode/epi: enum values
 * of csrc/gemm.h (0 = row-major k-contiguous, 1 = k-major). */
typedef struct sat_gemm_desc {
    const float* A; int64_t lda; const int32_t* a_rows; /* optional row gather, -1 = zero row */
    const float* B; int64_t ldb;
    float* C; int64_t ldc;       const int32_t* c_rows; /* optional row scatter, -1 = skip */
    int32_t M, N, K;
    int32_t amode, bmode;
    int32_t accumulate;          /* C += */
    int32_t epi;                 /* 0 none, 1 +bias, 2 +bias & sigmoid on cols [c0,c1), 3 tanh(v+e0), 4 v*(1-e0^2), 5 relu(v+bias) */
    const float* bias; const float* e0; int64_t lde0; int32_t c0, c1;
    float* slab; int64_t slab_elems;   /* optional split-K scratch */
} sat_gemm_desc;
int sat_gemm_f32(const sat_gemm_desc* d, void* stream);
/* Same contraction with explicit storage types and matrix-core choice: *_bf16 = operand stored as bf16 in HBM
 * (pointers in the descriptor are then reinterpreted), bf16_mfma = use v_mfma_f32_32x32x16_bf16 with fp32
 * accumulation (fp32 operands are rounded to bf16 on the way into LDS). */
typedef struct sat_gemm_types { int32_t a_bf16, b_bf16, c_bf16, bf16_mfma; } sat_gemm_types;
int sat_gemm_ex(const sat_gemm_desc* d, const sat_gemm_types* t, void* stream);

/* ------------------------------------------------------------------ decoder (train_batch, model.py:474-557) */
typedef struct sat_decoder_dims {
    int32_t B;            /* images in the batch                                   */
    int32_t R;            /* captions per image (lengths.size(1), model.py:487)    */
    int32_t T;            /* caption tensor width; T-1 decode steps                */
    int32_t L;            /* locations h*w                                         */
    int32_t D;            /* encoder_dim                                           */
    int32_t A;            /* attention_dim                                         */
    int32_t m;            /* embed_dim                                             */
    int32_t n;            /* decoder_dim                                           */
    int32_t V;            /* vocab_size                                            */
    int32_t P;            /* packed tokens = sum(lengths)                          */
    int32_t deep_output;  /* DeepOutput.deep (model.py:116)                        */
    int32_t padding_idx;  /* <PAD> id (model.py:162)                               */
    int32_t precision;    /* 0: exact fp32 MFMA (parity mode); 1: bf16 MFMA, fp32 accumulate/state */
    int32_t layers;       /* nn.LSTM num_layers (model.py:178), 1..SAT_MAX_LSTM_LAYERS; h/c are (layers, N, n) */
    float embed_max_norm; /* nn.Embedding max_norm (model.py:161); <= 0: off.  Renormalises embedding rows IN PLACE */
    float dropout;        /* nn.Dropout p of InitLSTM / DeepOutput (model.py:74,117) in training mode; 0: off     */
    float embedding_dropout; /* p of embedding_dropout (model.py:164); 0: off                                    */
    uint64_t dropout_seed;   /* masks = counter-based hash of (seed, stream, element): same seed for fwd and bwd */
    float weight_drop;       /* train step only: DropConnect p on every lstm.weight_hh_l{l}, one mask per call (stream 3); 0: off */
    int32_t variational_dropout; /* train step only: 1 = the embedding / DeepOutput masks keep one row per caption for all time steps */
} sat_decoder_dims;

/* state-dict tensors of the decoder; used for weights and, with the same
 * field meaning, for gradient outputs. */
#define SAT_MAX_LSTM_LAYERS 4
typedef struct sat_decoder_params {
    float* embedding;                 /* embedding.weight            (V, m)      */
    float* init_f_w; float* init_f_b; /* init_lstm.factorize         (m, D), (m) */
    float* init_i_w; float* init_i_b; /* init_lstm.init              (2n*layers, m), (2n*layers) */
    float* w_ih; float* w_hh;         /* lstm.weight_ih_l0 (4n, m+D), lstm.weight_hh_l0 (4n, n) */
    float* b_ih; float* b_hh;         /* lstm.bias_ih_l0, lstm.bias_hh_l0 (4n)   */
    float* att_enc;                   /* attention.encoder_att.weight (A, D)     */
    float* att_dec;                   /* attention.decoder_att.weight (A, n)     */
    float* att_f;                     /* attention.f_att.weight       (1, A)     */
    float* beta_w; float* beta_b;     /* beta.0                       (D, n), (D) */
    float* out_hidden;                /* output.hidden.weight         (m, n)     */
    float* out_context;               /* output.context.weight        (m, D), NULL when shallow */
    float* out_w; float* out_b;       /* output.output (V, m), (V); out_b NULL under weight tying */
    /* stacked layers l = 1 .. layers-1 at index l-1: lstm.weight_ih_l{l} (4n, n), weight_hh_l{l} (4n, n), bias_ih_l{l}, bias_hh_l{l} (4n) */
    float* up_w_ih[SAT_MAX_LSTM_LAYERS - 1]; float* up_w_hh[SAT_MAX_LSTM_LAYERS - 1];
    float* up_b_ih[SAT_MAX_LSTM_LAYERS - 1]; float* up_b_hh[SAT_MAX_LSTM_LAYERS - 1];
    /* layer-normalised LSTM cell (lstm_layer_norm; see "layer-normalised LSTM cell" below), one entry per layer l = 0 .. layers-1:
     * lstm_ln.gates_l{l}.weight / .bias (4n), lstm_ln.cell_l{l}.weight / .bias (n).  These are the switch: all NULL (a zero-initialised
     * struct) = the plain cell; all non-NULL for l < layers = the normalised cell; a mixture is refused. */
    float* ln_gate_w[SAT_MAX_LSTM_LAYERS]; float* ln_gate_b[SAT_MAX_LSTM_LAYERS];
    float* ln_cell_w[SAT_MAX_LSTM_LAYERS]; float* ln_cell_b[SAT_MAX_LSTM_LAYERS];
} sat_decoder_params;

typedef struct sat_decoder_batch {
    const float* ann;            /* (B, L, D) annotations = encoder output, NHWC flattened          */
    const int32_t* caps;         /* (B*R, T) encoded captions                                        */
    const int32_t* lengths;      /* (B*R)                                                            */
    const int32_t* prow;         /* (T-1, B*R) packed row of (step, caption) or -1 when finished    */
    const int32_t* src_row;      /* (P) step*N + caption of packed row p                             */
    const int32_t* step_offsets_host; /* HOST (T) : first packed row of each step, [T-1] = P         */
    const int32_t* teacher_host;      /* HOST (T-1): 1 = feed the caption token, 0 = argmax of the
                                         previous step's logits (scheduled sampling, model.py:518-523) */
} sat_decoder_batch;

size_t sat_decoder_workspace_bytes(const sat_decoder_dims* d);

/* train_batch decoder forward (model.py:487-548): writes logits in packed order
 * (pack_padded_sequence(...).data order, model.py:553) and alphas (N, T-1, L). */
int sat_decoder_train_fwd(const sat_decoder_dims* d, const sat_decoder_params* w, const sat_decoder_batch* b,
                          float* logits_packed, float* alphas, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the above through time (what autograd does for loss.backward()).
 * dlogits_packed (P, V); dalphas (N, T-1, L) or NULL.  Overwrites every field of `g`
 * and dann (B, L, D).  Must follow a forward on the same workspace. */
int sat_decoder_train_bwd(const sat_decoder_dims* d, const sat_decoder_params* w, const sat_decoder_batch* b,
                          const float* dlogits_packed, const float* alphas /* forward output */, const float* dalphas,
                          const sat_decoder_params* g, float* dann, void* workspace, size_t workspace_bytes, void* stream);

/* The same backward with the parameter gradients on a second stream.  Only dann lies on the way to the encoder backward; every field of `g`
 * feeds the optimizer alone.  With `side_stream` and `event` (a hipStream_t and a hipEvent_t, both or neither) the launches that lead to dann
 * are issued first on `stream`; `event` is recorded on `stream` behind the last kernel whose output a parameter gradient reads, `side_stream`
 * waits for it once, and every launch that writes into `g` goes to `side_stream`, with a split-K / column-sum scratch of its own inside the
 * workspace.  The call returns WITHOUT joining: dann is ordered on `stream`; the caller makes `stream` wait for `side_stream` before anything
 * reads `g`, and keeps dlogits_packed, the annotations and the workspace alive until then.  With both NULL this is sat_decoder_train_bwd. */
int sat_decoder_train_bwd_fork(const sat_decoder_dims* d, const sat_decoder_params* w, const sat_decoder_batch* b,
                               const float* dlogits_packed, const float* alphas, const float* dalphas, const sat_decoder_params* g,
                               float* dann, void* workspace, size_t workspace_bytes, void* side_stream, void* event, void* stream);

/* ------------------------------------------------------------------ losses
 * LabelSmoothing.forward (util.py:105-112) over packed rows.  out[0] = loss, out[1] = accuracy
 * (model.py:596-597).  scratch: P floats lse + P floats loss + P ints. */
int sat_ce_label_smooth_fwd(const float* logits, const int32_t* targets, int32_t P, int32_t V, float smoothing,
                            float* lse_rows, float* loss_rows, int32_t* correct_rows, float* out, void* stream);
/* dlogits = gscale[0] * d loss / d logits  (gscale device pointer or NULL = 1) */
int sat_ce_label_smooth_bwd(const float* logits, const int32_t* targets, const float* lse_rows, int32_t P, int32_t V,
                            float smoothing, const float* gscale, float* dlogits, void* stream);
/* model.py:594: out[0] = gamma * mean((1 - sum_t alphas)^2); asum (N, L) kept for backward;
 * part: ceil(N*L/256) floats scratch. */
int sat_doubly_stochastic_fwd(const float* alphas, int32_t N, int32_t T1, int32_t L, float gamma,
                              float* asum, float* part, float* out, void* stream);
int sat_doubly_stochastic_bwd(const float* asum, const float* gscale, int32_t N, int32_t T1, int32_t L, float gamma,
                              float* dalphas, void* stream);

/* ------------------------------------------------------------------ activation regularisation (Merity et al. 2017: AR / TAR)
 * hidden (T1, N, n), time-major: hidden[t][i] = top-layer LSTM state of caption i after decode step t; live while t < lengths[i].  Rows
 * that are not live are never read (they may hold anything) and never written.  With P = sum_i lengths[i] and
 * Q = sum_i max(lengths[i] - 1, 0) (both given by the caller; 0 <= Q <= P <= N * T1):
 *   out[0] = ar  = 1/(P n) sum_{live (t,i)}        |hidden[t][i]|^2                      (0 when P = 0)
 *   out[1] = tar = 1/(Q n) sum_{live (t,i), t >= 1} |hidden[t][i] - hidden[t-1][i]|^2     (0 when Q = 0)
 * Equal lengths: h.pow(2).mean() and (h[1:] - h[:-1]).pow(2).mean().  Squares and differences in fp32, sums in double in a fixed order
 * (no atomics): bit-reproducible.  scratch: sat_activation_reg_scratch_bytes(N, T1, n) bytes, 8-byte aligned.
 * _bwd ADDS gscale[0] * d ar / d hidden + gscale[1] * d tar / d hidden into the live rows of dH (T1, N, n); gscale: device, 2 floats.
 * Every other element of dH keeps its bits. */
size_t sat_activation_reg_scratch_bytes(int32_t N, int32_t T1, int32_t n);
int sat_activation_reg_fwd(const float* hidden, const int32_t* lengths, int32_t N, int32_t T1, int32_t n, int64_t P, int64_t Q,
                           void* scratch, float* out, void* stream);
int sat_activation_reg_bwd(const float* hidden, const int32_t* lengths, int32_t N, int32_t T1, int32_t n, int64_t P, int64_t Q,
                           const float* gscale, float* dH, void* stream);
/* After sat_decoder_train_fwd on the same workspace: out (device, 2 floats) = ar / tar of that forward's top-layer states; P and Q
 * come from d and b.step_offsets_host.  scratch: sat_activation_reg_scratch_bytes(B * R, T - 1, n) bytes. */
int sat_decoder_train_reg_fwd(const sat_decoder_dims* d, const sat_decoder_batch* b, void* workspace, size_t workspace_bytes,
                              void* scratch, float* out, void* stream);
/* sat_decoder_train_bwd_fork plus reg_gscale (device, 2 floats: d loss / d ar, d loss / d tar) or NULL.  Given, the regularisers'
 * direct gradient is added into the output layer's gradient of the top-layer states on `stream`, in front of the time loop, which
 * carries it like any other; the parameter gradients on the side stream do not read it.  NULL: exactly sat_decoder_train_bwd_fork. */
int sat_decoder_train_bwd_reg(const sat_decoder_dims* d, const sat_decoder_params* w, const sat_decoder_batch* b,
                              const float* dlogits_packed, const float* alphas, const float* dalphas, const sat_decoder_params* g,
                              float* dann, void* workspace, size_t workspace_bytes, void* side_stream, void* event, void* stream,
                              const float* reg_gscale);

/* ------------------------------------------------------------------ weight-drop (Merity et al. 2017; Wan et al. 2013: DropConnect)
 * The mask of the decoder train step's weight_drop on its own: for w (layers, rows, cols), element (l, r, c) has the scale
 *   s = 0 or 1 / (1 - p), the counter hash of (seed, stream 3, index (l * rows + r) * cols + c)
 * (the decoder: rows = 4n, cols = n, l = the LSTM layer).  0 <= p < 1; 1 <= layers <= SAT_MAX_LSTM_LAYERS.
 * sat_weight_drop writes out_f32 = w * s and, when out_bf16 is not NULL, the bf16 rounding of the same fp32 product; out_f32 may be w.
 * sat_weight_drop_grad multiplies g by s in place: the gradient with respect to w from the gradient with respect to w * s.
 * sat_decoder_pack_weights: the packing launch of the train step on its own -- wcat (A + D + 4n, n) = [W_d ; W_beta ; W_hh * s(layer 0)]
 * with d->weight_drop and d->dropout_seed (0: the plain pack), its bf16 copy (or NULL), bcat (A + D + 4n). */
int sat_weight_drop(const float* w, float* out_f32, void* out_bf16, int32_t layers, int32_t rows, int32_t cols, float p, uint64_t seed, void* stream);
int sat_weight_drop_grad(float* g, int32_t layers, int32_t rows, int32_t cols, float p, uint64_t seed, void* stream);
int sat_decoder_pack_weights(const sat_decoder_dims* d, const sat_decoder_params* w, float* wcat, void* wcat_bf16, float* bcat, void* stream);

/* ------------------------------------------------------------------ layer-normalised LSTM cell (Ba et al. 2016)
 * With the pre-activation a = x W_ih^T + b_ih + h W_hh^T + b_hh (gate order i, f, g, o; width 4n) summed exactly as for the plain cell:
 *   a^_k = LN(a_k; gamma_k, beta_k) over the n units of gate k;  i, f, o = sigmoid(a^), g = tanh(a^_g)
 *   c_t = f c_{t-1} + i g (carried un-normalised);  h_t = o tanh(LN(c_t; gamma_c, beta_c))
 * LN = layer_norm with biased variance and eps = 1e-5 (a constant of the library).  Every decoder entry point (train forward / backward,
 * the searches, the infer step) runs this cell, still one launch per cell and step, when sat_decoder_params carries the ln_* tensors.
 * The train step then needs a larger workspace: sat_decoder_workspace_bytes_ln (w NULL or without ln_*: sat_decoder_workspace_bytes).
 * The searches' workspaces do not change.
 *
 * The two launches on caller-supplied gates:
 * sat_lstm_ln_cell_fwd: gates (rows, 4n; row stride g_ld >= 4n) hold a, gy (rows, 4n) or NULL is added to it; rows with live[i] <= 0 carry
 *   h and c and get zero gates (live NULL: all live); activated gates are written back in place; c_new / h_new may be c_prev / h_prev;
 *   h_bf16 (rows, n) or NULL: bf16 copy of h_new; xhat (rows, 5n) = [x^_i x^_f x^_g x^_o c^] and rstd (rows, 5) or both NULL: what the
 *   backward needs (live rows only).
 * sat_lstm_ln_cell_bwd: dh_carry / dc_carry (rows, n) are read and updated as by the plain cell (dc_carry <- dc f, dh_carry <- 0 on live
 *   rows); dh_out (rows, n) or NULL joins dh_carry; dgates (rows, 4n; stride dg_ld) = gradient of the PRE-NORM sum a, zero on dead rows;
 *   dgates_bf16: copy with the same stride, or NULL.  part (sat_lstm_ln_slots(rows), 10n) or NULL: each block ADDS its rows' partial sums
 *   [dgamma_gates 4n | dbeta_gates 4n | dgamma_cell n | dbeta_cell n] into its own slot (zero it before the first step; no atomics).
 * sat_lstm_ln_param_grads: the sum over the slots in slot order into the four gradients; scratch: 16n floats.  Bit-reproducible. */
/* The plain cell's pointwise pair on caller-supplied gates, with the arguments of the two launches above that it shares (c_new: the forward's
 * output, read by the backward): what the time loops launch without the norm.  tools/bench_lstm_layer_norm.py times the two pairs side by side. */
int sat_lstm_cell_pointwise_fwd(float* gates, int32_t g_ld, const float* gy, const float* c_prev, const float* h_prev, float* c_new, float* h_new,
                                const int32_t* live, void* h_bf16, int32_t rows, int32_t n, void* stream);
int sat_lstm_cell_pointwise_bwd(const float* gates, int32_t g_ld, const float* c_prev, const float* c_new, const float* dh_out, float* dh_carry,
                                float* dc_carry, float* dgates, int32_t dg_ld, const int32_t* live, void* dgates_bf16, int32_t rows, int32_t n,
                                void* stream);
size_t sat_decoder_workspace_bytes_ln(const sat_decoder_dims* d, const sat_decoder_params* w);
int32_t sat_lstm_ln_slots(int32_t rows);
int sat_lstm_ln_cell_fwd(float* gates, int32_t g_ld, const float* gy, const float* c_prev, const float* h_prev, float* c_new, float* h_new,
                         const int32_t* live, void* h_bf16, const float* ln_gate_w, const float* ln_gate_b, const float* ln_cell_w,
                         const float* ln_cell_b, float* xhat, float* rstd, int32_t rows, int32_t n, void* stream);
int sat_lstm_ln_cell_bwd(const float* gates, int32_t g_ld, const float* c_prev, const float* xhat, const float* rstd, const float* dh_out,
                         float* dh_carry, float* dc_carry, float* dgates, int32_t dg_ld, const int32_t* live, void* dgates_bf16,
                         const float* ln_gate_w, const float* ln_cell_w, const float* ln_cell_b, float* part, int32_t rows, int32_t n,
                         void* stream);
int sat_lstm_ln_param_grads(const float* part, int32_t slots, int32_t n, float* d_gate_w, float* d_gate_b, float* d_cell_w, float* d_cell_b,
                            float* scratch, void* stream);

/* ------------------------------------------------------------------ policy-gradient loss (self-critical sequence training; Rennie et al. 2017)
 * The REINFORCE surrogate over packed logits (P, V): every packed row p is one sampled action (targets[p]) with a weight of its own
 * (row_weight[p], the advantage of the caption it belongs to; any sign, 0 allowed).  The distribution differentiated is the one
 * SAT_SAMPLE_ANCESTRAL draws from: the softmax at the search's temperature over the words the search leaves unmasked.
 * masked_ids is a DEVICE array of 4 ids {START, PAD, END, UNK}: the first n_first_rows rows (the rows of decode step 0: packed rows are
 * time-major) mask all four, the other rows the first two.  An id outside [0, V) masks nothing.  With x = logits[p] * inv_temperature
 * and U the unmasked ids of the row:
 *   lse_rows[p]  = logsumexp over v in U of x[v]
 *   logq_rows[p] = x[targets[p]] - lse_rows[p]                 (NaN when the target is outside [0, V) or masked in its row; never a stray read)
 *   out[0]       = -scale * sum over the rows with row_weight != 0 of row_weight[p] * logq_rows[p]
 * The row terms are summed in double in a fixed order without atomics: the same input gives the same bits.  The forward reads every
 * row once (logq_rows is written for the rows of weight zero too); a row of weight zero adds exactly 0 to the loss whatever it holds.
 * Backward: dlogits[p][v] = gscale[0] * scale * row_weight[p] * inv_temperature * (softmax_U(x)[v] - [v == targets[p]]) for v in U and
 * exactly 0 for masked v; a row of weight zero is written as zeros and its logits are not read.  gscale: device pointer or NULL = 1.
 * One 256-thread block per row; 16-byte loads and stores when V % 4 == 0 and logits (and dlogits) are 16-byte aligned, 4-byte ones
 * otherwise.  SAT_EINVAL before any launch: a null pointer, P <= 0, V <= 0, n_first_rows outside [0, P], an inv_temperature that is
 * not a positive finite number, a non-finite scale.  scratch: lse_rows, logq_rows P floats each. */
int sat_policy_nll_fwd(const float* logits, const int32_t* targets, const float* row_weight, int32_t P, int32_t V, float inv_temperature,
                       const int32_t* masked_ids, int32_t n_first_rows, float scale, float* lse_rows, float* logq_rows, float* out, void* stream);
int sat_policy_nll_bwd(const float* logits, const int32_t* targets, const float* row_weight, const float* lse_rows, int32_t P, int32_t V,
                       float inv_temperature, const int32_t* masked_ids, int32_t n_first_rows, float scale, const float* gscale, float* dlogits,
                       void* stream);
/* From the scores of sampled captions to the train batch of the policy loss, one launch, one block per image, no host read.
 *   cap_tokens (N, S + 1), cap_len (N): sat_beam_select's output for N = B * K rows, image b owning rows b * K .. b * K + K - 1
 *   scores (N, 2) float64: sat_caption_consensus's [CIDEr-D, ROUGE-L]; scores_greedy (B, 2): the same for the image's greedy caption
 *   reward[n]    = w_cider * cider + w_rouge * rouge
 *   baseline[n]  = SAT_SCST_BASELINE_GREEDY: the image's greedy reward; SAT_SCST_BASELINE_MEAN: the mean reward of the image's other
 *                  K - 1 samples, summed in ascending order (needs K >= 2)                     (optional output: NULL skips it)
 *   advantage[n] = reward[n] - baseline[n], in double up to the final float
 *   caps (N, S + 2) int32 = START, w_1 .. w_len, END, PAD ...;  lengths[n] = len + 1, the decode steps (the dataset's convention)
 *   step_weight (N, S + 1): advantage[n] for the steps 0 .. len - 1 and for the END step len when len < S, else 0.  A caption of S
 *                words was cut by the search: the word drawn at its last step is dropped, that draw cannot change the reward, and
 *                its step carries no gradient.
 *   count[n]     = len + (len < S): the steps the mask keeps
 * len = cap_len[n] clamped to [1, S] before it addresses anything.  special_ids_host {START, PAD, END, UNK} is a HOST array.
 * SAT_EINVAL before the launch: a null pointer, B / K / S < 1, K > SAT_SCST_MAX_SAMPLES, S + 1 > SAT_CAPTION_MAX_LEN, an unknown
 * mode, the greedy baseline without scores_greedy, the mean baseline with K < 2, a non-finite reward weight. */
#define SAT_SCST_BASELINE_GREEDY 0
#define SAT_SCST_BASELINE_MEAN 1
#define SAT_SCST_MAX_SAMPLES 256
int sat_scst_prepare(const int32_t* cap_tokens, const int32_t* cap_len, const double* scores, const double* scores_greedy /* or NULL */, int32_t B,
                     int32_t K, int32_t S, double w_cider, double w_rouge, int32_t baseline_mode, const int32_t* special_ids_host, float* reward,
                     float* baseline /* or NULL */, float* advantage, int32_t* caps, int32_t* lengths, float* step_weight, int32_t* count,
                     void* stream);

/* ------------------------------------------------------------------ distillation loss (Hinton et al. 2015; DESIGN.md 5, "Distillation")
 * Word-level knowledge distillation of M teachers into one student over packed rows.  logits z (P, V): the student's; teachers: a HOST
 * array of `members` device pointers t_i (P, V); weights: a HOST array, >= 0, summing to 1 within 1e-5; combine: SAT_ENSEMBLE_*;
 * targets y (P); inv_tau = 1 / tau > 0, the distillation temperature of student and teachers alike; alpha in [0, 1]; smoothing in
 * [0, 1).  Per row p, with l_i = log_softmax(t_i[p] * inv_tau):
 *   c      = the combination of the l_i exactly as sat_beam_search_ensemble defines it (mixture or product; members of weight 0 are
 *            skipped and their logits are not read)
 *   log q  = log_softmax(c),   s = log_softmax(z[p] * inv_tau)
 *   soft_p = sum_v q_v (log q_v - s_v) = KL(q || softmax(z[p] * inv_tau)); a word with q_v == 0 adds exactly 0, so finite logits give a
 *            finite loss and gradient however peaked a teacher is
 *   hard_p = the row loss of sat_ce_label_smooth_fwd on z[p], y[p], smoothing (NaN for a target outside [0, V): never a stray read);
 *            the correct-prediction flag is that entry point's too
 *   out[0] = (1 - alpha) mean_p hard_p + alpha tau^2 mean_p soft_p;  out[1] = mean_p hard_p;  out[2] = mean_p soft_p;  out[3] = accuracy
 *   dlogits[p][v] = gscale[0] / P * [ (1 - alpha) (softmax(z[p])_v - h_v) + alpha tau (softmax(z[p] * inv_tau)_v - q_v) ], h the smoothed
 *            target distribution of sat_ce_label_smooth_bwd (a target outside [0, V) leaves its one-hot out)
 * alpha == 0: the teachers are not read, soft rows and out[2] are 0.  alpha == 1: the hard term is skipped, hard rows and out[1] are 0
 * (accuracy is still reported).  The row terms are summed in double in a fixed order without atomics: the same input gives the same bits.
 * Row scratch, written by the forward and read by the backward so that no reduction is redone: lse_rows (P, 2) = logsumexp(z[p]),
 * logsumexp(z[p] * inv_tau); teacher_lse_rows (P, members) = logsumexp(t_i[p] * inv_tau) (0 for a member that is not read);
 * cnorm_rows (P) = logsumexp(c); loss_rows (P, 2) = hard_p, soft_p; correct_rows (P).
 * sat_distill_fwd with dlogits != NULL also writes the gradient for gscale = 1 in the same launch (the rows are still in the cache);
 * sat_distill_bwd with dlogits_from_fwd != 0 is then the in-place scale by gscale[0] and nothing more (gscale == NULL: no launch).
 * With dlogits_from_fwd == 0 it produces dlogits from the logits and the scratch.  gscale: device pointer or NULL = 1.
 * One 256-thread block per row; 16-byte accesses when V % 4 == 0 and the student's, every read teacher's and the gradient's pointer are
 * 16-byte aligned, 4-byte ones otherwise.  SAT_EINVAL before any launch: a null pointer (a teacher's included), P, V or members < 1,
 * members > SAT_ENSEMBLE_MAX, a weight that is negative or not finite, weights that do not sum to 1 within 1e-5, an unknown combine,
 * an inv_tau that is not a positive finite number, alpha outside [0, 1], smoothing outside [0, 1). */
int sat_distill_fwd(const float* logits, const float* const* teachers, const float* weights, int32_t members, int32_t combine, const int32_t* targets,
                    int32_t P, int32_t V, float inv_tau, float alpha, float smoothing, float* lse_rows, float* teacher_lse_rows, float* cnorm_rows,
                    float* loss_rows, int32_t* correct_rows, float* out, float* dlogits /* or NULL */, void* stream);
int sat_distill_bwd(const float* logits, const float* const* teachers, const float* weights, int32_t members, int32_t combine, const int32_t* targets,
                    int32_t P, int32_t V, float inv_tau, float alpha, float smoothing, const float* lse_rows, const float* teacher_lse_rows,
                    const float* cnorm_rows, const float* gscale, int32_t dlogits_from_fwd, float* dlogits, void* stream);

/* ------------------------------------------------------------------ token losses ("Token losses")
 * The label-smoothed cross entropy, focal loss (Lin et al. 2017) and token-level unlikelihood (Welleck et al. 2019) over packed logits
 * (P, V) in one pass.  Per row p, with x = logits[p], y = targets[p], lse = logsumexp(x), p_v = exp(x_v - lse), q = p_y:
 *   ce_p   = the row loss of sat_ce_label_smooth_fwd on x, y, smoothing (NaN for y outside [0, V): never a stray read)
 *   fl_p   = (1 - q)^gamma (lse - x_y): the unsmoothed negative log-likelihood times the focal factor; gamma == 0: the plain one
 *   C_p    = the negative candidates.  context (N, T) int32: the captions as sat_decoder_train_fwd takes them; src_row (P):
 *            src_row[p] = t * N + i (the packing plan's): row p is decode step t of caption i.  C_p = the DISTINCT ids among
 *            context[i][1 .. t] (the targets of the steps 0 .. t - 1) that are != y, != pad_id (-1: none) and inside [0, V).  A
 *            src_row[p] outside [0, (T - 1) N) gives the row a NaN ul_p and nothing is read through it.
 *   ul_p   = - sum_{c in C_p} log(max(1 - p_c, 1e-5)), 1 - p_c taken as -expm1(x_c - lse);   mass_p = sum_{c in C_p} p_c
 *   out[0] = mean_p (ce_weight ce_p + focal_weight fl_p + ul_alpha ul_p);  out[1] = accuracy (sat_ce_label_smooth_fwd's);
 *   out[2..5] = the means of ce_p, fl_p, ul_p, mass_p
 *   dlogits[p][v] = gscale[0] / P * [ ce_weight (p_v - smoothing/V - (1 - smoothing) [v == y]) + focal_weight w_p (p_v - [v == y])
 *                                     + ul_alpha ([v in C_p] r_v - p_v R_p) ]
 *            w_p = (1 - q)^gamma - gamma q (1 - q)^(gamma - 1) log q   (1 at gamma == 0; 0 at q == 1 with gamma > 0)
 *            r_c = p_c / (1 - p_c) where 1 - p_c >= 1e-5, else 0 (the clamp passes no gradient);  R_p = sum_{c in C_p} r_c
 * A weight of zero skips its term: its rows and its mean are 0 and nothing is read for it; with ul_alpha == 0 context and src_row are
 * not read and may be NULL.  With ce_weight 1 and the other two 0, out[0..1], lse_rows and dlogits are sat_ce_label_smooth_fwd / _bwd's
 * bit for bit (one device code).  The row terms are summed in double in a fixed order without atomics: the same input gives the same bits.
 * Row scratch, written by the forward and read by the backward so that no reduction is redone: lse_rows (P); aux_rows (P, 2) = w_p, R_p;
 * loss_rows (P, 4) = ce_p, fl_p, ul_p, mass_p; correct_rows (P).  gscale: device pointer or NULL = 1.
 * One 256-thread block per row, one thread per context id; 16-byte accesses when V % 4 == 0 and logits (and dlogits) are 16-byte
 * aligned, 4-byte ones otherwise.  No (P, V) mask or temporary: the sweeps never ask whether a word is a candidate, the backward writes
 * the target's and the candidates' entries whole behind its sweep.  SAT_EINVAL before any launch: a null pointer (context / src_row
 * only with ul_alpha != 0), P or V < 1, smoothing outside [0, 1), a weight, gamma or alpha that is negative or not finite, all three
 * weights zero, and with ul_alpha != 0: N < 1, T < 2 or T - 1 > 256. */
int sat_token_loss_fwd(const float* logits, const int32_t* targets, int32_t P, int32_t V, float smoothing, float ce_weight, float focal_weight,
                       float focal_gamma, float ul_alpha, const int32_t* context, const int32_t* src_row, int32_t N, int32_t T,
                       int32_t pad_id /* -1: none */, float* lse_rows, float* aux_rows, float* loss_rows, int32_t* correct_rows, float* out /* 6 floats */,
                       void* stream);
int sat_token_loss_bwd(const float* logits, const int32_t* targets, int32_t P, int32_t V, float smoothing, float ce_weight, float focal_weight,
                       float focal_gamma, float ul_alpha, const int32_t* context, const int32_t* src_row, int32_t N, int32_t T, int32_t pad_id,
                       const float* lse_rows, const float* aux_rows, const float* gscale /* or NULL = 1 */, float* dlogits, void* stream);

/* ------------------------------------------------------------------ temperature-scaling calibration (temperature_scaling.py:51-59)
 * For packed logits (P, V) and targets (P):  loss(T) = F.cross_entropy(logits / T, targets)  and its derivative
 * dloss/dT = mean_i [ x_iy - sum_j softmax(x_i / T)_j x_ij ] / T^2.  The row maximum does not depend on T > 0, so it is taken once;
 * each evaluation is then ONE streaming read of the logits and writes nothing of size P*V.  Reductions run in a fixed order in
 * double (no atomics): the same input gives the same bits.  A target outside [0, V) or a non-finite logit gives NaN, never an
 * out-of-bounds read.  workspace: sat_temperature_workspace_bytes(P, V) bytes, 16-byte aligned; 0 + message for non-positive sizes. */
#define SAT_TEMPERATURE_MAX 8
size_t sat_temperature_workspace_bytes(int32_t P, int32_t V);
/* loss_out[t], grad_out[t] at temperatures[t] (device array, every one > 0), t < n_temperatures <= SAT_TEMPERATURE_MAX, all from the
 * same read of the logits; n temperatures in one call equal n single calls bit for bit. */
int sat_temperature_nll(const float* logits, const int32_t* targets, int32_t P, int32_t V, const float* temperatures,
                        int32_t n_temperatures, float* loss_out, float* grad_out, void* workspace, void* stream);
/* `iters` steps of torch.optim.SGD(lr, momentum, nesterov) on the scalar T from `init`, in fp32 as the reference's tensor: first step
 * buf = g, then buf = momentum * buf + g; step = g + momentum * buf (nesterov) or buf; T -= lr * step.  T never visits the host:
 * t_trace (iters + 1 floats, t_trace[0] = init) and loss_trace (iters floats, the loss at t_trace[k]) are device arrays.  If T
 * becomes non-positive or non-finite at step k, t_trace[k + 1] holds that value, T is left alone from then on (t_trace repeats
 * it) and the later loss_trace entries are NaN. */
int sat_temperature_fit(const float* logits, const int32_t* targets, int32_t P, int32_t V, float init, float lr, float momentum,
                        int32_t nesterov, int32_t iters, float* t_trace, float* loss_trace, void* workspace, void* stream);

/* ------------------------------------------------------------------ inference: SAT.forward / caption (model.py:214-472)
 * The reference decodes one image at a time with the beam as the batch (model.py:260-266).  `begin` computes att_enc
 * and the initial state of `beams` rows (InitLSTM over the expanded annotations, F3 reshape: model.py:265-269);
 * `step` is one pass of model.py:298-327 for the live beams (h, c updated in place; d->B/R/T/P are ignored);
 * `sat_beam_scores` = log_softmax(logit / temperature) with the special tokens masked and the parent scores added
 * (model.py:330-351); `sat_topk` = torch.topk on the flattened scores (model.py:343, 359). */
size_t sat_decoder_infer_workspace_bytes(const sat_decoder_dims* d, int32_t max_beams);
int sat_decoder_infer_begin(const sat_decoder_dims* d, const sat_decoder_params* w, const float* ann /* (L, D) */, int32_t beams,
                            int32_t max_beams, float* h /* (layers, beams, n) */, float* c, void* workspace, size_t workspace_bytes, void* stream);
int sat_decoder_infer_step(const sat_decoder_dims* d, const sat_decoder_params* w, const float* ann, const int32_t* tokens, int32_t beams,
                           int32_t max_beams, float* h, float* c, float* logits /* (beams, V) */, float* alpha /* (beams, L) */,
                           const float* h_noise /* (layers, beams, n) or NULL: decoder_noise (model.py:322-324), added to h for the
                                                   LSTM update only; attention and the beta gate see the clean h[-1] */,
                           void* workspace, size_t workspace_bytes, void* stream);
/* Batched beam search ("beam" sampling, model.py:260-448 for every image of the batch at once; d->B = images, rows are (B, beamk)).
 * Enqueues max_gen_length + 1 decode steps without a host round trip and leaves the back-trace on the device:
 *   tok_in   (max_gen_length + 2, B, beamk)  token fed to each live row of each step ([0] = START)
 *   prev_row (max_gen_length + 2, B, beamk)  row of the previous step the hypothesis came from
 *   alpha_hist (max_gen_length + 1, B, beamk, L)  attention weights of each step's rows
 *   fin_*    (B, beamk)  finished hypotheses in the reference's append order: step at which they ended, the row they came from, raw score,
 *            mean beam score at that moment (for "BAR" rescoring); fin_count (B)
 * temperatures and special ids {START, PAD, END, UNK} are HOST arrays (read while enqueueing).
 * This entry point and the six sat_beam_search_* below it are adapters over sat_beam_search (further down), kept for existing callers. */
size_t sat_beam_search_workspace_bytes(const sat_decoder_dims* d, int32_t beamk);
int sat_beam_search_batched(const sat_decoder_dims* d, const sat_decoder_params* w, const float* ann /* (B, L, D) */, int32_t beamk,
                            int32_t max_gen_length, const float* temperatures_host, int32_t n_temperatures, const int32_t* special_ids_host,
                            int32_t* tok_in, int32_t* prev_row, float* alpha_hist, int32_t* fin_count, int32_t* fin_step, int32_t* fin_row,
                            float* fin_score, float* fin_mean, void* workspace, size_t workspace_bytes, void* stream);
/* The same search with the continuing hypotheses DRAWN instead of taken (SAT.forward sample_method, model.py:360-379) and / or
 * decoder noise (model.py:322-324).  torch.multinomial(p, k) without replacement is an ordered Plackett-Luce sample; it is drawn
 * here as the top k of log p + Gumbel noise.  The variates come from a counter-based hash of (seed, step, row, candidate) or
 * from the caller's tables (tests):
 *   gumbel  : method 1: (max_gen_length + 1, B * beamk, V)            Gumbel(0, 1) variate of candidate word v of a row
 *             method 2: (max_gen_length + 1, B * beamk, sample_topk)  ... of the row's t-th best candidate (torch.topk order)
 *             method 3: (max_gen_length + 1, B * beamk, V)            as method 1
 *             method 4: (max_gen_length + 1, B * beamk, V)            as method 1; slab 0 (step 0) is read as well
 *   normals : (max_gen_length + 1, layers, B * beamk, n) standard normals of the state noise
 * rows are the compacted beam rows of that step (image b owns rows b * beamk ...).  sampling = NULL is sat_beam_search_batched.
 *
 * SAT_SAMPLE_NUCLEUS (top-p; Holtzman et al. 2019) differs from SAT_SAMPLE_TOPK only in which words of a hypothesis are candidates.
 * For a live row at a free step >= 1 with scores s[v] (running sum + this step's log-probability; masked and banned words at -inf):
 *   F = the finite entries, w[v] = exp(s[v] - max_F s), W = sum_F w; F ordered by score descending, ties to the lower word id;
 *   the nucleus N is the shortest leading run of that order with sum w >= sample_topp * W.  sample_topp >= 1, or a target that
 *   rounding keeps the running sum from reaching, gives N = F; a non-empty F always gives a non-empty N.  The parent's score is a
 *   constant of the row, so N is the top-p set of the step's own conditional distribution.
 *   key[v] = s[v] / step + G[v] for v in N, else -inf: method 2's rule, candidate_probs = softmax(candidate_scores / step)
 *   (model.py:365-379), on another candidate set.  The per-image top-k over the keys and the score gather then run as for the
 *   other methods, and the first free step stays the deterministic top beamk of row 0 (model.py:338-347).
 * With beamk = 1 this draws proportionally to p^(1/step) inside the nucleus, as SAT_SAMPLE_TOPK does inside its candidates, NOT
 * proportionally to p: the reference's convention, kept on purpose so that the two methods differ in the candidate set only.
 * Without a table the variate of word v is the hash at (seed, step, row * V + v), method 1's indexing.  sample_topp must be finite
 * and in (0, 1] (SAT_EINVAL before any launch); top-g clipping does not combine with it; prefix, banned ids and the masks do.
 *
 * SAT_SAMPLE_ANCESTRAL draws every word, the first one included, from the model's own distribution: methods 1 to 3 sharpen it
 * (softmax(20 s / step), p^(1/step)) and take the first step deterministically, which biases a policy gradient.  For a live row with
 * masked scores s[v] (step 0 masks {START, PAD, END, UNK}, later steps {START, PAD}; masked words stay at -inf):
 *   key[v] = s[v] + G[v]; the row takes the arg-max key, ties to the lower word id; the recorded score is s at the pick.
 * That is one draw from softmax(logits / T) renormalised over the unmasked words (the Gumbel-max identity), T the search's own
 * temperature of the step.  G comes from the table gumbel (max_gen_length + 1, B * beamk, V) or from the hash at
 * (seed, step, row * V + v): method 1's layout and indexing, here for step 0 too.  Defined for beamk == 1 only (independent samples
 * of one image are rows of a larger batch, so that no per-image top-k couples them); beamk != 1, any constraint, or a stream that
 * is being captured gives SAT_EINVAL before any launch.  The cut rule holds as for every method: the word drawn at step
 * max_gen_length is dropped, so a hypothesis of max_gen_length words does not depend on the last step's draw. */
#define SAT_SAMPLE_BEAM 0
#define SAT_SAMPLE_MULTINOMIAL 1
#define SAT_SAMPLE_TOPK 2
#define SAT_SAMPLE_NUCLEUS 3
#define SAT_SAMPLE_ANCESTRAL 4
typedef struct sat_beam_sampling {
    int32_t method;            /* SAT_SAMPLE_*                                                  */
    int32_t sample_topk;       /* candidates per hypothesis, method 2                            */
    uint64_t seed;
    const float* gumbel;       /* device pointer or NULL                                         */
    float decoder_noise;       /* 0 = off; step s adds N(0,1) * decoder_noise / (s + 1) to h     */
    float sample_topp;         /* method 3: the nucleus' share of the mass, (0, 1]; all-zero bits = unset (methods 0-2 ignore it) */
    const float* normals;      /* device pointer or NULL                                         */
} sat_beam_sampling;
int sat_beam_search_sampled(const sat_decoder_dims* d, const sat_decoder_params* w, const float* ann, int32_t beamk, int32_t max_gen_length,
                            const float* temperatures_host, int32_t n_temperatures, const int32_t* special_ids_host, const sat_beam_sampling* sampling,
                            int32_t* tok_in, int32_t* prev_row, float* alpha_hist, int32_t* fin_count, int32_t* fin_step, int32_t* fin_row,
                            float* fin_score, float* fin_mean, void* workspace, size_t workspace_bytes, void* stream);
/* The same search under constraints on the selection step ("Constrained search"); step s is 0-based, image b has a forced
 * prefix of P_b = prefix_len[b] words:
 *   banned  : score[:, id] = -inf for every banned id at every step of every image, on top of the START / PAD (/ END / UNK) masks.
 *   prefix  : s < P_b   every one of the beamk rows keeps its parent and takes prefix[b][s]; its score is the word's own
 *                       log-probability added to the running sum (masks and banned ids apply; the sampling method is not consulted)
 *             s == P_b  the first free step: the top beamk of row 0 only (model.py:343), row j keeps parent j; the first-step mask
 *                       {START, PAD, END, UNK} when P_b == 0, the mask of the later steps {START, PAD} when P_b > 0
 *             s > P_b   the free search
 *   topg    : at s > P_b the candidates of an image are the topg best words of every live row (value descending, ties to the lower
 *             id); the kept hypotheses are the top k of these k * topg candidates (value descending, ties to the lower flat index
 *             row * V + word).  Deterministic; combines with SAT_SAMPLE_BEAM only.  topg >= beamk is the plain search.
 * Finished hypotheses, tok_in, prev_row, alpha_hist and fin_* keep the layout above; sequences and scores include the prefix.
 * The ids are DEVICE arrays and are not read on the host: prefix ids must lie in [0, V) and be none of START / PAD / END / UNK / banned
 * (out-of-range ids are clamped, prefix_len to 0..max_prefix).  constraints = NULL, or topg == 0 && max_prefix == 0 && n_banned == 0,
 * enqueues exactly what sat_beam_search_sampled enqueues.  Workspace: sat_beam_search_constrained_workspace_bytes (topg adds the
 * (B * beamk, topg) candidate list to the plain search's workspace; with topg == 0 both queries agree). */
typedef struct sat_beam_constraints {
    int32_t topg;              /* 0 = off, else 1..V                                             */
    int32_t max_prefix;        /* row stride of prefix; 0 = no prefix; <= max_gen_length         */
    const int32_t* prefix;     /* device (B, max_prefix) or NULL                                 */
    const int32_t* prefix_len; /* device (B) or NULL                                             */
    const int32_t* banned;     /* device (n_banned) or NULL                                      */
    int32_t n_banned;
    int32_t reserved;
} sat_beam_constraints;
size_t sat_beam_search_constrained_workspace_bytes(const sat_decoder_dims* d, int32_t beamk, int32_t topg);
int sat_beam_search_constrained(const sat_decoder_dims* d, const sat_decoder_params* w, const float* ann, int32_t beamk, int32_t max_gen_length,
                                const float* temperatures_host, int32_t n_temperatures, const int32_t* special_ids_host, const sat_beam_sampling* sampling,
                                const sat_beam_constraints* constraints, int32_t* tok_in, int32_t* prev_row, float* alpha_hist, int32_t* fin_count,
                                int32_t* fin_step, int32_t* fin_row, float* fin_score, float* fin_mean, void* workspace, size_t workspace_bytes,
                                void* stream);
/* The same search under rules that read what a hypothesis has already said ("History rules").  A live row of step s has
 * the history w_1 .. w_s: the words fed at steps 1..s, without START, forced prefix words included.  With x the row's raw fp32 logits
 * and T the step's temperature, in this order:
 *   1. repetition_penalty theta (CTRL, Keskar et al. 2019): for every DISTINCT word v of the history, once however often it occurs,
 *      x[v] = x[v] > 0 ? x[v] / theta : x[v] * theta; then log-softmax of x / T plus the parent score as in every search.  Every
 *      step with a non-empty history, forced steps included (the forced word's penalised score joins the running sum).
 *   2. the START / PAD (/ END / UNK) masks and the banned ids, unchanged.
 *   3. min_length m: at a free step s < m, score[END] = -inf.  END taken at step s closes a caption of s words, so no finished caption
 *      has fewer than m words; the cut at max_gen_length is unchanged.
 *   4. no_repeat_ngram n: at a free step s >= n - 1, with u the last n - 1 words of the history (empty for n = 1), every p in 0 .. s - n
 *      with hist[p : p + n - 1] == u sets score[hist[p + n - 1]] = -inf.  n = 1 blocks every word already used.
 *   Rules 3 and 4 skip the forced steps (s < P_b): a prefix is obeyed even if it repeats, and its words count as history afterwards.
 * Everything downstream (top-g candidates, multinomial / top-k / nucleus keys, the per-image top-k, the score gather, the update) reads
 * these scores as it reads today's; SAT_SAMPLE_ANCESTRAL refuses the rules as it refuses every constraint.  A row loses at most one
 * word per earlier position, so V - masked - banned - max_gen_length >= max(beamk, topg, 1) keeps enough words selectable (the caller's
 * check; sat_amd/constraints.py makes it).  The history is a (B * beamk, max_gen_length + 1) int32 table in the workspace, double-buffered
 * and advanced by one small launch per step; the search stays launches only but is not graph-replayed.
 * history = NULL, or every rule off (no_repeat_ngram == 0 && min_length == 0 && repetition_penalty all-zero bits or 1.0f), enqueues
 * exactly what sat_beam_search_constrained enqueues and needs only sat_beam_search_constrained_workspace_bytes; the query below adds
 * the two history tables of a search with a rule on to that figure (and serves either).  SAT_EINVAL before any launch: a negative
 * no_repeat_ngram or min_length, min_length > max_gen_length, repetition_penalty <= 0 or not finite, and with a rule on:
 * max_gen_length + 1 > SAT_CAPTION_MAX_LEN, ancestral sampling, a stream that is being captured. */
typedef struct sat_beam_history {
    int32_t no_repeat_ngram;     /* 0 = off, else >= 1 */
    int32_t min_length;          /* 0 = off, <= max_gen_length */
    float   repetition_penalty;  /* all-zero bits or 1.0f = off; finite, > 0 */
    int32_t reserved;
} sat_beam_history;
size_t sat_beam_search_history_workspace_bytes(const sat_decoder_dims* d, int32_t beamk, int32_t topg, int32_t max_gen_length);
int sat_beam_search_history(const sat_decoder_dims* d, const sat_decoder_params* w, const float* ann, int32_t beamk, int32_t max_gen_length,
                            const float* temperatures_host, int32_t n_temperatures, const int32_t* special_ids_host, const sat_beam_sampling* sampling,
                            const sat_beam_constraints* constraints, const sat_beam_history* history, int32_t* tok_in, int32_t* prev_row,
                            float* alpha_hist, int32_t* fin_count, int32_t* fin_step, int32_t* fin_row, float* fin_score, float* fin_mean,
                            void* workspace, size_t workspace_bytes, void* stream);
/* Diverse (group) beam search: Hamming diversity between the groups of a beam (Vijayakumar et al. 2016; DESIGN.md 5, "Diverse beam
 * search").  beamk = K rows of an image are G = groups groups of Kg = K / G rows (K % G == 0); rows g * Kg .. (g + 1) * Kg - 1 belong to
 * group g for the whole search.  A group is a beam of its own: its own live count, its own parents (a hypothesis descends from a row of
 * its group only), its own finished list, its own cut at max_gen_length, and the initial state of a plain search at beamk = Kg (the
 * reshape of the initial state acts on the group's Kg rows).  At a step the groups of an image select in the order
 * g = 0 .. G - 1; group g ranks its candidates (row j of the group, word v) by
 *   pen = s[j, v] - lambda * c[v]
 * with s the score of every search above (log-softmax, parent score, masks, banned ids, history rules) and c[v] the number of
 * hypotheses the groups < g of this image kept AT THIS STEP with word v (END included; a group without a live row adds nothing).  pen
 * is fp32 with two roundings, the product then the difference, so c == 0 or lambda == 0 leaves s bit for bit.  The group keeps its
 * klive best candidates by pen descending, ties to the lower flat index j * V + v (sat_topk's rule, its -inf behaviour included); at
 * step 0 it selects from its first row only.  A hypothesis CARRIES s, NOT pen: fin_score, the parent scores, perplexity and every
 * rescoring stay sums of model log-probabilities; fin_mean is the mean over the group's kept hypotheses at that moment.
 * The layout of the results is the one above: tok_in / prev_row / alpha_hist (., B, K[, L]) with image-level parent rows in prev_row,
 * fin_* (B, K) compacted per image (group ascending, inside a group the append order), fin_row image-level, fin_count[b] ends at K.
 * groups = NULL, or groups->groups 0 or 1, enqueues exactly what sat_beam_search_history enqueues.  SAT_EINVAL before any launch: groups
 * < 0, diversity_penalty negative or not finite; and with groups > 1: beamk % groups != 0, beamk > 1024, a sampling method other than
 * SAT_SAMPLE_BEAM, decoder_noise, topg, a forced prefix, a stream that is being captured.  Banned ids and the history rules combine.
 * Workspace: sat_beam_search_groups_workspace_bytes (sat_beam_search_history_workspace_bytes with topg = 0, plus the live counts and
 * the finished lists per group; it serves the call with groups off as well). */
typedef struct sat_beam_groups {
    int32_t groups;              /* 0 or 1 = off, else a divisor of beamk */
    float   diversity_penalty;   /* lambda: finite, >= 0 */
} sat_beam_groups;
size_t sat_beam_search_groups_workspace_bytes(const sat_decoder_dims* d, int32_t beamk, int32_t groups, int32_t max_gen_length);
int sat_beam_search_groups(const sat_decoder_dims* d, const sat_decoder_params* w, const float* ann, int32_t beamk, int32_t max_gen_length,
                           const float* temperatures_host, int32_t n_temperatures, const int32_t* special_ids_host, const sat_beam_sampling* sampling,
                           const sat_beam_constraints* constraints, const sat_beam_history* history, const sat_beam_groups* groups, int32_t* tok_in,
                           int32_t* prev_row, float* alpha_hist, int32_t* fin_count, int32_t* fin_step, int32_t* fin_row, float* fin_score,
                           float* fin_mean, void* workspace, size_t workspace_bytes, void* stream);
/* Required words: a caption must contain the words of its image (Anderson et al. 2017, constrained beam search; Post & Vilar 2018,
 * dynamic beam allocation; DESIGN.md 5, "Required words").  Image b requires its C_b = n_words[b] words q_0 .. q_{C_b - 1} (n_words is
 * clamped to 0 .. max_required on the device; a word id outside [0, V) requires nothing: it is dropped from the image's list and C_b
 * counts the rest).  A step runs as in sat_beam_search_history, with the history tables on even when every rule is off, up to the
 * scores s[j, v] (log-softmax at the step's temperature, parent score, masks, banned ids, history rules) of the image's
 * k = clamp(klive[b], 0, K) live rows (row 0 alone at step 0).  Then, per image:
 *   met(j)       the set of c for which q_c is among the words row j has said (its `step` history entries)
 *   END held     s'[j, v] = s[j, v], except s'[j, END] = -inf while met(j) is not all of 0 .. C_b - 1: a hypothesis that ends by saying
 *                <END> contains every required word; the cut at max_gen_length records whatever is live, as in every search
 *   candidates   the union, by flat index j * V + v, of  A: the k picks of sat_topk's rule over s' (value descending, ties to the lower
 *                flat index), those at -inf dropped;  R: (j, q_c) for every row j and every c not in met(j), where s' > -inf;
 *                M: every row's single best word (the lowest v on ties), where s' > -inf
 *   bank(j, v)   |met(j) U {c : q_c == v}|, in 0 .. C_b; at the last step (step == max_gen_length) |met(j)|: the word picked there is
 *                not part of the caption (it is <END>, or the cut drops it), and counting it would let a hypothesis that completes its
 *                words with the dropped word push a complete one out of the beam
 *   allocation   round robin from the fullest bank: a pointer p starts at C_b; for pick t = 0 .. k - 1 walk the banks p, p - 1, .., 0,
 *                C_b, .., p + 1 to the first that still holds an untaken candidate, take its best one (value descending, ties to the
 *                lower flat index), set p = (that bank - 1) mod (C_b + 1); nothing left: -inf / index 0 (the groups' rule)
 *   stores       the pick's s', unchanged, and its image-level flat index: a hypothesis carries model log-probabilities, the allocation
 *                steers the selection only
 * An image with C_b == 0 takes sat_topk's picks exactly (its -inf behaviour included), so in a mixed batch it gets the result of
 * sat_beam_search_history.  No atomics: same input, same bits.  After the last step one kernel back-traces every finished hypothesis
 * (as sat_beam_hypotheses does), counts the required words it contains, writes req_met[b] = the largest count of image b and compacts
 * the image's fin_* lists, order kept, to the hypotheses that reach it; fin_count[b] becomes their number (>= 1).  Every consumer of
 * the lists then chooses among the captions that meet the most words.
 * Guarantee: if beamk >= 1, max_gen_length >= C_b and a required word a row has not said is never at -inf (not masked, banned, or
 * blocked by no_repeat_ngram == 1 after it was said), the fullest bank gains a word every step until it is complete and always holds
 * slot 0, so req_met[b] == C_b.
 * Banned ids, the three history rules, temperature lists, layers > 1, deep output and bf16 combine.  required == NULL or max_required
 * == 0 enqueues exactly what sat_beam_search_history enqueues; req_met may then be NULL and is not written.  SAT_EINVAL before any
 * launch: max_required outside 0 .. SAT_BEAM_REQUIRED_MAX; and with max_required > 0: a null words / n_words / req_met, beamk >
 * SAT_BEAM_REQUIRED_MAX_K, max_required > max_gen_length, max_gen_length + 1 > SAT_CAPTION_MAX_LEN (the history table), a sampling
 * method other than SAT_SAMPLE_BEAM, decoder_noise, topg, a forced prefix, a stream that is being captured.  Workspace:
 * sat_beam_search_required_workspace_bytes (sat_beam_search_history_workspace_bytes with topg = 0; it refuses the sizes the search
 * refuses and serves the call with required words off as well). */
#define SAT_BEAM_REQUIRED_MAX   8      /* required words per image */
#define SAT_BEAM_REQUIRED_MAX_K 256    /* beamk with required words on: K * (MAX + 2) candidates live in LDS */
typedef struct sat_beam_required {
    int32_t max_required;        /* C: 0 = off, else 1..SAT_BEAM_REQUIRED_MAX; row stride of `words` */
    int32_t reserved;
    const int32_t* words;        /* device (B, C): image b's required ids, its first n_words[b] entries */
    const int32_t* n_words;      /* device (B): 0..C; an image with 0 is searched as today */
} sat_beam_required;
size_t sat_beam_search_required_workspace_bytes(const sat_decoder_dims* d, int32_t beamk, int32_t max_gen_length, int32_t max_required);
int sat_beam_search_required(const sat_decoder_dims* d, const sat_decoder_params* w, const float* ann, int32_t beamk, int32_t max_gen_length,
                             const float* temperatures_host, int32_t n_temperatures, const int32_t* special_ids_host, const sat_beam_sampling* sampling,
                             const sat_beam_constraints* constraints, const sat_beam_history* history, const sat_beam_required* required,
                             int32_t* tok_in, int32_t* prev_row, float* alpha_hist, int32_t* fin_count, int32_t* fin_step, int32_t* fin_row,
                             float* fin_score, float* fin_mean, int32_t* req_met /* (B) */, void* workspace, size_t workspace_bytes, void* stream);
/* The selection kernel of sat_beam_search_required on its own: scores (B, beamk, V), klive (B) live rows (clamped to 0 .. beamk; an
 * image with none keeps its slots untouched), hist (B * beamk, hist_stride) the words every row has said, its first hist_len entries
 * (clamped to 0 .. hist_stride; hist may be NULL with hist_stride 0); first_step & 1 selects from row 0 only, first_step & 2 is the
 * search's last step (banks of |met(j)|).  Slot t of image b
 * receives its t-th pick: values the score, indices the flat index row * V + word.  work is scratch, (B, beamk, V) floats.
 * required->max_required == 0 gives every image sat_topk's picks.  No atomics: same input, same bits.  SAT_EINVAL before the launch: a
 * null pointer, a size < 1, beamk > SAT_BEAM_REQUIRED_MAX_K, max_required outside 0 .. SAT_BEAM_REQUIRED_MAX, hist_stride outside
 * 0 .. SAT_CAPTION_MAX_LEN.  NaN in scores: unspecified. */
int sat_beam_required_select(const float* scores, const int32_t* klive, int32_t B, int32_t beamk, int32_t V, const int32_t* hist, int32_t hist_stride,
                             int32_t hist_len, int32_t first_step, const sat_beam_required* required, int32_t end_id, float* work, float* values,
                             int32_t* indices, void* stream);
/* Ensemble decoding: ONE beam search over several captioning models ("Ensemble decoding").  Members i = 0 .. M - 1 are
 * whole decoders, each with its own sizes (L, D, A, m, n, layers, deep_output, precision), parameters and annotations (B, L_i, D_i) of
 * the same B images; they share the vocabulary (V and the four special ids).  weight[i] >= 0, summing to 1 within 1e-5.  Every member
 * is fed the same tokens.  At a step with temperature T, for every hypothesis row, with l_i = log_softmax(z_i / T) of member i's logits:
 *   SAT_ENSEMBLE_ARITHMETIC  a mixture of the distributions: c_v = log sum_i w_i exp(l_i,v), evaluated per word as
 *                            mx + log sum_i exp(l_i,v + log w_i - mx) with mx the largest exponent
 *   SAT_ENSEMBLE_GEOMETRIC   a product of experts:           c_v = sum_i w_i l_i,v
 * members with weight 0 are skipped in both.  The step's score is parent + log_softmax(c)_v (for the mixture that normalisation is zero
 * up to rounding, for the product it makes c a distribution); the masks, banned ids and history rules then apply as in every search.
 * That is: the ensemble is a model whose logits are c, searched at temperature 1 with the kernels of the searches above.  After the
 * update every member's state is gathered through the same parent map.  The outputs have sat_beam_search_batched's layout;
 * alpha_hist (max_gen_length + 1, B, beamk, L_0) holds member 0's attention (the members' L differ, so there is no common map).
 * "beam" sampling only.  constraints may carry banned ids; history may carry min_length and no_repeat_ngram; either may be NULL.
 * SAT_EINVAL before any launch: members outside 1..SAT_ENSEMBLE_MAX, a null member pointer (dims / params / ann), members that differ
 * in B or V, a weight that is negative or not finite, weights that do not sum to 1 within 1e-5, an unknown combine, topg > 0,
 * max_prefix > 0, a repetition_penalty other than all-zero bits or 1.0f, a stream that is being captured.
 * Workspace: sat_beam_search_ensemble_workspace_bytes (the members' search workspaces, the combined logits and one step of attention
 * maps for every member but the first; it holds the history tables wherever the history rules can run). */
#define SAT_ENSEMBLE_MAX 8
#define SAT_ENSEMBLE_ARITHMETIC 0
#define SAT_ENSEMBLE_GEOMETRIC 1
typedef struct sat_beam_ensemble {
    int32_t members;                                     /* 1..SAT_ENSEMBLE_MAX */
    int32_t combine;                                     /* SAT_ENSEMBLE_* */
    const sat_decoder_dims* dims[SAT_ENSEMBLE_MAX];      /* per member; B and V agree */
    const sat_decoder_params* params[SAT_ENSEMBLE_MAX];
    const float* ann[SAT_ENSEMBLE_MAX];                  /* device (B, L_i, D_i) */
    float weight[SAT_ENSEMBLE_MAX];                      /* host; >= 0, sum 1 */
} sat_beam_ensemble;
size_t sat_beam_search_ensemble_workspace_bytes(const sat_beam_ensemble* ensemble, int32_t beamk, int32_t max_gen_length);
int sat_beam_search_ensemble(const sat_beam_ensemble* ensemble, int32_t beamk, int32_t max_gen_length, const float* temperatures_host,
                             int32_t n_temperatures, const int32_t* special_ids_host, const sat_beam_constraints* constraints,
                             const sat_beam_history* history, int32_t* tok_in, int32_t* prev_row, float* alpha_hist, int32_t* fin_count,
                             int32_t* fin_step, int32_t* fin_row, float* fin_score, float* fin_mean, void* workspace, size_t workspace_bytes,
                             void* stream);
/* One search descriptor ("One search descriptor"): everything a batched search is asked to do, named once.  sat_beam_search
 * runs what the entry points above run - the same checks in the same order, the same launches, the same bits - for the single-model
 * search (d, w, ann) or the ensemble search (ensemble != NULL; d, w and ann are then NULL).  sampling / constraints / history / groups /
 * required: NULL is off, and each struct's specification is the comment at its typedef above; the outputs have
 * sat_beam_search_batched's layout, req_met is sat_beam_search_required's.  SAT_EINVAL before any launch: a null descriptor or output
 * struct, whatever the entry points above refuse, and with an ensemble: a non-NULL d / w / ann, a sampling method other than
 * SAT_SAMPLE_BEAM, decoder_noise, groups > 1, max_required > 0 (each message names its field).
 * sat_beam_search_desc_workspace_bytes is the figure sat_beam_search compares workspace_bytes against: both come from one plan of
 * the descriptor, so the query is exact and refuses (0, with sat_last_error set) every descriptor the search refuses; it reads no
 * output, no workspace and no stream, so "the stream is being captured" is the search's refusal alone.
 * The seven sat_beam_search_* entry points above are adapters kept for existing callers: each fills a descriptor and runs this path
 * under its own name.  Their six workspace queries keep their documented figures; for the call a query was written for, its figure is
 * never below this one (the groups, required and ensemble queries add history tables that a search without a rule does not use). */
typedef struct sat_beam_search_desc {
    const sat_decoder_dims*   d;        /* single model: d, w, ann; all three NULL with an ensemble */
    const sat_decoder_params* w;
    const float*              ann;      /* device (B, L, D) */
    const sat_beam_ensemble*  ensemble; /* or NULL */
    int32_t beamk, max_gen_length;
    const float*   temperatures_host;
    int32_t n_temperatures, reserved;
    const int32_t* special_ids_host;    /* {START, PAD, END, UNK} */
    const sat_beam_sampling*    sampling;
    const sat_beam_constraints* constraints;
    const sat_beam_history*     history;
    const sat_beam_groups*      groups;
    const sat_beam_required*    required;
} sat_beam_search_desc;
typedef struct sat_beam_search_out {
    int32_t *tok_in, *prev_row;
    float* alpha_hist;
    int32_t *fin_count, *fin_step, *fin_row;
    float *fin_score, *fin_mean;
    int32_t* req_met;                   /* (B); NULL unless required words are on */
} sat_beam_search_out;
size_t sat_beam_search_desc_workspace_bytes(const sat_beam_search_desc* s);
int sat_beam_search(const sat_beam_search_desc* s, const sat_beam_search_out* o, void* workspace, size_t workspace_bytes, void* stream);
/* The combine kernel of sat_beam_search_ensemble on its own: combined (rows, V) = c as above from `members` device arrays (rows, V).
 * logits is a HOST array of device pointers, weights a HOST array.  Finite logits give finite output (no -inf, no NaN), however
 * peaked a member is; a -inf logit contributes no mass.  No atomics: same input, same bits.  SAT_EINVAL before the launch: a null
 * pointer, members / weights / combine as above, rows or V < 1, a temperature that is not positive. */
int sat_beam_ensemble_scores(const float* const* logits, const float* weights, int32_t members, int32_t combine, int32_t rows, int32_t V,
                             float temperature, float* combined, void* stream);
/* The selection kernel of sat_beam_search_groups on its own: scores (B, beamk, V), klive (B, groups) live rows per group (clamped to
 * 0 .. beamk / groups), first_step != 0 selects from each group's first row only.  Slot g * Kg + t of image b receives the group's t-th
 * pick: values the UNPENALISED score, indices the group-local flat index row * V + word; slots past klive stay untouched.  work is
 * scratch, (B, beamk, V) floats.  No atomics: same input, same bits.  SAT_EINVAL before the launch: a null pointer, a size < 1,
 * beamk % groups != 0, beamk > 1024, beamk / groups > V, diversity_penalty negative or not finite.  NaN in scores: unspecified. */
int sat_beam_group_select(const float* scores, const int32_t* klive, int32_t B, int32_t beamk, int32_t groups, int32_t V, int32_t first_step,
                          float diversity_penalty, float* work, float* values, int32_t* indices, void* stream);
/* A -inf logit gets the score -inf and leaves the rest of its row as torch.log_softmax does; a row of nothing but -inf gives NaN, as
 * torch does.  Masked ids outside [0, V) mask nothing. */
int sat_beam_scores(const float* logits, int32_t beams, int32_t V, float temperature, const int32_t* masked_ids /* device */,
                    int32_t n_masked, const float* parent_scores /* (beams) or NULL */, float* scores, void* stream);
/* The score kernel of sat_beam_search_history on its own, every row at a free step: row r has said the first hist_len[r] words of
 * hist (rows, hist_stride), hist_stride <= SAT_CAPTION_MAX_LEN (lengths are clamped to 0..hist_stride, ids outside [0, V) are skipped).
 * Rules 1, 2 (masked_ids) and 4 as above with s = hist_len[r]; rule 3 masks end_id when step < rules->min_length.  logits is only read.
 * With every rule off the output is sat_beam_scores' bit for bit.  No atomics: same input, same bits.  SAT_EINVAL before the launch:
 * a null pointer, rows / V < 1, a temperature that is not positive, hist_stride outside 0..SAT_CAPTION_MAX_LEN, malformed rules (as
 * above), a stream that is being captured. */
int sat_beam_history_scores(const float* logits /* (rows, V) */, int32_t rows, int32_t V, float temperature, const int32_t* masked_ids,
                            int32_t n_masked, const float* parent_scores /* (rows) or NULL */, const int32_t* hist /* (rows, hist_stride) */,
                            const int32_t* hist_len /* (rows) */, int32_t hist_stride, const sat_beam_history* rules, int32_t step, int32_t end_id,
                            float* scores, void* stream);
/* The k largest of x (1 <= k <= n) in descending order, equal values in increasing index order, every index once: a stable descending
 * sort cut at k.  -inf entries are ordinary values that sort last, so with fewer than k entries above -inf the result ends in the -inf
 * entries of lowest index.  (torch.topk promises no order among equal values.)  NaN in x: the result is unspecified. */
int sat_topk(const float* x, float* work /* n floats scratch */, int64_t n, int32_t k, float* values, int32_t* indices, void* stream);
/* The key kernel of SAT_SAMPLE_NUCLEUS on its own, every row live: keys (rows, V) as above with `step` the divisor (> 0) and
 * `stream` the hash stream (the search passes the step); gumbel (rows, V) or NULL; nucleus_size (rows) or NULL receives |N| per row
 * (0 for a row without a finite entry, whose keys are all -inf).  Same input, same output, bit for bit. */
int sat_nucleus_keys(const float* scores, int32_t rows, int32_t V, float topp, float step, uint64_t seed, uint64_t stream,
                     const float* gumbel /* (rows, V) or NULL */, float* keys, int32_t* nucleus_size /* (rows) or NULL */, void* stream_handle);

/* ------------------------------------------------------------------ scoring decoded captions (SAT.val_batch: model.py:449-472, 646-682)
 * The three calls below take the buffers sat_beam_search_batched / _sampled leave on the device to per-image metric statistics
 * without a host round trip (kernel launches only: capturable).  Tokens are int32 everywhere: pass int32 device copies of the
 * dataset's int64 captions and lengths.  Limits (SAT_EINVAL with a message beyond them, never a truncated count):
 * max_gen_length + 1 = cap_width <= SAT_CAPTION_MAX_LEN, T <= SAT_CAPTION_MAX_LEN, R <= SAT_CAPTION_MAX_REFS, m <= SAT_CAPTION_MAX_EMBED.
 * Indices read from device memory (steps, rows, lengths) are clamped to their ranges before they address anything. */
#define SAT_CAPTION_MAX_LEN 128
#define SAT_CAPTION_MAX_REFS 16
#define SAT_CAPTION_MAX_EMBED 2048
#define SAT_RESCORE_NONE 0
#define SAT_RESCORE_LN 1   /* s / step                 */
#define SAT_RESCORE_WR 2   /* s + reward * step        */
#define SAT_RESCORE_BAR 3  /* s + reward * (-fin_mean) */
/* Winning hypothesis of every image (model.py:341-348, 467-471): the fin_count[b] finished hypotheses are rescored in fp32 without
 * FMA contraction (the reward is the fp32 the caller passes), the FIRST maximum in append order wins (list.index(max(...))), and its
 * parent rows are walked from fin_step down to step 1.
 *   cap_tokens (B, max_gen_length + 1)  tokens fed at steps 1..step, then pad_id
 *   cap_len, cap_step (B)               step = number of tokens;  cap_score (B) the rescored value;  cap_raw (B) the raw score
 *   cap_alpha (B, max_gen_length, L)    optional (needs alpha_hist): the attention maps of steps 0..step-1, zero beyond */
int sat_beam_select(const int32_t* tok_in, const int32_t* prev_row, const int32_t* fin_count, const int32_t* fin_step, const int32_t* fin_row,
                    const float* fin_score, const float* fin_mean, const float* alpha_hist /* or NULL */, int32_t B, int32_t beamk,
                    int32_t max_gen_length, int32_t L, int32_t rescore_method, float rescore_reward, int32_t pad_id, int32_t* cap_tokens,
                    int32_t* cap_len, float* cap_score, float* cap_raw, int32_t* cap_step, float* cap_alpha /* or NULL */, void* stream);
/* sat_beam_select with the winner given instead of computed (consensus reranking picks it: sat_caption_mbr below).  pick (B): a
 * hypothesis index in append order, clamped into [0, max(fin_count[b] - 1, 0)]; pick_score (B, beamk) float64 or NULL: cap_score[b] is
 * (float)pick_score[b][pick] when it is given and the raw score otherwise.  cap_tokens, cap_len, cap_raw, cap_step and the optional
 * cap_alpha are sat_beam_select's for that hypothesis (one back-trace, shared by the two kernels); an image without a finished
 * hypothesis gets the empty caption, raw 0 and, without pick_score, cap_score -inf, as there. */
int sat_beam_select_at(const int32_t* tok_in, const int32_t* prev_row, const int32_t* fin_count, const int32_t* fin_step, const int32_t* fin_row,
                       const float* fin_score, const float* alpha_hist /* or NULL */, const int32_t* pick, const double* pick_score /* or NULL */,
                       int32_t B, int32_t beamk, int32_t max_gen_length, int32_t L, int32_t pad_id, int32_t* cap_tokens, int32_t* cap_len,
                       float* cap_score, float* cap_raw, int32_t* cap_step, float* cap_alpha /* or NULL */, void* stream);
/* The back-trace of EVERY finished hypothesis of every image, tokens only: one thread per (b, f) walks the parent rows as
 * sat_beam_select does for the winner (steps and rows clamped before they address anything).
 *   hyp_tokens (B, beamk, max_gen_length + 1)  tokens fed at steps 1..step of hypothesis f (append order), then pad_id
 *   hyp_len (B, beamk)                         step; slots f >= fin_count[b]: length 0, all pad_id */
int sat_beam_hypotheses(const int32_t* tok_in, const int32_t* prev_row, const int32_t* fin_count, const int32_t* fin_step, const int32_t* fin_row,
                        int32_t B, int32_t beamk, int32_t max_gen_length, int32_t pad_id, int32_t* hyp_tokens, int32_t* hyp_len, void* stream);
/* The integers nltk's corpus BLEU / GLEU sum per segment (sat_amd/metrics.py is the specification).  Hypothesis b = the first
 * cap_len[b] tokens of cap_tokens (B, cap_width); reference (b, r) = refs[b][r][1:ref_lengths[b][r]] of refs (B, R, T) (without START
 * and END, as score_captions slices them).  stats (B, 12) int32:
 *   [0..3]  clipped n-gram matches, n = 1..4          [4..7]  max(1, hyp_len - n + 1), per segment as modified_precision
 *   [8]     hyp_len                                    [9]     closest reference length (a tie goes to the shorter reference)
 *   [10,11] GLEU tp and max(tp + fp, tp + fn) over all 1..4-grams of the reference with the best ratio (integer cross-multiplication;
 *           a later reference replaces an earlier one only if strictly better; references with a zero total are skipped; 0, 0 if all are) */
int sat_caption_stats(const int32_t* cap_tokens, const int32_t* cap_len, int32_t cap_width, const int32_t* refs, const int32_t* ref_lengths,
                      int32_t B, int32_t R, int32_t T, int32_t* stats, void* stream);
/* best_cosine[b] = max over r of F.cosine_similarity(mean embedding of reference (b, r), mean embedding of hypothesis b) (model.py:660-673;
 * torch 2's definition: sum_d (x_d / max(|x|, eps)) (y_d / max(|y|, eps)), eps = 1e-8).  A kernel of its own, not fused into
 * sat_caption_stats.  Rows of embedding (V, m) are gathered in fp32; an empty hypothesis or reference gives NaN like torch's empty mean,
 * and so does a token outside [0, V) (it is not read). */
int sat_caption_cosine(const int32_t* cap_tokens, const int32_t* cap_len, int32_t cap_width, const int32_t* refs, const int32_t* ref_lengths,
                       int32_t B, int32_t R, int32_t T, const float* embedding, int32_t V, int32_t m, float* best_cosine, void* stream);

/* ------------------------------------------------------------------ CIDEr-D and ROUGE-L against a corpus of references
 * (sat_amd/metrics.py is the specification: document_frequency, cider_d, rouge_l).  Reference (b, r) and hypothesis b are sliced as in
 * sat_caption_stats; an "n-gram" is n = 1..4 consecutive tokens; the same limits and SAT_EINVAL messages apply, and a capacity that is
 * not a power of two (or is above 2^36) is refused.  Tokens are clamped into [0, 65534] before they are packed: a vocabulary needs
 * vocab_size <= 65535, and out-of-range input gives a wrong score, never a stray access.
 *
 * The document-frequency table is an open-addressing hash table (linear probing) in device memory that the caller allocates:
 * sat_ngram_table_bytes(capacity) bytes = capacity 64-bit keys followed by capacity 32-bit counts.  A key packs an n-gram exactly:
 * (token + 1) in 16 bits per position, the first token in the lowest bits, unused positions 0; the order n is implicit, different
 * n-grams never share a key, key 0 is an empty slot.  count = df = the number of images added whose references contain the n-gram at
 * least once, in any of the image's R references (duplicated references count once).  The content as a key -> count mapping does not
 * depend on the order in which images arrive; slot positions may differ from run to run.
 *   sat_ngram_table_clear   empties the table (a launch; call it before the first add)
 *   sat_ngram_table_add     adds B images, one launch (may be called again and again; launches on one stream are ordered).  A full table
 *                           sets *error_flag (device int32, zeroed by the caller) to non-zero and drops the n-gram; the probe loop is
 *                           bounded by the capacity and the launch always completes.  The caller keeps the number of images added.
 *   sat_caption_consensus   scores (B, 2) float64 = [CIDEr-D, ROUGE-L] per image against a table holding n_images images, in a LATER
 *                           launch than the adds.  All arithmetic in fp64, every sum in a fixed order: the same table content gives
 *                           bit-identical scores.
 * CIDEr-D (sigma = 6 in the COCO scorer): with logN = log(n_images), every distinct n-gram g of a sentence s with term frequency tf
 * weighs w_s[g] = tf * (logN - log(max(1, df[g]))); norm_s[n] = sqrt(sum w^2); len_s = max(len - 1, 0) (the number of bigram
 * positions: the scorer's quirk).  For hypothesis h and reference r, val[n] = sum over g in h of min(w_h[g], w_r[g]) * w_r[g], divided
 * by norm_h[n] * norm_r[n] if both are non-zero, times exp(-(len_h - len_r)^2 / (2 sigma^2)); the image scores
 * 10 * mean over n of (sum over r of val[n]) / R.  n_images = 1 gives 0; an n-gram of every image weighs 0; an n-gram of no reference
 * has df 0 and weighs tf * logN.
 * ROUGE-L (beta = 1.2): p = max over r of LCS(r, h) / len(h), q = max over r of LCS(r, h) / len(r) (an empty reference gives 0);
 * (1 + beta^2) p q / (q + beta^2 p) if both are non-zero, else 0; an empty hypothesis scores 0. */
#define SAT_NGRAM_TABLE_MAX_CAPACITY (1LL << 36)
size_t sat_ngram_table_bytes(int64_t capacity);   /* 0 (and a message) for a refused capacity */
int sat_ngram_table_clear(void* table, int64_t capacity, void* stream);
int sat_ngram_table_add(const int32_t* refs, const int32_t* ref_lengths, int32_t B, int32_t R, int32_t T, void* table, int64_t capacity,
                        int32_t* error_flag, void* stream);
int sat_caption_consensus(const int32_t* cap_tokens, const int32_t* cap_len, int32_t cap_width, const int32_t* refs, const int32_t* ref_lengths,
                          int32_t B, int32_t R, int32_t T, const void* table, int64_t capacity, int64_t n_images, double sigma,
                          double* scores /* (B, 2) */, void* stream);

/* ------------------------------------------------------------------ consensus (minimum-Bayes-risk) reranking of a beam
 * (sat_amd/metrics.py is the specification: consensus_utilities).  Image b has hyp_count[b] hypotheses (clamped into [0, K]) in
 * append order: hypothesis f = the first hyp_len[b][f] tokens (clamped into [0, width]) of hyp_tokens (B, K, width) -- the layout
 * sat_beam_hypotheses leaves -- with raw scores hyp_logp (B, K) float32 (fin_score).  Against a document-frequency table of n_images
 * images (above), with cider(i|j) / rouge(i|j) the CIDEr-D / ROUGE-L of hypothesis i taking hypothesis j as its single reference:
 *   gain(i|j) = w_cider * cider(i|j) + w_rouge * rouge(i|j)      a weight of 0 skips its term, and its work
 *   q_j       = exp(alpha * (s_j - max_k s_k)) in fp64           alpha = 0: every q_j = 1 and hyp_logp is not read (may be NULL)
 *   U_i       = (sum over j != i of q_j * gain(i|j)) / (sum over j != i of q_j), j ascending; 0 when the denominator is 0 (one hypothesis)
 *   winner    = the first i with U_i = max U (append order, as sat_beam_select breaks ties); 0 for an image without hypotheses
 * utilities (B, K) float64, 0.0 in the slots f >= hyp_count[b]; winner (B) int32, ready for sat_beam_select_at.  One launch, one
 * workgroup per image; fp64 throughout, every sum one thread's loop in a fixed order, no atomics: the same inputs give the same bits.
 * SAT_EINVAL before any launch: a null pointer, K > SAT_MBR_MAX_HYPS, width > SAT_CAPTION_MAX_LEN, a refused capacity, n_images < 1,
 * sigma <= 0, a weight or alpha that is negative or not finite, both weights 0, alpha != 0 without hyp_logp. */
#define SAT_MBR_MAX_HYPS 32
int sat_caption_mbr(const int32_t* hyp_tokens, const int32_t* hyp_len, const int32_t* hyp_count, const float* hyp_logp /* (B, K) or NULL */, int32_t B,
                    int32_t K, int32_t width, const void* table, int64_t capacity, int64_t n_images, double sigma, double w_cider, double w_rouge,
                    double alpha, double* utilities /* (B, K) */, int32_t* winner /* (B) */, void* stream);

/* ------------------------------------------------------------------ diversity of a beam: distinct-n, mBLEU (self-BLEU), unique captions
 * (sat_amd/metrics.py is the specification: diversity_stats, diversity_per_hypothesis, diversity_from_stats).  The hypotheses come in
 * sat_caption_mbr's layout: image b has hyp_count[b] of them (clamped into [0, K]) in append order, hypothesis f = the first
 * hyp_len[b][f] tokens (clamped into [0, width]) of hyp_tokens (B, K, width).  Tokens are compared as the n-gram keys above see them
 * (clamped into [0, 65534]): out-of-range input gives a wrong count, never a stray access.  stats (B, SAT_DIVERSITY_STATS) int32:
 *   [0..3]    distinct n-grams, n = 1..4, pooled over all hypotheses of the image
 *   [4..7]    n-gram positions pooled: the sum over hypotheses of max(len - n + 1, 0); [n-1] / [3+n] is distinct-n (0 positions: 0.0)
 *   [8]       number of hypotheses                 [9]  number of distinct hypotheses (equal token sequences; two empty ones count once)
 *   [10..13]  sum over hypotheses i of the clipped n-gram matches of i against all the OTHER hypotheses as references (corpus BLEU's
 *             numerator: per distinct n-gram min(count in i, largest count in another hypothesis)); duplicates and empty hypotheses
 *             stay among the others
 *   [14..17]  sum over i of max(1, len_i - n + 1), per segment as in sat_caption_stats [4..7]
 *   [18]      sum over i of len_i                  [19] sum over i of the closest other length (a tie goes to the shorter)
 * An image with fewer than 2 hypotheses has nothing to compare with: its columns 10..19 are 0.  per_hyp (B, K, 10) int32, optional:
 * for hypothesis f the columns [0..9] of sat_caption_stats with the other hypotheses as its references; all 0 in the slots
 * f >= hyp_count[b] and for an image with fewer than 2 hypotheses.  One launch, one workgroup per image: the n-gram positions of one
 * order are sorted in LDS by (n-gram, hypothesis) and everything is read off the sorted runs; integers only, no atomics: the same
 * input gives the same bits.  B == 0 returns SAT_OK without a launch.  SAT_EINVAL before any launch: a null pointer (per_hyp may be
 * NULL), B < 0, K < 1, K > SAT_MBR_MAX_HYPS, width < 1, width > SAT_CAPTION_MAX_LEN. */
#define SAT_DIVERSITY_STATS 20
int sat_caption_diversity(const int32_t* hyp_tokens, const int32_t* hyp_len, const int32_t* hyp_count, int32_t B, int32_t K, int32_t width,
                          int32_t* stats /* (B, 20) */, int32_t* per_hyp /* (B, K, 10) or NULL */, void* stream);
/* The vocabulary captions use: counts[t] += 1 for each of the first cap_len[b] tokens t (cap_len clamped into [0, cap_width]) of
 * cap_tokens (B, cap_width) that lies in [0, V); others are skipped.  counts (V) int32 is ADDED to (zero it before the first call).
 * Integer atomicAdd on global memory: a sum, the same whatever the order.  B == 0 returns SAT_OK without a launch.  SAT_EINVAL before
 * any launch: a null pointer, B < 0, V < 1, cap_width < 1 or above SAT_CAPTION_MAX_LEN. */
int sat_caption_vocab_usage(const int32_t* cap_tokens, const int32_t* cap_len, int32_t cap_width, int32_t B, int32_t V,
                            int32_t* counts /* (V), added to */, void* stream);

/* ------------------------------------------------------------------ chrF over the characters of the vocabulary's spelling
 * (sat_amd/metrics.py is the specification: chrf_text, chrf_stats, chrf_sentence, chrf; nltk's sentence_chrf with whitespace ignored).
 * Reference (b, r) and hypothesis b are sliced as in sat_caption_stats, with the same limits and SAT_EINVAL messages.  A sentence is
 * the concatenation of its tokens' spellings without a separator: token v spells word_chars[word_offsets[v] .. word_offsets[v + 1])
 * (int32 code points, whitespace already stripped; word_offsets (V + 1), ascending from 0); a token outside [0, V) contributes no
 * character.  max_word_chars bounds every word's length; cap_width * max_word_chars and (T - 1) * max_word_chars must not exceed
 * SAT_CHRF_MAX_CHARS, and beta must be positive and finite (SAT_EINVAL before any launch).  Offsets and lengths read from device memory
 * are clamped before they address anything ([0, min(word_offsets[V], V * max_word_chars)], a word to max_word_chars); characters
 * beyond SAT_CHRF_MAX_CHARS would be dropped, which only a misstated max_word_chars can reach.
 *   per reference and order n = 1..SAT_CHRF_MAX_ORDER, with Lh / Lr the hypothesis's / reference's characters:
 *     nh = max(Lh - n + 1, 0), nr = max(Lr - n + 1, 0), tp = sum over distinct character n-grams g of min(count_h(g), count_r(g));
 *     F_n = 1e-16 if nh, nr or tp is 0, else with p = tp / nh, q = tp / nr: ((1 + beta^2) * (p * q)) / (beta^2 * p + q), in fp64;
 *     the sentence scores (F_1 + ... + F_6) / 6, summed in ascending n;
 *   scores (B) float64: the maximum over the image's R references (the first maximum);
 *   stats (B, R, 8) int32, optional: tp_1..tp_6, Lh, Lr.
 * One launch, integer arithmetic up to the F-scores: the same input gives bit-identical scores. */
#define SAT_CHRF_MAX_ORDER 6
#define SAT_CHRF_MAX_CHARS 2048      /* code points per sentence */
int sat_caption_chrf(const int32_t* cap_tokens, const int32_t* cap_len, int32_t cap_width, const int32_t* refs, const int32_t* ref_lengths,
                     int32_t B, int32_t R, int32_t T, const int32_t* word_offsets, const int32_t* word_chars, int32_t V,
                     int32_t max_word_chars, double beta, double* scores /* (B) */, int32_t* stats /* (B, R, 8) or NULL */, void* stream);

/* out[c] = sum_r x[r*ld + c] in a fixed order (bias gradients).  scratch: ceil(rows/256)*cols floats */
int sat_colsum(const float* x, int64_t ld, int64_t rows, int32_t cols, float* out, float* scratch, void* stream);

/* ------------------------------------------------------------------ sub-module entry points
 * (drop-in for attention / init_lstm called on their own, e.g. from caption(), model.py:269,299) */
/* att_enc = ann * W_e^T (model.py:100), hoisted */
int sat_attention_precompute(const float* ann, const float* att_enc_w, float* U, int32_t B, int32_t L, int32_t D, int32_t A, void* stream);
/* one SoftAttention.forward + beta gate for N = B*R rows: hc (N, hc_ld) holds [q | beta | ...]; alphas (N, T1, L), written at `step`.
 * B, R, L, D, A, T1 >= 1, 0 <= step < T1, hc_ld >= A + D, else SAT_EINVAL.  Any D, A and alignment (they only select the kernel). */
int sat_attention_step_fwd(const float* ann, const float* U, const float* hc, int32_t hc_ld, const float* att_f,
                           const int32_t* lengths, int32_t step, float* alphas, int32_t T1, float* Z, float* XZ,
                           int32_t B, int32_t R, int32_t L, int32_t D, int32_t A, void* stream);

/* Backward of sat_attention_step_fwd (what autograd does for SoftAttention.forward + the gate product, model.py:94-109, 541).
 * dZ: gradient of the un-gated context Z (from DeepOutput), dXZ: gradient of the gated context beta * z (from the LSTM input).
 * Outputs: DZ (rows, D) = total gradient of z; dhc[:, 0:A] = gradient of q = h W_d^T, dhc[:, A:A+D] = gradient of the gate's
 * pre-activation; dU (B, L, A) and dwf_part (B, A) are ACCUMULATED (+=: zero them before the first step; attention.f_att.weight's
 * gradient is the column sum of dwf_part); da_scratch: (B*R, L) floats.  dalphas: external gradient of alphas (same layout) or NULL.
 * The annotation gradient is  dann = sat_attention_context_bwd(alphas, DZ) + dU * W_e  (the second term a GEMM). */
int sat_attention_step_bwd(const float* ann, const float* U, const float* hc, int32_t hc_ld, const float* att_f, const int32_t* lengths, int32_t step,
                           const float* alphas, const float* dalphas, int32_t T1, const float* Z, const float* dZ, const float* dXZ, float* DZ, float* dhc,
                           int32_t dhc_ld, float* dU, float* dwf_part, float* da_scratch, int32_t B, int32_t R, int32_t L, int32_t D, int32_t A, void* stream);
/* The two step entry points with the operands only the train loop used to reach; every extra pointer may be NULL, which gives the plain call.
 *   scores_scratch (B*R, L) floats: lets the forward run as the split pair (scores + context kernels) where the shape allows it;
 *   ann_bf16 (B, L, D): a bf16 copy of ann that the context / dalpha kernels stream instead of ann (products and sums stay fp32);
 *   xz_bf16 (B*R, D) / dhc_bf16 (B*R, dhc_ld): bf16 copies of XZ and of dhc[:, 0:A+D], written next to the fp32 outputs.
 * The bf16 operands exist in the split kernels only: a shape or view that the plan sends to the single launch refuses them (SAT_EINVAL). */
int sat_attention_step_fwd_ex(const float* ann, const float* U, const float* hc, int32_t hc_ld, const float* att_f,
                              const int32_t* lengths, int32_t step, float* alphas, int32_t T1, float* Z, float* XZ,
                              int32_t B, int32_t R, int32_t L, int32_t D, int32_t A,
                              float* scores_scratch, const void* ann_bf16, void* xz_bf16, void* stream);
int sat_attention_step_bwd_ex(const float* ann, const float* U, const float* hc, int32_t hc_ld, const float* att_f, const int32_t* lengths, int32_t step,
                              const float* alphas, const float* dalphas, int32_t T1, const float* Z, const float* dZ, const float* dXZ, float* DZ, float* dhc,
                              int32_t dhc_ld, float* dU, float* dwf_part, float* da_scratch, int32_t B, int32_t R, int32_t L, int32_t D, int32_t A,
                              const void* ann_bf16, void* dhc_bf16, void* stream);
/* The launch plan of one attention call (host arithmetic only, no device is touched; the launchers read the same function).
 * op: 0 sat_attention_step_fwd, 1 sat_attention_step_bwd, 2 sat_attention_context_bwd (A, hc_ld and flags are ignored).
 * flags: 1 a score / dalpha scratch is passed, 2 ann (and its bf16 copy) is 16-byte (8-byte) aligned, 4 hc, Z and XZ are 16-byte aligned
 * (forward only), 8 a bf16 operand is passed.
 * out: [0] form (0 split pair, 1 single launch), [1] caption rows per pass RN, [2] passes, [3] floats per annotation load VW,
 * [4] features per block of the forward (dchunk), [5] NQ and [6] Lq of the context backward, [7] dynamic LDS bytes of the scores /
 * dalpha / single kernel, [8] of the context / tanh kernel.  A shape no call accepts returns SAT_EINVAL and zeros. */
#define SAT_ATT_PLAN_SCRATCH 1
#define SAT_ATT_PLAN_ANN_ALIGNED 2
#define SAT_ATT_PLAN_ROWS_ALIGNED 4
#define SAT_ATT_PLAN_BF16 8
int sat_attention_step_plan(int32_t op, int32_t B, int32_t R, int32_t L, int32_t D, int32_t A, int32_t hc_ld, int32_t T1, int32_t flags, int32_t out[9]);
/* dann[b, l, :] (+)= sum over the image's R captions and their live steps t < lengths of alphas[b*R + r, t, l] * DZ[t, b*R + r, :]
 * (alphas (B*R, T1, L); DZ time-major (T1, B*R, D)) */
int sat_attention_context_bwd(const float* alphas, const float* DZ, const int32_t* lengths, float* dann, int32_t accumulate, int32_t B, int32_t R, int32_t T1,
                              int32_t L, int32_t D, void* stream);
/* nn.LSTM, one layer, one time step for N rows (model.py:175-180, called with seq_len 1 at model.py:326, 544).  x (N, in), weights in
 * torch's layout (4n, in) / (4n, n), gate order i,f,g,o.  `gates` (N, 4n) receives the ACTIVATED gates, the only tensor backward needs
 * besides the states.  bias_scratch: 4n floats.  Backward: dx, dh_prev, dc_prev and the four parameter gradients are overwritten;
 * dc_new may be NULL (no gradient into the new cell state); dgates (N, 4n) and scratch (ceil(N/256) * 4n floats) are work space. */
int sat_lstm_cell_fwd(const float* x, int32_t in, const float* h_prev, const float* c_prev, const float* w_ih, const float* w_hh, const float* b_ih,
                      const float* b_hh, float* gates, float* h_new, float* c_new, float* bias_scratch, int32_t N, int32_t n, void* stream);
int sat_lstm_cell_bwd(const float* x, int32_t in, const float* h_prev, const float* c_prev, const float* c_new, const float* gates, const float* dh_new,
                      const float* dc_new, const float* w_ih, const float* w_hh, float* dx, float* dh_prev, float* dc_prev, float* dw_ih, float* dw_hh,
                      float* db_ih, float* db_hh, float* dgates, float* scratch, int32_t N, int32_t n, void* stream);
/* DeepOutput.forward (model.py:125-131): logits = (dropout(tanh(prev_embed + hidden W_h^T + context W_c^T))) W_o^T + b_o; context = NULL is the
 * shallow form (x = hidden W_h^T; prev_embed unused).  u (N, m) keeps x for backward, udrop (N, m) the dropped copy (dropout > 0 only; masks =
 * counter-based hash of (seed, element), the same in backward).  Backward overwrites every output; d_prev_embed doubles as the (N, m) work
 * buffer in the shallow form; db_out may be NULL (weight tying); scratch: ceil(N/256) * V floats. */
int sat_deep_output_fwd(const float* prev_embed, const float* hidden, const float* context, const float* w_hidden, const float* w_context, const float* w_out,
                        const float* b_out, float dropout, uint64_t seed, float* u, float* udrop, float* logits, int32_t N, int32_t m, int32_t n, int32_t D,
                        int32_t V, void* stream);
int sat_deep_output_bwd(const float* dlogits, const float* hidden, const float* context, const float* u, const float* udrop, const float* w_hidden,
                        const float* w_context, const float* w_out, float dropout, uint64_t seed, float* d_prev_embed, float* d_hidden, float* d_context,
                        float* dw_hidden, float* dw_context, float* dw_out, float* db_out, float* scratch, int32_t N, int32_t m, int32_t n, int32_t D, int32_t V,
                        void* stream);
/* InitLSTM.forward (model.py:76-81) for N annotation rows (N, L, D): mean over L -> dropout -> factorize -> init.  `init` (N, n2 = 2 n layers)
 * row-major IS the reference's (2 layers, N, n) buffer: its `.reshape` without a permute is a reinterpretation, h0 = the first
 * layers*N*n floats, c0 = the rest.  mean (N, D) (after dropout) and f (N, m) are kept for backward, which overwrites the four parameter
 * gradients and dann (N, L, D); df (N, m), dmean (N, D), scratch (ceil(N/256) * max(n2, m) floats) are work space. */
int sat_init_lstm_fwd(const float* ann, const float* w_f, const float* b_f, const float* w_i, const float* b_i, float dropout, uint64_t seed, float* mean, float* f,
                      float* init, int32_t N, int32_t L, int32_t D, int32_t m, int32_t n2, void* stream);
int sat_init_lstm_bwd(const float* dinit, const float* mean, const float* f, const float* w_f, const float* w_i, float dropout, uint64_t seed, float* dw_f,
                      float* db_f, float* dw_i, float* db_i, float* dann, float* df, float* dmean, float* scratch, int32_t N, int32_t L, int32_t D, int32_t m,
                      int32_t n2, void* stream);

/* nn.Embedding(V, m, max_norm, padding_idx) as the reference calls it (model.py:158-164; uses at 298, 526).  Forward: rows of `table`
 * gathered by token id (-1, and any other id outside [0, V) = zero row: the ids the backward skips); max_norm > 0 first renormalises,
 * IN PLACE like torch, the table rows that occur in `tokens` (flags_scratch: V ints).  Backward: dtable fully overwritten; rows of dY
 * are added per vocabulary row in increasing row order (no floating-point atomics), the padding row stays zero; scratch:
 * 3 V + 1 + rows ints. */
int sat_embedding_fwd(float* table, const int32_t* tokens, float* out, int32_t rows, int32_t V, int32_t m, float max_norm, int32_t* flags_scratch, void* stream);
int sat_embedding_bwd(const float* dY, const int32_t* tokens, float* dtable, int32_t rows, int32_t V, int32_t m, int32_t padding_idx, int32_t* scratch, void* stream);
/* backward of the beta gate's Sigmoid (model.py:187-192): dpre = dy * y * (1 - y); the Linear around it is sat_gemm_f32 (epi 2 forward) */
int sat_sigmoid_bwd(const float* dy, const float* y, float* dpre, int64_t n, void* stream);

/* ------------------------------------------------------------------ encoder (get_encoder, model.py:16-63)
 * The reference builds the encoder from torchvision ResNet layers (model.py:19-29) + Normalize
 * (model.py:59) + an optional 1x1 Conv2d with bias (model.py:53).  These entry points are the layers
 * of that nn.Sequential on NHWC fp32 activations and KRSC filters. */
typedef struct sat_conv_geom {
    int32_t N, H, W, C;     /* input  (N, H, W, C), C % 4 == 0                    */
    int32_t K, R, S;        /* filter (K, R, S, C), K % 4 == 0                    */
    int32_t stride, pad;    /* output (N, P, Q, K), P = (H + 2 pad - R)/stride + 1 */
    int32_t stride_w;       /* 0: = stride.  Otherwise the horizontal stride (bf16 forward / weight gradient only): the stem's tap-pair view.
                             * The fp32 forward / weight gradient and every data gradient return SAT_EINVAL for a stride_w that differs from stride */
} sat_conv_geom;
/* nn.Conv2d forward / autograd (input gradient, weight gradient) as implicit GEMMs on MFMA */
int sat_conv2d_fwd(const float* x, const float* w, const float* bias /* or NULL */, float* y, const sat_conv_geom* g, void* stream);
int sat_conv2d_dgrad(const float* dy, const float* w, float* dx, const sat_conv_geom* g, int32_t accumulate, void* stream);
int sat_conv2d_wgrad(const float* dy, const float* x, float* dw, const sat_conv_geom* g, float* slab, int64_t slab_elems, void* stream);
size_t sat_conv2d_wgrad_slab_bytes(const sat_conv_geom* g);
/* bf16 storage variants (activations and filters bf16 in HBM, C % 8 == 0 and K % 8 == 0): bf16 MFMA, fp32
 * accumulation; the weight gradient is produced in fp32 (master weights stay fp32). */
int sat_conv2d_fwd_bf16(const void* x, const void* w, const float* bias, void* y, const sat_conv_geom* g, void* stream);
/* forward that also leaves BatchNorm statistics of its (bf16-rounded) output: per row tile of *tile_rows output pixels and per
 * filter the fp32 (sum, sum of squares) -> tile_stats[tile][K][2] (sat_conv2d_fwd_stats_bytes).  *tile_rows = 0 when the launch
 * went to a kernel without that epilogue (the caller then takes sat_bn_train_fwd_t).  sat_bn_train_fwd_tiles_bf16 is
 * sat_bn_train_fwd_t(dtype = bf16) without the statistics pass over x. */
size_t sat_conv2d_fwd_stats_bytes(const sat_conv_geom* g);
int sat_conv2d_fwd_bf16_stats(const void* x, const void* w, void* y, const sat_conv_geom* g, float* tile_stats, int32_t* tile_rows, void* stream);
int sat_bn_train_fwd_tiles_bf16(const void* x, int64_t rows, int32_t C, const float* tile_stats, int32_t tile_rows, const float* gamma,
                                const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* save_mean,
                                float* save_invstd, const void* residual, int32_t relu, void* y, uint8_t* relu_mask, float* scratch, void* stream);
/* The same with the residual given RAW: residual_raw is the input of another train-mode BatchNorm (the projection shortcut of a ResNet block,
 * statistics already in res_mean / res_invstd); y = relu(bn(x) + bn_res(residual_raw)) with the shortcut's normalised value rounded to bf16 as if it had
 * been stored, but never written.  Bit-identical to sat_bn_train_fwd_tiles_bf16 on the materialised shortcut. */
int sat_bn_train_fwd_tiles_bf16_resbn(const void* x, int64_t rows, int32_t C, const float* tile_stats, int32_t tile_rows, const float* gamma, const float* beta,
                                      float eps, float momentum, float* running_mean, float* running_var, float* save_mean, float* save_invstd,
                                      const void* residual_raw, const float* res_mean, const float* res_invstd, const float* res_gamma, const float* res_beta,
                                      int32_t relu, void* y, uint8_t* relu_mask, float* scratch, void* stream);
int sat_conv2d_dgrad_bf16(const void* dy, const void* w, void* dx, const sat_conv_geom* g, int32_t accumulate, void* stream);
/* Data gradient that also leaves the BACKWARD statistics of the BatchNorm in front of this convolution: dx is the gradient of that
 * BatchNorm's (ReLU'd) output, so with its input bn_x (same NHWC shape as dx), the forward's ReLU sign mask (or NULL: no ReLU) and its
 * saved mean / invstd, the epilogue adds up per row tile and channel (sum g, sum g * xhat), g = the stored dx masked by the sign bits ->
 * tile_stats[tile][C][2] (sat_conv2d_dgrad_stats_bytes).  sat_bn_train_bwd_tiles_bf16 is sat_bn_train_bwd_t(dtype = bf16) without the
 * statistics pass over dy and x.  *tile_rows = 0 when the launch could not produce them (stride 2, odd shapes): take sat_bn_train_bwd_t.
 * With accumulate = 1 the statistics are those of the accumulated dx. */
size_t sat_conv2d_dgrad_stats_bytes(const sat_conv_geom* g);
int sat_conv2d_dgrad_bf16_bnstats(const void* dy, const void* w, void* dx, const sat_conv_geom* g, int32_t accumulate, const void* bn_x,
                                  const uint8_t* bn_relu_mask, const float* bn_mean, const float* bn_invstd, float* tile_stats, int32_t* tile_rows, void* stream);
/* The same launch joining a residual block's identity path: dx = dgrad(dy, w) + add_src, add_src (bf16, dx's shape: the gradient that arrived at
 * the block's output) gated per element by the bits of add_mask (the block's final ReLU sign mask, or NULL) - the masked gradient is never
 * written out on its own (torchvision Bottleneck / BasicBlock backward: out = relu(bn(...) + identity), model.py:19-29).  stride 1 only.
 * bn_x = NULL: no statistics (the other bn_* / tile_* arguments are ignored). */
int sat_conv2d_dgrad_bf16_fused(const void* dy, const void* w, void* dx, const sat_conv_geom* g, const void* add_src, const uint8_t* add_mask, const void* bn_x,
                                const uint8_t* bn_relu_mask, const float* bn_mean, const float* bn_invstd, float* tile_stats, int32_t* tile_rows, void* stream);
int sat_bn_train_bwd_tiles_bf16(const void* dy, const void* x, int64_t rows, int32_t C, const float* tile_stats, int32_t tile_rows, const float* save_mean,
                                const float* save_invstd, const float* gamma, int32_t relu, void* dx, float* dgamma, float* dbeta, void* dres,
                                int32_t dres_accumulate, const uint8_t* relu_mask, float* scratch, void* stream);
int sat_conv2d_wgrad_bf16(const void* dy, const void* x, float* dw, const sat_conv_geom* g, float* slab, int64_t slab_elems, void* stream);
/* ---- the residual-block loop of the trunk inside the library (training, bf16 storage; csrc/encoder_loop.hip) --------------------------------
 * Replaces, per block, the ~10 forward and ~14 backward per-layer calls above (and the tensor allocations between them) that a host-side
 * driver of torchvision's BasicBlock / Bottleneck (inside `self.encoder(img)`, model.py:19-29, 483, and its autograd) would issue: ONE call
 * for the forward of a run of blocks, ONE for their backward, over one activation arena whose layout is a pure function of the descriptors.
 * The loop calls the same per-layer entry points in the same order: results are bit-identical to driving them one by one.
 * Pointers: filters are the bf16 KRSC copies the convolutions read; BatchNorm index 0..3 = bn1, bn2, bn3 (bottleneck only), downsample's;
 * gradient destinations are fp32 (filters KRSC).  Backward only: dw* / dgamma / dbeta.                                                      */
typedef struct sat_block_desc {
    int32_t kind;                 /* 0 = BasicBlock (3x3, 3x3), 1 = Bottleneck (1x1, 3x3 strided, 1x1)                       */
    int32_t stride, cin, mid, cout, has_ds;
    int32_t N, H, W;              /* the block's input map (N, H, W, cin)                                                     */
    int32_t fwd_res_bn;           /* projection blocks: the shortcut's BatchNorm applied inside the last BatchNorm's kernel   */
    int32_t dgrad_join;           /* the block's input gradient joins identity + conv path inside the data-gradient launch    */
    int32_t bn_bwd_epilogue;      /* BatchNorm-backward statistics out of the data-gradient epilogues                         */
    const void *w1, *w2, *w3, *wd;
    const float* gamma[4]; const float* beta[4]; float* running_mean[4]; float* running_var[4]; float eps[4]; float momentum[4];
    float *dw1, *dw2, *dw3, *dwd; float* dgamma[4]; float* dbeta[4];
} sat_block_desc;
size_t sat_encoder_blocks_arena_bytes(const sat_block_desc* blocks, int32_t nblocks);
/* x: bf16 (N, H, W, cin) input of blocks[0]; *out_ptr = the last block's output inside the arena; bn_scratch: sat_bn_scratch_bytes of the largest map */
int sat_encoder_blocks_fwd(const sat_block_desc* blocks, int32_t nblocks, const void* x, void* arena, size_t arena_bytes, float* bn_scratch, void** out_ptr,
                           void* stream);
/* Backward of blocks [last .. first], descending (the whole trunk, or one ResNet stage at a time so that a gradient exchange can start per stage).
 * dout: bf16 gradient of block `last`'s output; dout_tiles / dout_tile_rows: the BatchNorm-backward statistics that came with it from the previous
 * call (NULL / 0 for the first call).  *dx_ptr = gradient of block `first`'s input inside the arena, *dx_tiles / *dx_tile_rows its statistics.
 * side_stream (or NULL): the weight gradients are launched there (fork / join through `event`, a hipEvent_t of the caller; joined before the call
 * returns), with their own split-K scratch.                                                                                                   */
int sat_encoder_blocks_bwd(const sat_block_desc* blocks, int32_t nblocks, int32_t first, int32_t last, const void* x, void* arena, size_t arena_bytes, const void* dout,
                           const float* dout_tiles, int32_t dout_tile_rows, float* bn_scratch, float* slab_main, int64_t slab_main_elems, float* slab_side,
                           int64_t slab_side_elems, void* side_stream, void* event, void** dx_ptr, float** dx_tiles, int32_t* dx_tile_rows, void* stream);

/* ResNet stem tail in one pass (model.py:19-29 keeps torchvision's bn1 -> relu -> maxpool): BatchNorm(train statistics already in
 * mean / invstd: sat_bn_train_fwd_t with y = NULL computes them and updates the running statistics) + ReLU + MaxPool2d(3, 2, 1)
 * of the NHWC convolution output x (N, H, W, C) -> y_pool (N, P, Q, C), argmax (same shape, bytes: window position of the first
 * maximum).  The backward takes the pooled gradient and returns dx, dgamma, dbeta; the full-size BatchNorm output, its sign
 * mask and the dense pre-pool gradient are never materialised.  scratch: sat_bn_scratch_bytes(N * H * W, C). */
int sat_stem_tail_fwd_t(int32_t dtype, const void* x, int32_t N, int32_t H, int32_t W, int32_t C, const float* mean, const float* invstd, const float* gamma,
                        const float* beta, void* y_pool, uint8_t* argmax, void* stream);
int sat_stem_tail_bwd_t(int32_t dtype, const void* dy_pool, const uint8_t* argmax, const void* x, int32_t N, int32_t H, int32_t W, int32_t C, const float* mean,
                        const float* invstd, const float* gamma, const float* beta, void* dx, float* dgamma, float* dbeta, float* scratch, void* stream);
/* torchvision Normalize(mean, std) (model.py:59) fused with NCHW -> NHWC and 3 -> 4 channel padding */
int sat_image_normalize_nhwc4(const float* img_nchw, float* out_nhwc4, int32_t N, int32_t H, int32_t W,
                              const float* mean3_host, const float* std3_host, void* stream);
/* bf16 stem as a 7 x 4 convolution over PAIRS of pixels (model.py:19-29 keeps torchvision's conv1: 7x7, stride 2, pad 3, 3 channels).
 * With 4 stored channels a pixel is 8 bytes, so the 16 bytes one lane gathers hold two horizontally adjacent pixels = two filter
 * taps.  The normalised image is written zero-padded by 3 on every side, (N, H + 6, W + 6, 4) bf16; viewed as (N, H + 6, (W + 6) / 2, 8)
 * the stem is R = 7, S = 4, C = 8, stride 2 vertically and 1 horizontally (stride_w), no padding: 224 products per output instead
 * of the 392 of an 8-channel layout (5 of 8 channels zero).  W must be even.  filter_pairs: (K, 7, 7, 3) fp32 -> (K, 7, 4, 8) bf16
 * (tap 2s in slots 0-2, tap 2s + 1 in slots 4-6, the eighth tap and slots 3 / 7 zero); grad_unpairs: its fp32 gradient back. */
int sat_image_normalize_nhwc4_padded_bf16(const float* img_nchw, void* out, int32_t N, int32_t H, int32_t W, const float* mean3_host, const float* std3_host, void* stream);
int sat_stem_filter_pairs(const float* w3, void* w_pairs_bf16, int32_t K, void* stream);
/* resnext archs (model.py:28 keeps torchvision's resnext50_32x4d / resnext101_32x8d in the ResNet branch): their 3x3 convolutions have `groups`
 * groups.  The grouped filter (K, R, S, C / groups; fp32 or bf16) is expanded into the dense block-diagonal filter (K, R, S, C) that
 * sat_conv2d_* read, and the gradient of the grouped filter is gathered from the diagonal blocks of the dense filter's fp32 gradient.       */
int sat_grouped_filter_expand(const void* w_grouped, void* w_dense, int32_t K, int32_t C, int32_t RS, int32_t groups, int32_t bf16, void* stream);
int sat_grouped_filter_grad_extract(const float* dw_dense, float* dw_grouped, int32_t K, int32_t C, int32_t RS, int32_t groups, void* stream);
int sat_stem_filter_grad_unpairs(const float* dw_pairs, float* dw3, int32_t K, void* stream);
/* ShuffleNetV2 trunk (the reference's CLI default --encoder_arch shufflenet_v2_x0_5, train.py:43; model.py:30-31 keeps torchvision's
 * conv1, maxpool, stage2-4, conv5).  dtype: 0 = fp32, 1 = bf16 activations; NHWC; C a multiple of 4 (fp32) / 8 (bf16).
 *   depthwise 3x3, pad 1, stride 1 | 2 (InvertedResidual.depthwise_conv): w = the (C, 1, 3, 3) fp32 parameter as it lies in memory ([C][9],
 *     master weights in both modes); fp32 accumulation.  wgrad: fp32 dw [C][9] from per-chunk partial sums added in a fixed order
 *     (scratch: sat_dwconv3x3_wgrad_scratch_bytes);
 *   channel_shuffle(cat(a, b), groups = 2) of two (rows, Ch) branches: element c of the result = (c odd ? b : a)[c / 2].  join writes
 *     either `full` (rows, 2 Ch), or - full == NULL - its two halves x1 = [:, :Ch], x2 = [:, Ch:] as separate dense tensors (what the
 *     next stride-1 unit's x.chunk(2, dim = 1) reads); split is the backward: (d full | its halves) -> (da, db).
 *     Ch = the real branch width, Chp >= Ch (a multiple of 4) the width of the branch tensors and of the halves in memory: channels past Ch
 *     are zero padding and stay zero (x1_0 / x2_0: 58- / 122-channel branches held in 64 / 128); `full` has (2 Ch rounded up to 8) channels. */
int sat_dwconv3x3_fwd_t(int32_t dtype, const void* x, const float* w, void* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t stride, void* stream);
int sat_dwconv3x3_dgrad_t(int32_t dtype, const void* dy, const float* w, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t stride, void* stream);
size_t sat_dwconv3x3_wgrad_scratch_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t stride);
int sat_dwconv3x3_wgrad_t(int32_t dtype, const void* dy, const void* x, float* dw, int32_t N, int32_t H, int32_t W, int32_t C, int32_t stride,
                          float* scratch, void* stream);
/* The launch plan the three entry points above take for a shape, without touching a device (callable on a machine without a GPU).
 * op: 0 forward, 1 data gradient, 2 filter gradient.  out = {form (0 generic kernel, 1 rolling window over the rows of a column),
 * rows per thread R, channel vectors per block cvb, partial [9][C] slices in the scratch}; cvb and the slices are 0 for op 0 and 1, R is 1
 * for the generic filter-gradient form.  Validates like the entry points (C % 4 | 8 by dtype, stride 1 | 2, positive sizes).            */
int sat_dwconv3x3_plan(int32_t op, int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t stride, int32_t out[4]);
int sat_shuffle_join_t(int32_t dtype, const void* a, const void* b, void* full, void* x1, void* x2, int64_t rows, int32_t Ch, int32_t Chp, void* stream);
int sat_shuffle_split_t(int32_t dtype, const void* dfull, const void* dx1, const void* dx2, void* da, void* db, int64_t rows, int32_t Ch, int32_t Chp, void* stream);
/* bf16 -> fp32 copy (n % 8 == 0): the annotations of a bf16 trunk without the 1x1 projection (encoder_dim == trunk width, model.py:56-57) */
int sat_cast_bf16_to_f32(const void* src, float* dst, int64_t n, void* stream);
/* (pixels, 3) <-> (pixels, 4) zero padded; used for the stem filters */
int sat_pad_channels_3to4(const float* src, float* dst, int64_t pixels, int32_t inverse, void* stream);
/* nn.BatchNorm2d in training mode over a (rows, C) NHWC view, fused with the residual add and ReLU of the
 * ResNet blocks.  scratch: sat_bn_scratch_bytes(rows, C).  Updates running stats like PyTorch. */
size_t sat_bn_scratch_bytes(int64_t rows, int32_t C);
int sat_bn_train_fwd(const float* x, int64_t rows, int32_t C, const float* gamma, const float* beta, float eps, float momentum,
                     float* running_mean, float* running_var, float* save_mean, float* save_invstd,
                     const float* residual /* or NULL */, int32_t relu, float* y, float* scratch, void* stream);
/* eval-mode BatchNorm: y = (x - running_mean) / sqrt(running_var + eps) * gamma + beta (+ residual)(ReLU) */
int sat_bn_eval_fwd(const float* x, int64_t rows, int32_t C, const float* running_mean, const float* running_var, float eps,
                    const float* gamma, const float* beta, const float* residual, int32_t relu, float* y, void* stream);
/* backward: dy is the gradient of the fused output y; dres (optional) receives the gradient of the residual input */
int sat_bn_train_bwd(const float* dy, const float* x, const float* y, int64_t rows, int32_t C, const float* save_mean,
                     const float* save_invstd, const float* gamma, int32_t relu, float* dx, float* dgamma, float* dbeta,
                     float* dres, int32_t dres_accumulate, float* scratch, void* stream);
/* Storage-typed variants (dtype 0 = fp32, 1 = bf16 activations; statistics, affine parameters and their
 * gradients stay fp32, reductions accumulate in double) */
int sat_bn_train_fwd_t(int32_t dtype, const void* x, int64_t rows, int32_t C, const float* gamma, const float* beta, float eps, float momentum,
                       float* running_mean, float* running_var, float* save_mean, float* save_invstd,
                       const void* residual, int32_t relu, void* y,
                       uint8_t* relu_mask /* or NULL; rows*C/8 bytes, C % 8 == 0: bit i of byte b = (element 8b+i of y > 0); relu == 2 (ReLU6,
                                             mobilenet_v2: y clamped to [0, 6]): bit = (0 < pre-clamp value < 6), i.e. "the gradient passes" */,
                       float* scratch, void* stream);
int sat_bn_eval_fwd_t(int32_t dtype, const void* x, int64_t rows, int32_t C, const float* running_mean, const float* running_var, float eps,
                      const float* gamma, const float* beta, const void* residual, int32_t relu, void* y, void* stream);
int sat_bn_train_bwd_t(int32_t dtype, const void* dy, const void* x, const void* y, int64_t rows, int32_t C, const float* save_mean,
                       const float* save_invstd, const float* gamma, int32_t relu, void* dx, float* dgamma, float* dbeta,
                       void* dres, int32_t dres_accumulate,
                       const uint8_t* relu_mask /* or NULL: the forward's sign mask, read instead of y (which may then be NULL) */,
                       float* scratch, void* stream);
/* The launch plan a training-mode BatchNorm call takes for a shape, without touching a device (callable on a machine without a GPU).  It is
 * the function the launchers and sat_bn_scratch_bytes read, under the current bn_vpt / bn_onepass debug options and the SAT_BN_* environment
 * values latched at first use.  backward: 0 forward, 1 backward; dtype: 0 fp32, 1 bf16; tile_rows: 0 = statistics from a pass over the
 * activation (sat_bn_train_fwd_t / _bwd_t), > 0 = from ceil(rows / tile_rows) tile statistics (the *_tiles_bf16 entry points, bf16 only);
 * resbn: 1 = sat_bn_train_fwd_tiles_bf16_resbn (forward on tile statistics only).  out =
 *   [0] statistics form: 0 column-statistics pass + finalize, 1 tile finish <8 channels, 8 loads>, 2 tile finish <4, 16>, 3 fused tile
 *       finalize (forward only), 4 tile reduce + finalize pair
 *   [1] CV: vector columns (16 bytes each) per block of the column pass, a divisor of 256; channels per block for the tile forms
 *   [2] blocks along the channels
 *   [3] row parts = partials per channel in the scratch (form 4: tile parts; forms 1 - 3 finish in one launch: 0)
 *   [4] rows per part; -1 = groups of rows dealt round-robin to the parts (backward pass); form 4: tiles per part; forms 1 - 3: 0
 *   [5] tiles (0 for form 0)
 *   [6] apply kernel: vectors per thread VPT (1, 2, 4)   [7] ... which lie ceil(rows / VPT) rows apart (the last part is short when VPT
 *       does not divide rows)
 * Validates like the entry points (positive sizes, C % 4 | 8 by dtype); on an error out is all zero. */
int sat_bn_plan(int32_t backward, int32_t dtype, int64_t rows, int32_t C, int32_t tile_rows, int32_t resbn, int64_t out[8]);
int sat_maxpool3x3s2_fwd_t(int32_t dtype, const void* x, void* y, uint8_t* argmax, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
int sat_maxpool3x3s2_bwd_t(int32_t dtype, const void* dy, const uint8_t* argmax, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
/* bf16 plumbing: fp32 -> bf16 copies of filters/gradients (n % 4 == 0); Normalize fused with NCHW -> NHWC and
 * 3 -> 8 channel padding; stem filter (K,7,7,3) fp32 -> (K,7,7,8) bf16 and its fp32 gradient back */
int sat_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
int sat_image_normalize_nhwc8_bf16(const float* img_nchw, void* out_nhwc8, int32_t N, int32_t H, int32_t W,
                                   const float* mean3_host, const float* std3_host, void* stream);
int sat_stem_filter_pad(const float* w3, void* w8_bf16, int64_t pixels, void* stream);
int sat_stem_filter_grad_unpad(const float* dw8, float* dw3, int64_t pixels, void* stream);
/* nn.MaxPool2d(3, 2, 1) of the ResNet stem; argmax (N,P,Q,C) bytes keep the window position */
int sat_maxpool3x3s2_fwd(const float* x, float* y, uint8_t* argmax, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
int sat_maxpool3x3s2_bwd(const float* dy, const uint8_t* argmax, float* dx, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
/* encoder_size option (readme.md:118-121): AdaptiveAvgPool2d when P <= H, bilinear Upsample(align_corners=False) otherwise */
int sat_resize_fwd(const float* x, float* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t P, int32_t Q, void* stream);
int sat_resize_bwd(const float* dy, float* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t P, int32_t Q, void* stream);

/* ------------------------------------------------------------------ optimizer (SAT.configure_optimizers, model.py:723-757;
 * gradient clipping train.py:93-96,273-274): every parameter tensor updated by one launch.
 * `tensors` and `chunks` are DEVICE arrays built by the caller: one sat_opt_tensor per parameter (its gradient pointer
 * changes per step), one sat_opt_chunk per sat_optimizer_chunk_elems() elements of a tensor. */
#define SAT_OPT_SGD 0
#define SAT_OPT_ADAM 1
#define SAT_OPT_ADAMW 2
typedef struct sat_opt_tensor {
    float* p; const float* g;
    float* m;             /* Adam exp_avg / SGD momentum_buffer (NULL when unused) */
    float* v;             /* Adam exp_avg_sq                                       */
    int64_t n;
    float lr, weight_decay;    /* of the parameter's group                        */
    void* shadow_bf16;         /* or NULL: the updated parameter is also written here as bf16 (same element order): the
                                  filter copies the bf16 convolutions read, kept current without a cast pass per step */
} sat_opt_tensor;
typedef struct sat_opt_chunk { int32_t tensor; int32_t reserved; int64_t start; } sat_opt_chunk;
typedef struct sat_opt_hyper {
    int32_t kind;              /* SAT_OPT_*                                            */
    int32_t nesterov, first_step;   /* SGD: nesterov momentum; first step (momentum buffer = gradient) */
    float beta1, beta2, eps;
    float bias_correction1;         /* 1 - beta1^step                                  */
    float bias_correction2_sqrt;    /* sqrt(1 - beta2^step)                            */
    float momentum;
    float clip_value;               /* > 0: clamp every gradient element to [-v, v] (clip_grad_value_: +-inf become +-v, a NaN stays NaN) */
} sat_opt_hyper;
int32_t sat_optimizer_chunk_elems(void);
/* coef[0] = min(1, max_norm / (||g||_2 + 1e-6)) over ALL tensors (clip_grad_norm_), coef[1] = the norm; fixed-order reduction.
 * Non-finite gradients as in torch: a NaN anywhere makes the norm AND the coefficient NaN, so the step that reads coef[0] writes NaN
 * into every element of every tensor (a diverged run shows, it does not train on); an infinite norm gives coefficient 0.           */
int sat_grad_clip_coef(const sat_opt_tensor* tensors, const sat_opt_chunk* chunks, int32_t n_chunks, float max_norm, double* scratch,
                       float* coef, void* stream);
/* p, m, v updated in place from g * clip_coef[0] (clip_coef NULL = 1) */
int sat_optimizer_step(const sat_opt_tensor* tensors, const sat_opt_chunk* chunks, int32_t n_chunks, const sat_opt_hyper* hyper,
                       const float* clip_coef, void* stream);
/* the same launch with the hyper-parameters in DEVICE memory (one sat_opt_hyper): a captured / replayed launch (hipGraph) then follows the
 * step count (bias corrections) and the clipping settings that the host writes there before every replay (sat_amd/graph.py)            */
int sat_optimizer_step_dev(const sat_opt_tensor* tensors, const sat_opt_chunk* chunks, int32_t n_chunks, const sat_opt_hyper* hyper_dev,
                           const float* clip_coef, void* stream);
/* ---- averaged weights (sat_amd/optim.py: kind="asgd", ema_decay=): the average is taken in the pass that updates p.
 * `avg` is a DEVICE array of one float* per sat_opt_tensor (same order; NULL = this tensor keeps no average), each in the
 * element order of its p.  After the update of an element:   a = (coef == 1) ? p : a + (p - a) * coef   (coef exactly 1
 * stores p itself).  EMA over SGD / Adam / AdamW: coef = 1 - decay (1 on the first step: the average starts as a copy).
 * SAT_OPT_ASGD is torch.optim.ASGD:  g += weight_decay * p;  p = p * (1 - lambd * eta) - eta * g  with the tensor's step size
 * eta in sat_opt_tensor.lr (m and v are not read), coef = mu.  The kind is accepted by the _avg entry points only;
 * sat_optimizer_step / _dev and their kernel are what they were.  8 more bytes per element than the plain step, no launch more. */
#define SAT_OPT_ASGD 3
typedef struct sat_opt_avg_hyper {
    float coef;                /* in [0, 1]                                             */
    float lambd;               /* >= 0; SAT_OPT_ASGD only                               */
    int32_t flags, reserved;   /* 0                                                     */
} sat_opt_avg_hyper;
/* validated on the host before the launch: null tables, coef outside [0, 1], lambd < 0, an unknown kind -> SAT_EINVAL */
int sat_optimizer_step_avg(const sat_opt_tensor* tensors, float* const* avg, const sat_opt_chunk* chunks, int32_t n_chunks,
                           const sat_opt_hyper* hyper, const sat_opt_avg_hyper* avg_hyper, const float* clip_coef, void* stream);
/* both hyper blocks in DEVICE memory (graph replay, as sat_optimizer_step_dev).  The host cannot read them here, so only the
 * tables are validated: the caller checks coef / lambd / kind before it writes them there (FusedOptimizer does).          */
int sat_optimizer_step_avg_dev(const sat_opt_tensor* tensors, float* const* avg, const sat_opt_chunk* chunks, int32_t n_chunks,
                               const sat_opt_hyper* hyper_dev, const sat_opt_avg_hyper* avg_hyper_dev, const float* clip_coef,
                               void* stream);
/* p <-> its average, element by element, for every tensor whose avg entry is not NULL (g, m, v, lr of the table are not
 * read); shadow_bf16, where set, is rewritten from the values that now sit in p.  Twice restores every bit.              */
int sat_optimizer_swap(const sat_opt_tensor* tensors, float* const* avg, const sat_opt_chunk* chunks, int32_t n_chunks, void* stream);

/* ---- input pipeline on device ------------------------------------------------------------------------
 * Replaces, per batch, the per-sample PIL / torchvision chain of train.py:208-233: T.RandomResizedCrop | T.Resize +
 * T.CenterCrop (Pillow's antialiased BILINEAR Image.resize, bit exact), T.RandomHorizontalFlip, T.ToTensor, and
 * util.py:121-130 AddGaussianNoise.  Input: the decoded pictures of one batch, uint8 RGB (height, width, 3), concatenated
 * in one device buffer; one descriptor per picture (the random draws are the caller's: torch RNG on the host).
 * Output: (n, 3, out_h, out_w) fp32 in [0, 1] (+ noise * std) - the `img` of the reference's batch (util.py:40-45).      */
typedef struct sat_image_desc {
    int64_t offset;                                    /* byte offset of the picture in `pixels`                        */
    int32_t height, width;
    int32_t crop_top, crop_left, crop_h, crop_w;       /* box cut out first (PIL crop)                                  */
    int32_t resized_h, resized_w;                      /* size the box is resampled to (PIL resize, BILINEAR)           */
    int32_t out_top, out_left;                         /* (out_h, out_w) window of the resampled picture (T.CenterCrop) */
    int32_t flip;                                      /* mirror left-right                                             */
    int32_t reserved;
} sat_image_desc;
size_t sat_image_batch_workspace_bytes(const sat_image_desc* desc_host, int32_t n, int32_t out_h, int32_t out_w);
/* desc_host / desc_dev: the same n descriptors in host memory (validated, sizes the launch) and in device memory (read by
 * the kernels).  noise: (n, 3, out_h, out_w) standard normal draws or NULL.  out_u8 (optional): the (n, out_h, out_w, 3)
 * bytes before ToTensor, i.e. what PIL would hold.  At least one of out_nchw / out_u8.  pixels_bytes bounds the offsets. */
int sat_image_batch_transform(const uint8_t* pixels, int64_t pixels_bytes, const sat_image_desc* desc_host, const sat_image_desc* desc_dev,
                              int32_t n, int32_t out_h, int32_t out_w, const float* noise, float noise_std, float* out_nchw,
                              uint8_t* out_u8, void* workspace, size_t workspace_bytes, void* stream);
/* T.ColorJitter(brightness, contrast, saturation, hue) of train.py:223-224 on the resampled (and mirrored) bytes, before
 * ToTensor and noise: the four PIL adjustments of torchvision's functional_pil (ImageEnhance.Brightness / Contrast / Color,
 * adjust_hue's HSV round trip), bit exact.  One per picture:
 *   order       a permutation of 0..3 (0 brightness, 1 contrast, 2 saturation, 3 hue), applied first to last
 *   brightness, contrast, saturation   blend factors, finite and >= 0
 *   hue_shift   trunc(hue_factor * 255), in [-128, 127]: added to the HSV hue byte modulo 256
 * jitter_host / jitter_dev: the same n records in host memory (validated) and device memory; NULL / NULL is
 * sat_image_batch_transform.  The workspace (sat_image_batch_jitter_workspace_bytes) also holds the bytes in front of the
 * contrast step and each picture's luma sum. */
typedef struct sat_image_jitter {
    int32_t order[4];
    float brightness, contrast, saturation;
    int32_t hue_shift;
} sat_image_jitter;
size_t sat_image_batch_jitter_workspace_bytes(const sat_image_desc* desc_host, const sat_image_jitter* jitter_host, int32_t n, int32_t out_h,
                                              int32_t out_w);
int sat_image_batch_transform_jitter(const uint8_t* pixels, int64_t pixels_bytes, const sat_image_desc* desc_host, const sat_image_desc* desc_dev,
                                     const sat_image_jitter* jitter_host, const sat_image_jitter* jitter_dev, int32_t n, int32_t out_h,
                                     int32_t out_w, const float* noise, float noise_std, float* out_nchw, uint8_t* out_u8, void* workspace,
                                     size_t workspace_bytes, void* stream);
/* The "optical" augmentation of train.py:225-231 (T.RandomChoice of RandomPerspective, RandomAffine, RandomRotation) on the
 * S x S bytes after ColorJitter, before ToTensor and noise: Pillow's Image.transform of the picture onto itself with fill 0,
 * bit exact.  One record per picture, Pillow's inverse map (output pixel -> input point):
 *   kind 0   affine map, NEAREST (RandomAffine, RandomRotation): coeffs[0..5], sampled in Pillow's 16.16 fixed point;
 *            |x*c0 + y*c1 + c2| and |x*c3 + y*c4 + c5| must be below 32768 at the four corners (0,0) (W,0) (0,H) (W,H),
 *            where Pillow takes that path
 *   kind 1   perspective map, BILINEAR (RandomPerspective): coeffs[0..7], sampled in double
 * Every coefficient must be finite.  warp_host / warp_dev: the same n records in host memory (validated) and device memory;
 * NULL / NULL is sat_image_batch_transform_jitter.  jitter_host / jitter_dev NULL / NULL: no ColorJitter.  The workspace
 * (sat_image_batch_warp_workspace_bytes) also holds the bytes in front of the warp. */
typedef struct sat_image_warp {
    int32_t kind;
    int32_t reserved;
    double coeffs[8];
} sat_image_warp;
size_t sat_image_batch_warp_workspace_bytes(const sat_image_desc* desc_host, const sat_image_jitter* jitter_host, const sat_image_warp* warp_host,
                                            int32_t n, int32_t out_h, int32_t out_w);
int sat_image_batch_transform_warp(const uint8_t* pixels, int64_t pixels_bytes, const sat_image_desc* desc_host, const sat_image_desc* desc_dev,
                                   const sat_image_jitter* jitter_host, const sat_image_jitter* jitter_dev, const sat_image_warp* warp_host,
                                   const sat_image_warp* warp_dev, int32_t n, int32_t out_h, int32_t out_w, const float* noise, float noise_std,
                                   float* out_nchw, uint8_t* out_u8, void* workspace, size_t workspace_bytes, void* stream);

/* ---- baseline JPEG decoding on device ---------------------------------------------------------------------------------
 * The step in front of the transform: util.py:136-137's Image.open(f).convert("RGB") for Huffman-coded sequential 8-bit
 * files (SOF0 / SOF1) with one scan of 1 (grayscale) or 3 YCbCr components, luma sampled h1v1, h2v1 or h2v2 and chroma
 * 1x1, with or without restart markers; bit exact with libjpeg-turbo's defaults (JDCT_ISLOW, fancy upsampling).  The
 * host parses the headers (sat_amd/jpeg.py) and sends every other file to Pillow (progressive files: the section after
 * this one, on request).  Three stages: entropy decoding,
 * dequantisation + ISLOW IDCT (per block), upsampling + YCbCr->RGB (per pixel).  Entropy decoding gives every restart
 * segment one thread; a restart-free picture (n_segments == 1) of at least parallel_min_bytes of data is instead cut into
 * subsequences of subseq_bytes raw bytes, each decoded by a thread of its own: a speculative pass from (slot 0, DC next),
 * a self-synchronisation loop in which every thread decodes again from its predecessor's exit state until no state
 * changes (one workgroup per picture, no host round trip), a prefix sum of the completed blocks, a write pass and a
 * prefix sum of the DC differences.  A picture on which that comes up short (a marker in the data, an unverified chain, a
 * wrong block count, a bad code met while writing) is cleared and decoded by the one-thread path in the same call, so
 * status words and pixels never depend on the path.  No host synchronisation, allocation or read-back inside the call.
 * The (height, width, 3) bytes of each picture are written at its out_offset in `pixels`.
 *   data_offset, data_bytes   the entropy-coded data of the scan in `compressed`, RST markers included, 0xFF00 stuffed
 *   segments_offset           byte offset in `compressed` of n_segments (start, end) uint32 pairs, 4-byte aligned: the
 *                             restart segments relative to data_offset, the markers themselves excluded
 *   restart_interval          MCUs per segment (DRI), 0: one segment
 *   block_offset, segment_base  coefficient blocks and segments of the pictures in front of this one (prefix sums; checked)
 *   quant, dc_table, ac_table per component (Y, Cb, Cr; a grayscale picture uses [0]): indices into the table arrays
 *   h_samp, v_samp            luma sampling factors (1,1) (2,1) (2,2); a grayscale picture uses (1,1)
 * status (n int32, device): 0, or an OR of 1 bad Huffman code, 2 ran out of data, 4 coefficient index past 63, 8 bad
 * segment bounds, 16 a marker inside a segment.  The rest of the batch is unaffected by a bad stream.                     */
typedef struct sat_jpeg_desc {
    int64_t data_offset, data_bytes, segments_offset, out_offset, block_offset;
    int32_t height, width, components, h_samp, v_samp, restart_interval, n_segments, segment_base;
    int32_t quant[3], dc_table[3], ac_table[3];
    int32_t reserved;
} sat_jpeg_desc;
typedef struct sat_jpeg_qtable {
    uint16_t q[64];                                    /* natural (row-major) order                                     */
} sat_jpeg_qtable;
typedef struct sat_jpeg_htable {
    uint16_t lookup[512];                              /* next 9 bits -> (length << 8) | symbol; 0: the code is longer   */
    int32_t maxcode[18];                               /* [l]: largest code of length l, -1 none; [17] = 0xFFFFF          */
    int32_t valoffset[18];                             /* symbol index = code + valoffset[l]                             */
    uint8_t huffval[256];
} sat_jpeg_htable;
size_t sat_jpeg_decode_workspace_bytes(const sat_jpeg_desc* desc_host, int32_t n);
int sat_jpeg_decode_batch(const uint8_t* compressed, int64_t compressed_bytes, const sat_jpeg_desc* desc_host, const sat_jpeg_desc* desc_dev,
                          int32_t n, const sat_jpeg_qtable* quant_dev, int32_t n_quant, const sat_jpeg_htable* huff_dev, int32_t n_huff,
                          uint8_t* pixels, int64_t pixels_bytes, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
/* The same two calls with options (NULL: the defaults, which is what the two calls above pass).
 *   subseq_bytes        0: SAT_JPEG_SUBSEQ_BYTES_DEFAULT; else a multiple of 4 from 16 to 2^20.  The grid is measured from
 *                       data_offset, stuffed bytes count; the workspace holds 24 bytes of state per subsequence.
 *   parallel_min_bytes  -1: SAT_JPEG_PARALLEL_MIN_BYTES_DEFAULT; 0: every restart-free picture; INT64_MAX: none.  (A
 *                       picture of more than 2^27 data bytes stays on the one-thread path.)
 *   info                NULL, or n x 4 int32 on the device, per picture: the path taken (0 one thread per segment,
 *                       1 subsequences, 2 subsequences abandoned for the one-thread path), its subsequences, the
 *                       synchronisation rounds run, 0.
 * SAT_EINVAL, before anything is enqueued: a bad subseq_bytes or parallel_min_bytes, null descriptors, a small workspace. */
#define SAT_JPEG_SUBSEQ_BYTES_DEFAULT 128
#define SAT_JPEG_PARALLEL_MIN_BYTES_DEFAULT 2048
typedef struct sat_jpeg_decode_opts {
    int32_t subseq_bytes;
    int32_t reserved;
    int64_t parallel_min_bytes;
    int32_t* info;
} sat_jpeg_decode_opts;
size_t sat_jpeg_decode_workspace_bytes_ex(const sat_jpeg_desc* desc_host, int32_t n, const sat_jpeg_decode_opts* opts);
int sat_jpeg_decode_batch_ex(const uint8_t* compressed, int64_t compressed_bytes, const sat_jpeg_desc* desc_host, const sat_jpeg_desc* desc_dev,
                             int32_t n, const sat_jpeg_qtable* quant_dev, int32_t n_quant, const sat_jpeg_htable* huff_dev, int32_t n_huff,
                             uint8_t* pixels, int64_t pixels_bytes, int32_t* status, void* workspace, size_t workspace_bytes, void* stream,
                             const sat_jpeg_decode_opts* opts);

/* ---- progressive JPEG decoding on device -------------------------------------------------------------------------------
 * The same step for Huffman-coded 8-bit progressive files (SOF2) whose scan script the host admits (sat_amd/jpeg.py,
 * parse(progressive=True): libjpeg's jpeg_simple_progression, the ten scans Pillow writes for YCbCr and the six for
 * grayscale, complete down to Al = 0, with or without restart markers; every other progressive file goes to Pillow).
 * Opt-in: nothing calls this unless the caller asks for progressive files on the GPU.
 * sat_jpeg_desc is reused for the geometry, the quantisation tables, out_offset and block_offset (prefix sums over the n
 * pictures of THIS call); its scan fields (data_*, segments_offset, restart_interval, n_segments, segment_base, dc_table,
 * ac_table) are ignored and reserved stays 0.  One sat_jpeg_scan per scan of every picture, ordered by level:
 *   picture                   index into desc
 *   level                     dependency level: 1 + the highest level of an earlier scan of the picture that touches one of
 *                             the same (component, coefficient) cells, 0 if none.  Non-decreasing along the array; the
 *                             scans of one level touch disjoint cells of a picture (the caller's promise).
 *   n_components, component   1 (a non-interleaved scan: the ceil(w_c / 8) x ceil(h_c / 8) blocks of that component in raster
 *                             order, which is what its restart interval counts) or all 3 in order 0, 1, 2 (DC scans only: the
 *                             padded MCU grid)
 *   ss, se, ah, al            band and successive-approximation bits: ss = se = 0 a DC scan, else 1 <= ss <= se <= 63;
 *                             ah = 0 a first scan, else a refinement with al = ah - 1
 *   dc_table, ac_table        indices into the Huffman tables as latched at the scan's SOS (dc_table per component of a DC
 *                             first scan, ac_table of an AC scan; the others are not read)
 *   restart_interval          MCUs of this scan per segment, 0: one segment
 *   data_offset, data_bytes, segments_offset, n_segments   as in sat_jpeg_desc, for this scan
 *   segment_base              segments of the scans in front of this one in the array (prefix sum; checked)
 * Stages: the coefficient blocks are cleared; one entropy launch per level with one lane per (scan, restart segment) running
 * jdphuff.c's DC-first / DC-refine / AC-first / AC-refine arithmetic, every read bounded by the lane's segment, every
 * coefficient index by se, every block by the scan's blocks; then the baseline path's IDCT and colour kernels.  status as
 * above (index past 63 reads: past se).  info: NULL or n x 4 int32 on the device, per picture (3, scans, levels, 0).
 * workspace: 192 bytes per coefficient block.  SAT_EINVAL, before anything is enqueued: null pointers, a small workspace,
 * scan records that do not fit their picture.  No host synchronisation, allocation or read-back inside the call.         */
typedef struct sat_jpeg_scan {
    int64_t data_offset, data_bytes, segments_offset;
    int32_t picture, level, n_components, component[3];
    int32_t ss, se, ah, al;
    int32_t dc_table[3], ac_table;
    int32_t restart_interval, n_segments, segment_base;
    int32_t reserved;
} sat_jpeg_scan;
size_t sat_jpeg_progressive_workspace_bytes(const sat_jpeg_desc* desc_host, int32_t n, const sat_jpeg_scan* scans_host, int32_t n_scans);
int sat_jpeg_decode_progressive_batch(const uint8_t* compressed, int64_t compressed_bytes, const sat_jpeg_desc* desc_host,
                                      const sat_jpeg_desc* desc_dev, int32_t n, const sat_jpeg_scan* scans_host, const sat_jpeg_scan* scans_dev,
                                      int32_t n_scans, const sat_jpeg_qtable* quant_dev, int32_t n_quant, const sat_jpeg_htable* huff_dev,
                                      int32_t n_huff, uint8_t* pixels, int64_t pixels_bytes, int32_t* status, void* workspace,
                                      size_t workspace_bytes, void* stream, int32_t* info);

/* ---- attention overlays on device (visualize.ipynb's make_visual) ------------------------------------------------------
 * The single-image front end of util.py:141-164: load_square = crop_center(min side) then Image.resize((S, S)) with no filter
 * named, which is Pillow's BICUBIC; prepare_image = the same once more, then T.ToTensor().  Bit exact with Pillow 12.2.
 * Input: n HWC uint8 pictures in `pixels`, one sat_image_desc each of which ONLY offset, height and width are read (the
 * bytes may be what sat_jpeg_decode_batch wrote).  The box is util.py's integer rule
 *   s = min(W, H);  left = (W - s) // 2;  top = (H - s) // 2     (right - left = lower - top = s for every parity)
 * and the resample is the code of sat_image_batch_transform (the same kernels, csrc/pillow_resample.h) with three differences:
 *   support = 2.0 * filterscale, so taps = ceil(support) * 2 + 1   (5 when enlarging, clipped at the borders)
 *   weight(x) = ((a + 2)|x| - (a + 3)) x^2 + 1  for |x| < 1,  (((|x| - 5)|x| + 8)|x| - 4) a  for |x| < 2,  else 0;  a = -0.5
 *   a negative coefficient is (int)(w 2^22 - 0.5): rounded away from zero, as the positive ones are
 * A box side above SAT_BICUBIC_MAX_SHRINK * S is SAT_EINVAL (129 taps at most, the table both filters share).
 * out_u8 (n, S, S, 3) and / or out_nchw (n, 3, S, S) = byte / 255 in fp32, one correctly rounded division (T.ToTensor()).
 * prepare_image(load_square(path, V), s) is two calls: the second reads the first's out_u8 through descriptors with
 * offset = i * V * V * 3 and height = width = V.  desc_host / desc_dev: the same records in host and device memory. */
#define SAT_BICUBIC_MAX_SHRINK 32
size_t sat_image_square_bicubic_workspace_bytes(const sat_image_desc* desc_host, int32_t n, int32_t S);
int sat_image_square_bicubic(const uint8_t* pixels, int64_t pixels_bytes, const sat_image_desc* desc_host, const sat_image_desc* desc_dev, int32_t n,
                             int32_t S, uint8_t* out_u8 /* or NULL */, float* out_nchw /* or NULL */, void* workspace, size_t workspace_bytes,
                             void* stream);
/* The panels of make_visual for B captioned pictures: square (B, V, V, 3) uint8, cap_alpha (B, Tmax, h * w) and cap_len (B) as
 * sat_beam_select leaves them (cap_len is clamped to [0, Tmax]) -> panels (B, Tmax + 2, V, V, 3) uint8.  With n = cap_len[b]:
 *   panel 0        the picture
 *   panel 1 + t    t < n: att = cap_alpha[b, t];  x = (att - min) / (max - min) in fp32;  x ** power (the host's powf: evaluated
 *                  in double, rounded once);  m = (uint8)(x * 255), truncated;  m enlarged from (h, w) to (V, V) by the BICUBIC
 *                  resample above (an L-mode resize: what the notebook's RGB resize of a grey mask gives in every channel);
 *                  byte = (uint8)(p + opacity * (m - p)) in fp32 without contraction, truncated = Image.blend(picture, mask, opacity)
 *   panel n + 1    "Total Attention": att = the fp32 sum of cap_alpha[b, 0..n-1] in step order, normalised the same way, no
 *                  power, enlarged, written to the three channels with no picture under it
 *   panels beyond  zero
 * max == min (a 1 x 1 map, the total of a blank caption; 0 / 0 in the notebook) gives a zero mask.
 * h * w <= SAT_ATTENTION_MAX_MAP, h <= V and w <= V (the mask is only ever enlarged), 0 <= opacity <= 1, power finite and > 0.
 * One launch; the masks live in LDS only. */
#define SAT_ATTENTION_MAX_MAP 256
int sat_attention_panels(const uint8_t* square, const float* cap_alpha, const int32_t* cap_len, int32_t B, int32_t Tmax, int32_t V, int32_t h,
                         int32_t w, float power, float opacity, uint8_t* panels, void* stream);

/* mobilenet_v3_small trunk (model.py:38-39 keeps torchvision's `features`; torchvision 0.10 _mobilenet_v3_conf("mobilenet_v3_small"), Howard et
 * al. 2019 table 2).  dtype: 0 = fp32, 1 = bf16 activations; NHWC; statistics, SE vectors, parameters and their gradients fp32.
 *   depthwise 5x5, pad 2, stride 1 | 2 (InvertedResidual's depthwise ConvBNActivation, kernel_size 5): as sat_dwconv3x3_*, C a multiple of 4
 *     in both storage types; w = the (C, 1, 5, 5) parameter in memory ([C][25]); wgrad: per-chunk partials added in a fixed order
 *     (scratch: sat_dwconv5x5_wgrad_scratch_bytes). */
int sat_dwconv5x5_fwd_t(int32_t dtype, const void* x, const float* w, void* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t stride, void* stream);
int sat_dwconv5x5_dgrad_t(int32_t dtype, const void* dy, const float* w, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t stride, void* stream);
size_t sat_dwconv5x5_wgrad_scratch_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t stride);
int sat_dwconv5x5_wgrad_t(int32_t dtype, const void* dy, const void* x, float* dw, int32_t N, int32_t H, int32_t W, int32_t C, int32_t stride,
                          float* scratch, void* stream);
/* BatchNorm2d + nn.Hardswish (ConvBNActivation with activation_layer = nn.Hardswish; BatchNorm2d(eps = 0.001, momentum = 0.01)):
 * y = v * min(max(v + 3, 0), 6) / 6 with v the BatchNorm output.  Training statistics (and running statistics) as sat_bn_train_fwd_t, or from
 * the producing bf16 convolution's tile statistics (tile_stats != NULL, as sat_bn_train_fwd_tiles_bf16).  The backward recomputes v from x,
 * mean, invstd, gamma and beta and takes torch's hardswish_backward: v <= -3 -> 0, v < 3 -> g (v / 3 + 0.5), else g.
 * scratch: sat_bn_scratch_bytes(rows, C).  C a multiple of 4 (fp32) / 8 (bf16). */
int sat_bn_hswish_train_fwd_t(int32_t dtype, const void* x, int64_t rows, int32_t C, const float* tile_stats /* or NULL */, int32_t tile_rows,
                              const float* gamma, const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                              float* save_mean, float* save_invstd, void* y, float* scratch, void* stream);
int sat_bn_hswish_eval_fwd_t(int32_t dtype, const void* x, int64_t rows, int32_t C, const float* running_mean, const float* running_var, float eps,
                             const float* gamma, const float* beta, void* y, void* stream);
int sat_bn_hswish_train_bwd_t(int32_t dtype, const void* dy, const void* x, int64_t rows, int32_t C, const float* save_mean, const float* save_invstd,
                              const float* gamma, const float* beta, void* dx, float* dgamma, float* dbeta, float* scratch, void* stream);
/* SqueezeExcitation (torchvision 0.10 mobilenetv3.py: fc1 / fc2 = 1x1 Conv2d with bias, squeeze width S): over x (N, HW, C),
 * pool = mean_hw x, h = relu(w1 pool + b1) (w1: (S, C)), z2 = w2 h + b2 (w2: (C, S)), s = hardsigmoid(z2), y = x * s.  pool / z2 / s: [N][C],
 * h: [N][S] fp32, written by the forward and read by the backward.  Backward: ds = sum_hw dy x, dz2 = ds / 6 where -3 < z2 < 3, the parameter
 * gradients summed over the images in order, dx = dy s + dpool / HW.  Every sum in a fixed order, no atomics.  C <= 1024, S <= 256;
 * scratch: sat_se_bwd_scratch_bytes(N, C, S). */
int sat_se_fwd_t(int32_t dtype, const void* x, int32_t N, int32_t HW, int32_t C, int32_t S, const float* w1, const float* b1, const float* w2, const float* b2,
                 float* pool, float* h, float* z2, float* s, void* y, void* stream);
size_t sat_se_bwd_scratch_bytes(int32_t N, int32_t C, int32_t S);
int sat_se_bwd_t(int32_t dtype, const void* dy, const void* x, int32_t N, int32_t HW, int32_t C, int32_t S, const float* w1, const float* w2, const float* pool,
                 const float* h, const float* z2, const float* s, void* dx, float* dw1, float* db1, float* dw2, float* db2, float* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SAT_HIP_H */
