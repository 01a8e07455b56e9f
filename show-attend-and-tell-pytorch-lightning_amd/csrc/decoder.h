// Internal C++ entry points of the decoder (wrapped by the C ABI in api.hip).
#pragma once
#include "../../include/sat_hip.h"
#include "common.h"

namespace sat {
struct Ws;
int check_dims(const sat_decoder_dims* d);
size_t decoder_workspace_bytes(const sat_decoder_dims& d, bool ln = false);      // ln: with what the layer-normalised cell saves
int decoder_fwd(const sat_decoder_dims& d, const sat_decoder_params& p, const sat_decoder_batch& b, float* logits, float* alphas,
                char* ws, size_t ws_bytes, hipStream_t st);
int decoder_bwd(const sat_decoder_dims& d, const sat_decoder_params& p, const sat_decoder_batch& b, const float* dlogits,
                const float* alphas, const float* dalphas, const sat_decoder_params& g, float* dann, char* ws, size_t ws_bytes, hipStream_t st,
                hipStream_t side = nullptr, hipEvent_t fork_event = nullptr,       // side: where the parameter gradients go (no join), see decoder.hip
                const float* reg_gscale = nullptr);                                // device (2): d loss / d (ar, tar), added into dHout in front of the time loop
// ar / tar of the top-layer states the last decoder_fwd left in ws (activation_reg.hip)
int decoder_reg_fwd(const sat_decoder_dims& d, const sat_decoder_batch& b, char* ws, size_t ws_bytes, void* scratch, float* out, hipStream_t st);
// weight-drop (decoder.hip): dst[l] = src[l] * s[layer0 + l] for `layers` matrices of `per` elements, s = dropout_scale(seed, 3, L * per + k, p);
// dst[l] may be src[l]; dstb (or its entries) may be NULL.  One launch.
int weight_drop(const float* const* src, float* const* dst, __bf16* const* dstb, int layers, long per, int layer0, float p, unsigned long long seed, hipStream_t st);
// the packing launch of the train step alone (layer 0: Wcat, its bf16 copy or NULL, bcat) under d.weight_drop / d.dropout_seed
int pack_weights_public(const sat_decoder_dims& d, const sat_decoder_params& p, float* wcat, void* wcat_b, float* bcat, hipStream_t st);
size_t activation_reg_scratch_bytes(int N, int T1, int n);
int activation_reg_fwd(const float* hidden, const int* lengths, int N, int T1, int n, long P, long Q, void* scratch, float* out, hipStream_t st);
int activation_reg_bwd(const float* hidden, const int* lengths, int N, int T1, int n, long P, long Q, const float* gscale, float* dH, hipStream_t st);
// launch plan of one attention step (decoder.hip: attention_plan decides it, the launchers and sat_attention_step_plan read it)
enum { ATT_OP_FWD = 0, ATT_OP_BWD = 1, ATT_OP_CONTEXT_BWD = 2 };
enum { ATT_FORM_SPLIT = 0, ATT_FORM_SINGLE = 1 };
enum : unsigned { ATT_HAS_SCRATCH = 1, ATT_ANN_ALIGNED = 2, ATT_ROWS_ALIGNED = 4, ATT_HAS_BF16 = 8 };
struct AttPlan {
    int form = 0, rn = 0, passes = 0;          // split pair or single launch; caption rows per pass; passes over the R rows of an image
    int vw = 0, dchunk = 0;                    // floats per annotation load; forward: features per block
    int nq = 0, lq = 0;                        // context backward: float4 per location slab, float4 per padded alphas row
    size_t lds0 = 0, lds1 = 0;                 // dynamic LDS bytes: scores | dalpha | the single kernel, and context | tanh
};
int attention_plan(int op, int R, int L, int D, int A, int hc_ld, int T1, unsigned flags, AttPlan& plan, const char* who);
int launch_attention_fwd(hipStream_t st, const float* ann, const float* U, const float* hc, int hc_ld, const float* wf,
                         const int* lengths, int step, float* alphas, int T1, float* Z, float* XZ, int B, int R, int L, int D, int A, float* sc, void* xzb,
                         const void* annb);
size_t decoder_infer_workspace_bytes(const sat_decoder_dims& d, int Kmax);
int decoder_infer_begin(const sat_decoder_dims& d, const sat_decoder_params& p, const float* ann, int K, int Kmax, float* h, float* c,
                        char* ws, size_t ws_bytes, hipStream_t st);
int decoder_infer_step(const sat_decoder_dims& d, const sat_decoder_params& p, const float* ann, const int* tokens, int K, int Kmax,
                       float* h, float* c, float* logits, float* alpha, const float* h_noise, char* ws, size_t ws_bytes, hipStream_t st);
size_t decoder_beam_workspace_bytes(const sat_decoder_dims& d, int K, int topg, int hist_stride, int groups);
int beam_groups_check(const sat_beam_groups* g, const char* what);
bool beam_history_on(const sat_beam_history* h);
int beam_history_check(const sat_beam_history* h, int max_gen_length, const char* what);
// one batched search, single-model or ensemble, described once (include/sat_hip.h, sat_beam_search_desc): the query returns the
// `total` the search compares its workspace against, and both refuse the same descriptors
int beam_search_workspace_bytes(const sat_beam_search_desc& s, size_t& total);
int beam_search(const sat_beam_search_desc& s, const sat_beam_search_out& o, char* ws, size_t ws_bytes, hipStream_t st);
int beam_required_check(const sat_beam_required* r, int K, int max_gen_length, const char* what);
int beam_ensemble_check_weights(const float* weight, int members, int combine, const char* what);
int beam_ensemble_check(const sat_beam_ensemble* e, const char* what);
size_t decoder_beam_ensemble_workspace_bytes(const sat_beam_ensemble& e, int K, int hist_stride);
int beam_ensemble_scores(const float* const* logits, const float* weight, int members, int combine, int rows, int V, float temperature, float* combined,
                         hipStream_t st);
int launch_attention_bwd(hipStream_t st, const float* ann, const float* U, const float* hc, int hc_ld, const float* wf, const int* lengths, int step,
                         const float* alphas, const float* dalphas, int T1, const float* Z, const float* dZ, const float* dXZ, float* DZ, float* dhc,
                         int dhc_ld, float* dU, float* dwf_part, float* da, int B, int R, int L, int D, int A, void* dhcb, const void* annb);
int attention_context_bwd(const float* alphas, const float* DZ, const int* lengths, float* dann, int accumulate, int B, int R, int T1, int L, int D, hipStream_t st);
int lstm_cell_fwd(const float* x, int in, const float* h_prev, const float* c_prev, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                  float* gates, float* h_new, float* c_new, float* bias_scratch, int N, int n, hipStream_t st);
int lstm_cell_bwd(const float* x, int in, const float* h_prev, const float* c_prev, const float* c_new, const float* gates, const float* dh_new, const float* dc_new,
                  const float* w_ih, const float* w_hh, float* dx, float* dh_prev, float* dc_prev, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh,
                  float* dgates, float* scratch, int N, int n, hipStream_t st);
int deep_output_fwd(const float* prev_embed, const float* hidden, const float* context, const float* w_hidden, const float* w_context, const float* w_out,
                    const float* b_out, float dropout, unsigned long long seed, float* u, float* udrop, float* logits, int N, int m, int n, int D, int V, hipStream_t st);
int deep_output_bwd(const float* dlogits, const float* hidden, const float* context, const float* u, const float* udrop, const float* w_hidden, const float* w_context,
                    const float* w_out, float dropout, unsigned long long seed, float* d_prev_embed, float* d_hidden, float* d_context, float* dw_hidden,
                    float* dw_context, float* dw_out, float* db_out, float* scratch, int N, int m, int n, int D, int V, hipStream_t st);
int init_lstm_fwd(const float* ann, const float* w_f, const float* b_f, const float* w_i, const float* b_i, float dropout, unsigned long long seed, float* mean,
                  float* f, float* init, int N, int L, int D, int m, int n2, hipStream_t st);
int init_lstm_bwd(const float* dinit, const float* mean, const float* f, const float* w_f, const float* w_i, float dropout, unsigned long long seed, float* dw_f,
                  float* db_f, float* dw_i, float* db_i, float* dann, float* df, float* dmean, float* scratch, int N, int L, int D, int m, int n2, hipStream_t st);
int embedding_fwd(float* table, const int* tokens, float* out, int rows, int V, int m, float max_norm, int* flags, hipStream_t st);
int embedding_bwd(const float* dY, const int* tokens, float* dtable, int rows, int V, int m, int padding_idx, int* scratch, hipStream_t st);
int sigmoid_bwd(const float* dy, const float* y, float* dpre, long n, hipStream_t st);
int beam_scores(const float* logits, int K, int V, float temperature, const int* masked, int n_masked, const float* parent, float* scores, hipStream_t st);
int beam_history_scores(const float* logits, int rows, int V, float temperature, const int* masked, int n_masked, const float* parent, const int* hist,
                        const int* hist_len, int hist_stride, const sat_beam_history& rules, int step, int end_id, float* scores, hipStream_t st);
int beam_group_select(const float* scores, const int* klive, int B, int K, int G, int V, int first_step, float lambda, float* work, float* values, int* indices,
                      hipStream_t st);
int beam_required_select(const float* scores, const int* klive, int B, int K, int V, const int* hist, int hist_stride, int hist_len, int first_step,
                         const sat_beam_required& req, int end_id, float* work, float* values, int* indices, hipStream_t st);
int topk(const float* x, float* work, long n, int k, float* values, int* indices, hipStream_t st);
int nucleus_keys(const float* scores, int rows, int V, float topp, float step, unsigned long long seed, unsigned long long stream, const float* gumbel,
                 float* keys, int* nucleus_size, hipStream_t st);
int colsum_public(const float* x, long ld, long rows, int cols, float* out, float* scratch, hipStream_t st);
int ce_fwd(const float* logits, const int* targets, int P, int V, float smoothing, float* lse_rows, float* loss_rows, int* correct_rows, float* out, hipStream_t st);
int ce_bwd(const float* logits, const int* targets, const float* lse_rows, int P, int V, float smoothing, const float* gscale, float* dlogits, hipStream_t st);
int ds_fwd(const float* alphas, int N, int T1, int L, float gamma, float* asum, float* part, float* out, hipStream_t st);
int ds_bwd(const float* asum, const float* gscale, int N, int T1, int L, float gamma, float* dalphas, hipStream_t st);
}  // namespace sat
