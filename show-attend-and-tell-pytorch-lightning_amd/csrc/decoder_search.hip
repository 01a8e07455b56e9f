// Host-side orchestration of caption decoding (model.py:255-448): one decoder start-up and one decode step, which the per-image entry
// points (SAT.beam_decode's host loop) and the batched searches both run; the batched search loop, single-model or ensemble, with its
// plans; and the search primitives that are entry points of their own.  Kernel launches only, everything in the caller's workspace.
#include "../../include/sat_hip.h"
#include "decoder_step.h"
#include "decoder_search_kernels.h"

namespace sat {

// ------------------------------------------------------------------ one decoder for every search: start-up and step
// A workspace is carved buffer by buffer, each rounded up to 256 bytes (base NULL: sizes only).
struct Carver {
    char* base; size_t off = 0;
    template <typename T> T* take(size_t elems) {
        const size_t o = off; off += (elems * sizeof(T) + 255) & ~(size_t)255;
        return base ? reinterpret_cast<T*>(base + o) : nullptr;
    }
};
// What a decode step needs besides the state: per image U = att_enc(ann), the annotation mean and InitLSTM's f / init vectors; the
// packed step weights; per row the [q | beta | gates] buffer, the context and its gated copy, the embedding, the deep-output sum,
// the stacked layers' gates and the attention scores.
struct StepWs { float *U, *Wcat, *bcat, *mean, *f, *init_img, *gu, *bup, *hc, *Z, *XZ, *Y, *u, *sc; };
static StepWs step_layout(const sat_decoder_dims& d, size_t images, size_t rows, Carver& cv) {
    StepWs w;
    const size_t HCW = d.A + d.D + 4 * (size_t)d.n;
    w.U = cv.take<float>(images * d.L * d.A); w.Wcat = cv.take<float>(HCW * d.n); w.bcat = cv.take<float>(HCW);
    w.mean = cv.take<float>(images * d.D); w.f = cv.take<float>(images * d.m); w.init_img = cv.take<float>(images * 2 * d.n * d.layers);
    w.gu = cv.take<float>(rows * 4 * d.n); w.bup = cv.take<float>((size_t)d.layers * 4 * d.n);
    w.hc = cv.take<float>(rows * HCW); w.Z = cv.take<float>(rows * d.D); w.XZ = cv.take<float>(rows * d.D);
    w.Y = cv.take<float>(rows * d.m); w.u = cv.take<float>(rows * d.m); w.sc = cv.take<float>(rows * d.L);
    return w;
}

// model.py:255-281, once per search: the packed step weights, att_enc, and the initial state h, c (layers, images * rows_per_image, n)
// of every row.  An image's rows are `groups` beams of rows_per_image / groups rows; the raw reshape of F3 depends on a beam's row count.
static int step_begin(const sat_decoder_dims& d, const sat_decoder_params& p, const float* ann, const StepWs& w, int images, int rows_per_image, int groups, float* h,
                      float* c, hipStream_t st) {
    t_bf16_mfma = d.precision ? 1 : 0;
    SAT_TRY(pack_step_weights(d, p, w.Wcat, nullptr, w.bcat, w.bup, st));
    SAT_TRY(image_begin(d, p, ann, images, w.U, w.mean, w.f, w.init_img, st));
    hipLaunchKernelGGL(init_expand_beams_kernel, dim3(cdiv(2L * d.layers * images * rows_per_image * d.n, 256)), dim3(256), 0, st, w.init_img, h, c, images, groups,
                       rows_per_image / groups, d.n, d.layers);
    return launch_ok("init_expand_beams");
}

// model.py:298-327 for all rows: embedding -> attention -> beta gate -> LSTM (-> stacked layers) -> deep output.  logits (rows, V) and the
// attention maps alpha (rows, L) from the tokens and h, c, which are updated in place; rows with live[i] == 0 get zero attention and
// carry their state.  noise (layers, rows, n) or NULL is decoder_noise (model.py:322-324): it joins h after attention and the gate were
// taken from the clean state, so it reaches the step through the recurrent products only, gates += noise * W_hh^T (the GEMM is linear
// in h).  The gate columns accumulate in the order hh (with bias), noise, embedding half, context half.
static int step_run(const sat_decoder_dims& d, const sat_decoder_params& p, const float* ann, const StepWs& w, const int* tok, float* h, float* c, const int* live,
                    int images, int rows_per_image, const float* noise, float* alpha, float* logits, hipStream_t st) {
    t_bf16_mfma = d.precision ? 1 : 0;
    const int N = images * rows_per_image, n = d.n, A = d.A, D = d.D, m = d.m, NL = d.layers, HCW = A + D + 4 * n;
    const long KS = (long)N * n;
    float* htop = h + (NL - 1) * KS;
    float* gates = w.hc + A + D;
    const float* w_hh = w.Wcat + (long)(A + D) * n;
    SAT_TRY(embedding_fwd(p.embedding, tok, w.Y, N, d.V, m, 0.f, nullptr, st));
    // attention and the gate read the TOP layer's state (h[-1], model.py:533,538); the recurrent term of layer 0 reads layer 0's
    if (NL == 1) {
        SAT_TRY(gemm(st, A_ROW, B_ROW, h, n, w.Wcat, n, w.hc, HCW, N, HCW, n, 0, EPI_BIAS_SIGMOID_RANGE, w.bcat, nullptr, nullptr, nullptr, 0, A, A + D));
    } else {
        SAT_TRY(gemm(st, A_ROW, B_ROW, htop, n, w.Wcat, n, w.hc, HCW, N, A + D, n, 0, EPI_BIAS_SIGMOID_RANGE, w.bcat, nullptr, nullptr, nullptr, 0, A, A + D));
        SAT_TRY(gemm(st, A_ROW, B_ROW, h, n, w_hh, n, gates, HCW, N, 4 * n, n, 0, EPI_BIAS, w.bcat + A + D));
    }
    SAT_TRY(launch_attention_fwd(st, ann, w.U, w.hc, HCW, p.att_f, live, 0, alpha, 1, w.Z, w.XZ, images, rows_per_image, d.L, D, A, w.sc, nullptr, nullptr));
    if (noise) SAT_TRY(gemm(st, A_ROW, B_ROW, noise, n, w_hh, n, gates, HCW, N, 4 * n, n, 1));
    SAT_TRY(gemm(st, A_ROW, B_ROW, w.Y, m, p.w_ih, m + D, gates, HCW, N, 4 * n, m, 1));
    SAT_TRY(gemm(st, A_ROW, B_ROW, w.XZ, D, p.w_ih + m, m + D, gates, HCW, N, 4 * n, D, 1));
    const bool ln = ln_on(p);                   // the layer-normalised cell: the same launch count, nothing saved
    LnCell lc = ln ? ln_layer(p, 0) : LnCell();
    SAT_TRY(lstm_cell_pointwise(gates, HCW, c, h, c, h, live, N, n, st, ln ? &lc : nullptr));
    for (int l = 1; l < NL; ++l) {              // stacked layers: input = the layer below's new h (nn.LSTM, no inter-layer dropout)
        float* hl = h + l * KS; float* cl = c + l * KS;
        SAT_TRY(gemm(st, A_ROW, B_ROW, hl - KS, n, p.up_w_ih[l - 1], n, w.gu, 4 * n, N, 4 * n, n, 0, EPI_BIAS, w.bup + (long)(l - 1) * 4 * n));
        SAT_TRY(gemm(st, A_ROW, B_ROW, hl, n, p.up_w_hh[l - 1], n, w.gu, 4 * n, N, 4 * n, n, 1));
        if (noise) SAT_TRY(gemm(st, A_ROW, B_ROW, noise + l * KS, n, p.up_w_hh[l - 1], n, w.gu, 4 * n, N, 4 * n, n, 1));
        if (ln) lc = ln_layer(p, l);
        SAT_TRY(lstm_cell_pointwise(w.gu, 4 * n, cl, hl, cl, hl, live, N, n, st, ln ? &lc : nullptr));
    }
    SAT_TRY(gemm(st, A_ROW, B_ROW, htop, n, p.out_hidden, n, w.u, m, N, m, n));
    if (d.deep_output) SAT_TRY(gemm(st, A_ROW, B_ROW, w.Z, D, p.out_context, D, w.u, m, N, m, D, 1, EPI_ADD_TANH, nullptr, nullptr, nullptr, w.Y, m));
    return gemm(st, A_ROW, B_ROW, w.u, m, p.out_w, m, logits, d.V, N, d.V, m, 0, p.out_b ? EPI_BIAS : EPI_NONE, p.out_b);
}

// ------------------------------------------------------------------ per-image entry points: one image, K <= Kmax live rows, the loop on the host
struct InferWs { size_t total; StepWs s; int* ones; };
static InferWs infer_layout(const sat_decoder_dims& d, int Kmax, char* base) {
    InferWs w; Carver cv{base};
    w.s = step_layout(d, 1, Kmax, cv);
    w.ones = cv.take<int>(Kmax);                 // every row the host passes is live
    w.total = cv.off;
    return w;
}
size_t decoder_infer_workspace_bytes(const sat_decoder_dims& d, int Kmax) { return infer_layout(d, Kmax, nullptr).total; }

int decoder_infer_begin(const sat_decoder_dims& d, const sat_decoder_params& p, const float* ann, int K, int Kmax, float* h, float* c,
                        char* ws, size_t ws_bytes, hipStream_t st) {
    InferWs w = infer_layout(d, Kmax, ws);
    SAT_REQUIRE(ws_bytes >= w.total && K >= 1 && K <= Kmax, "decoder_infer_begin: workspace %zu < %zu or bad beam count %d/%d", ws_bytes, w.total, K, Kmax);
    hipLaunchKernelGGL(fill_int_kernel, dim3(cdiv(Kmax, 256)), dim3(256), 0, st, w.ones, (long)Kmax, 1);
    SAT_TRY(launch_ok("fill ones"));
    return step_begin(d, p, ann, w.s, 1, K, 1, h, c, st);
}

int decoder_infer_step(const sat_decoder_dims& d, const sat_decoder_params& p, const float* ann, const int* tokens, int K, int Kmax,
                       float* h, float* c, float* logits, float* alpha, const float* h_noise, char* ws, size_t ws_bytes, hipStream_t st) {
    InferWs w = infer_layout(d, Kmax, ws);
    SAT_REQUIRE(ws_bytes >= w.total && K >= 1 && K <= Kmax, "decoder_infer_step: workspace or beam count");
    return step_run(d, p, ann, w.s, tokens, h, c, w.ones, 1, K, h_noise, alpha, logits, st);
}

// ------------------------------------------------------------------ batched beam search: every image of the batch at once
// (the reference loops over images, model.py:260).  Rows (B, K); the per-image semantics -- F3 initial
// states, top-k over the live beams' flattened scores, completed hypotheses leaving the beam, cut at max_gen_length -- are
// those of model.py:262-448; the whole loop is enqueued without a host round trip and leaves a back-trace
// (token and parent row of every step, attention maps, finished list) for the host to read once.
struct BeamWs {
    size_t total; StepWs s; float *h, *c, *h2, *c2, *logits, *scores, *work, *keys, *noise, *vals, *top;
    int *live, *klive, *inds, *gmap, *mask_first, *mask_rest;
    float* cand_val; int* cand_idx;        // top-g clipping only: (B*K, topg) candidates, after everything the plain search uses
    int *hist_a, *hist_b;                  // history rules only: (B*K, hist_stride) words every row has said, double-buffered, after the candidates
    int *g_count, *g_step, *g_row; float *g_score, *g_mean;   // groups only: the finished lists of the (image, group) pairs, (B*G) and (B*G, K/G)
};
static BeamWs beam_layout(const sat_decoder_dims& d, int K, char* base, int topg = 0, int hist_stride = 0, int groups = 1) {
    BeamWs w; Carver cv{base};
    const size_t N = (size_t)d.B * K, state = (size_t)d.layers * N * d.n;
    w.s = step_layout(d, d.B, N, cv);
    w.h = cv.take<float>(state); w.c = cv.take<float>(state); w.h2 = cv.take<float>(state); w.c2 = cv.take<float>(state);
    w.logits = cv.take<float>(N * d.V); w.scores = cv.take<float>(N * d.V); w.work = cv.take<float>(N * d.V); w.keys = cv.take<float>(N * d.V);
    w.noise = cv.take<float>(state);
    w.vals = cv.take<float>(N); w.top = cv.take<float>(N);
    w.live = cv.take<int>(N); w.klive = cv.take<int>((size_t)d.B * groups); w.inds = cv.take<int>(N); w.gmap = cv.take<int>(N);
    w.mask_first = cv.take<int>(4); w.mask_rest = cv.take<int>(4);
    w.cand_val = nullptr; w.cand_idx = nullptr;
    if (topg > 0) { w.cand_val = cv.take<float>(N * topg); w.cand_idx = cv.take<int>(N * topg); }
    w.hist_a = nullptr; w.hist_b = nullptr;
    if (hist_stride > 0) { w.hist_a = cv.take<int>(N * hist_stride); w.hist_b = cv.take<int>(N * hist_stride); }
    w.g_count = w.g_step = w.g_row = nullptr; w.g_score = w.g_mean = nullptr;
    if (groups > 1) {
        w.g_count = cv.take<int>((size_t)d.B * groups); w.g_step = cv.take<int>(N); w.g_row = cv.take<int>(N); w.g_score = cv.take<float>(N); w.g_mean = cv.take<float>(N);
    }
    w.total = cv.off;
    return w;
}
size_t decoder_beam_workspace_bytes(const sat_decoder_dims& d, int K, int topg, int hist_stride, int groups) {
    return beam_layout(d, K, nullptr, topg, hist_stride, groups < 1 ? 1 : groups).total;
}

// sat_beam_history: which rules are on, and are they well-formed (include/sat_hip.h)
bool beam_history_on(const sat_beam_history* h) {
    return h && (h->no_repeat_ngram != 0 || h->min_length != 0 || (h->repetition_penalty != 0.f && h->repetition_penalty != 1.0f));
}
int beam_history_check(const sat_beam_history* h, int max_gen_length, const char* what) {
    if (!h) return SAT_OK;
    SAT_REQUIRE(h->no_repeat_ngram >= 0, "%s: no_repeat_ngram %d is negative (0 = off)", what, h->no_repeat_ngram);
    SAT_REQUIRE(h->min_length >= 0 && (max_gen_length < 0 || h->min_length <= max_gen_length), "%s: min_length %d outside 0..max_gen_length=%d", what,
                h->min_length, max_gen_length);
    const float t = h->repetition_penalty;
    SAT_REQUIRE(t == 0.f ? !__builtin_signbit(t) : (t > 0.f && t < INFINITY), "%s: repetition_penalty %g is not a positive finite number (1 = off)", what, (double)t);
    return SAT_OK;
}
static int not_capturing(hipStream_t st, const char* what) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
    SAT_REQUIRE(cap == hipStreamCaptureStatusNone, "%s: not replayed from a graph (the stream is being captured)", what);
    return SAT_OK;
}

// the keys of one free step of a sampled search, (step, row, word): "nucleus", or "multinomial" / "topk" (method 1 reads its table by
// word, method 2 by rank)
static int launch_sample_keys(hipStream_t st, const float* scores, const int* klive, int N, int K, int V, const sat_beam_sampling& smp, int step, float* keys) {
    if (smp.method == SAT_SAMPLE_NUCLEUS) {
        hipLaunchKernelGGL(beam_nucleus_keys_kernel, dim3(N), dim3(256), 0, st, scores, klive, K, V, smp.sample_topp, (float)step, (unsigned long long)smp.seed,
                           (unsigned long long)step, smp.gumbel ? smp.gumbel + (long)step * N * V : (const float*)nullptr, keys, (int*)nullptr);
        return launch_ok("beam_nucleus_keys");
    }
    const int gstride = smp.method == 1 ? V : smp.sample_topk;
    hipLaunchKernelGGL(beam_sample_keys_kernel, dim3(N), dim3(256), 0, st, scores, klive, K, V, smp.method, smp.sample_topk, (float)step,
                       (unsigned long long)smp.seed, (unsigned long long)step, smp.gumbel ? smp.gumbel + (long)step * N * gstride : (const float*)nullptr, gstride,
                       keys);
    return launch_ok("beam_sample_keys");
}

// words (floats or ints) cleared by a launch
static void beam_zero_words(hipStream_t st, void* dst, long n_) {
    hipLaunchKernelGGL(fill_int_kernel, dim3(cdiv(n_, 256)), dim3(256), 0, st, reinterpret_cast<int*>(dst), n_, 0);
}
// The three parts of the batched search that belong to ONE model; the ensemble search (decoder_beam_ensemble) runs them once per member.
// once per batch: the decoder's start-up for the K copies (G groups of K / G) of every image, and the masks
static int beam_member_begin(const sat_decoder_dims& d, const sat_decoder_params& p, const float* ann, const BeamWs& w, int K, int G, const int* special_host,
                             hipStream_t st) {
    const int START = special_host[0], PAD = special_host[1], END = special_host[2], UNK = special_host[3];
    hipLaunchKernelGGL(set4_int_kernel, dim3(1), dim3(1), 0, st, w.mask_first, START, PAD, END, UNK);
    hipLaunchKernelGGL(set4_int_kernel, dim3(1), dim3(1), 0, st, w.mask_rest, START, PAD, -1, -1);
    SAT_TRY(launch_ok("beam masks"));
    return step_begin(d, p, ann, w.s, d.B, K, G, w.h, w.c, st);
}
// one decode step of one model for all rows: w.logits (N, V) and the attention maps alpha (N, L) from the tokens and h, c (updated in
// place); dead rows get zero attention, carry their state and are ignored by the selection
static int beam_member_step(const sat_decoder_dims& d, const sat_decoder_params& p, const float* ann, const BeamWs& w, const int* tok, float* alpha, float* h,
                            float* c, const int* live, int K, const sat_beam_sampling* smp, int step, hipStream_t st) {
    const bool noisy = smp && smp->decoder_noise != 0.f;
    if (noisy) {        // model.py:322-324: randn * decoder_noise / (step + 1) joins h of every layer before the LSTM
        const long N = (long)d.B * K, tot = (long)d.layers * N * d.n;
        hipLaunchKernelGGL(beam_state_noise_kernel, dim3(cdiv(tot, 256)), dim3(256), 0, st, w.noise, live, N, d.n, d.layers, smp->decoder_noise / (float)(step + 1),
                           (unsigned long long)smp->seed, 0x1000ull + step, smp->normals ? smp->normals + (long)step * tot : (const float*)nullptr);
        SAT_TRY(launch_ok("beam_state_noise"));
    }
    return step_run(d, p, ann, w.s, tok, h, c, live, d.B, K, noisy ? w.noise : nullptr, alpha, w.logits, st);
}
// the kept hypotheses' parents' states: h, c (layers, N, n) gathered through gmap into h2, c2; the pairs swap
static int beam_member_gather(const sat_decoder_dims& d, const int* gmap, const int* klive, int Bv, int Kv, int N, float*& h, float*& c, float*& h2, float*& c2,
                              hipStream_t st) {
    const int n = d.n, NL = d.layers;
    const long tot = (long)NL * N * n;
    hipLaunchKernelGGL(beam_gather_state_kernel, dim3(cdiv(tot, 256)), dim3(256), 0, st, h, h2, gmap, klive, Bv, Kv, n, NL);
    SAT_TRY(launch_ok("beam_gather h"));
    hipLaunchKernelGGL(beam_gather_state_kernel, dim3(cdiv(tot, 256)), dim3(256), 0, st, c, c2, gmap, klive, Bv, Kv, n, NL);
    SAT_TRY(launch_ok("beam_gather c"));
    float* t1 = h; h = h2; h2 = t1; t1 = c; c = c2; c2 = t1;
    return SAT_OK;
}

// One model of a search: what the three helpers above need, and where its attention maps go.
struct BeamMember {
    const sat_decoder_dims* d; const sat_decoder_params* p; const float* ann;
    BeamWs w;                                  // h / h2 and c / c2 swap here as the states are gathered
    float* alpha; long alpha_step;             // step s writes alpha + s * alpha_step (0: one step's scratch)
};
// The combine stage of an ensemble: the members' logits at 1 / T -> `combined`, the logits the search then scores at temperature 1.
struct BeamCombine { EnsembleArgs args; int geometric; float* combined; };

// What a search runs, decided once from its descriptor by beam_plan: the workspace query returns `total`, the search lays its workspace
// out from the same fields and compares `total` with the bytes it was given.  smp: NULL = "beam" sampling without noise; con: NULL, or
// the constrained search's per-image selection (the history rules, the groups and the required words run in it as well); hist: NULL, or
// the rules with the history tables on (every rule off with them on: required words); req: NULL, or the required words, which select
// in beam_select_kernel's place; G groups (1 = off) with diversity penalty lambda.
struct BeamPlan {
    const sat_beam_sampling* smp; const sat_beam_constraints* con; const sat_beam_history* hist; const sat_beam_required* req;
    int G; float lambda; int topg, hist_stride; size_t total;
};
// the call a plan is made for: NULL for the workspace query, which has no outputs, no workspace and no stream to refuse
struct BeamCall { const sat_beam_search_out* o; size_t ws_bytes; hipStream_t st; };

// The search loop of decoder_beam_batched and decoder_beam_ensemble, after beam_plan: M members step on the shared tokens, the scores
// come from member 0's logits at 1 / T (comb == NULL: the single-model search) or from the combined logits; the score kernels, the
// selection, beam_update and the history advance run once, in member 0's workspace.
static int beam_search_loop(BeamMember* mem, int M, const BeamCombine* comb, const sat_beam_search_desc& s, const sat_beam_search_out& o, const BeamPlan& plan,
                            hipStream_t st) {
    const int K = s.beamk, G = plan.G, max_gen_length = s.max_gen_length, n_temps = s.n_temperatures, hist_stride = plan.hist_stride, topg = plan.topg;
    const float lambda = plan.lambda, *const temps_host = s.temperatures_host;
    const int* special_host = s.special_ids_host;
    int *const tok_in = o.tok_in, *const prev_row = o.prev_row, *const fin_count = o.fin_count, *const fin_step = o.fin_step, *const fin_row = o.fin_row;
    float *const fin_score = o.fin_score, *const fin_mean = o.fin_mean;
    const sat_beam_sampling* smp = plan.smp; const sat_beam_constraints* con = plan.con; const sat_beam_history* hist = plan.hist; const sat_beam_required* req = plan.req;
    const BeamWs& w = mem[0].w;
    const int B = mem[0].d->B, N = B * K, V = mem[0].d->V;
    const int START = special_host[0], END = special_host[2];
    const int method = smp ? smp->method : 0;
    const bool hist_on = hist != nullptr;
    const float theta = hist_on && hist->repetition_penalty != 0.f ? hist->repetition_penalty : 1.0f;
    const int max_prefix = con ? con->max_prefix : 0;
    const int* prefix_len = max_prefix > 0 ? con->prefix_len : nullptr;
    for (int i = 0; i < M; ++i) SAT_TRY(beam_member_begin(*mem[i].d, *mem[i].p, mem[i].ann, mem[i].w, K, G, special_host, st));
    auto zero_w = [&](void* dst, long n_) { beam_zero_words(st, dst, n_); };
    // the bookkeeping below the selection sees (image, group) pairs as Bv images of Kv rows; without groups these are B and K
    const int Bv = B * G, Kv = K / G;
    int* const f_count = G > 1 ? w.g_count : fin_count; int* const f_step = G > 1 ? w.g_step : fin_step; int* const f_row = G > 1 ? w.g_row : fin_row;
    float* const f_score = G > 1 ? w.g_score : fin_score; float* const f_mean = G > 1 ? w.g_mean : fin_mean;
    hipLaunchKernelGGL(fill_int_kernel, dim3(cdiv(Bv, 256)), dim3(256), 0, st, w.klive, (long)Bv, Kv);
    SAT_TRY(launch_ok("fill klive"));
    zero_w(tok_in, (long)(max_gen_length + 2) * N);       // rows that are not live still index the embedding table
    zero_w(prev_row, (long)(max_gen_length + 2) * N);
    hipLaunchKernelGGL(fill_int_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, tok_in, (long)N, START);
    SAT_TRY(launch_ok("fill start tokens"));
    for (int i = 0; i < M; ++i) {
        zero_w(mem[i].w.h2, (long)mem[i].d->layers * N * mem[i].d->n);
        zero_w(mem[i].w.c2, (long)mem[i].d->layers * N * mem[i].d->n);
    }
    zero_w(w.top, N);
    zero_w(f_count, Bv);
    if (hist_on) { zero_w(w.hist_a, (long)N * hist_stride); zero_w(w.hist_b, (long)N * hist_stride); }
    SAT_TRY(launch_ok("beam: clears"));

    int *hcur = w.hist_a, *hnext = w.hist_b;
    for (int step = 0; step <= max_gen_length; ++step) {
        const int* tok = tok_in + (long)step * N;
        hipLaunchKernelGGL(beam_live_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, w.klive, w.live, Bv, Kv);
        SAT_TRY(launch_ok("beam_live"));
        for (int i = 0; i < M; ++i)
            SAT_TRY(beam_member_step(*mem[i].d, *mem[i].p, mem[i].ann, mem[i].w, tok, mem[i].alpha + step * mem[i].alpha_step, mem[i].w.h, mem[i].w.c, w.live, K,
                                     smp, step, st));
        // ---- model.py:330-359: log-softmax, special-token masks, parent scores, top-k per image
        const float inv_T = 1.0f / temps_host[step % n_temps];
        if (comb) {
            hipLaunchKernelGGL(beam_ensemble_combine_kernel, dim3(N), dim3(256), 0, st, comb->args, M, comb->geometric, V, inv_T, comb->combined);
            SAT_TRY(launch_ok("beam_ensemble_combine"));
        }
        const float* z = comb ? comb->combined : w.logits;
        const float inv_temp = comb ? 1.0f : inv_T;
        const float* parent = step == 0 ? (const float*)nullptr : w.top;
        const bool drawn = method != 0 && method != SAT_SAMPLE_ANCESTRAL && step > 0;      // the first step always takes the top beamk words (model.py:343)
        if (con) {                                     // per image: forced word (step < P_b), row 0 (step == P_b), the free search after it
            if (hist_on) {
                hipLaunchKernelGGL(beam_history_scores_kernel, dim3(N), dim3(256), 0, st, z, K, V, inv_temp, w.mask_first, 4, w.mask_rest, 2, step, prefix_len,
                                   max_prefix, con->banned, con->n_banned, parent, hcur, (const int*)nullptr, hist_stride, hist->no_repeat_ngram,
                                   hist->min_length, theta, END, w.scores);
                SAT_TRY(launch_ok("beam_scores (history)"));
            } else {
                hipLaunchKernelGGL(beam_scores_constrained_kernel, dim3(N), dim3(256), 0, st, z, K, V, inv_temp, w.mask_first, w.mask_rest, step, prefix_len,
                                   max_prefix, con->banned, con->n_banned, parent, w.scores);
                SAT_TRY(launch_ok("beam_scores (constrained)"));
            }
            if (topg > 0 && step > 0) {
                hipLaunchKernelGGL(beam_row_topg_kernel, dim3(N), dim3(256), 0, st, w.scores, w.klive, K, V, topg, step, prefix_len, max_prefix, w.cand_val, w.cand_idx);
                SAT_TRY(launch_ok("beam_row_topg"));
            }
            if (drawn) SAT_TRY(launch_sample_keys(st, w.scores, w.klive, N, K, V, *smp, step, w.keys));
            if (G > 1) {
                hipLaunchKernelGGL(beam_group_select_kernel, dim3(B), dim3(1024), 0, st, w.scores, w.work, w.klive, K, G, V, step == 0 ? 1 : 0, lambda, w.vals, w.inds);
                SAT_TRY(launch_ok("beam_group_select"));
            } else if (req) {
                hipLaunchKernelGGL(beam_required_select_kernel, dim3(B), dim3(1024), 0, st, w.scores, w.work, w.klive, hcur, hist_stride, step, req->words,
                                   req->n_words, req->max_required, K, V, (step == 0 ? 1 : 0) | (step == max_gen_length ? 2 : 0), END, w.vals, w.inds);
                SAT_TRY(launch_ok("beam_required_select"));
            } else {
                hipLaunchKernelGGL(beam_select_kernel, dim3(B), dim3(1024), 0, st, w.scores, drawn ? w.keys : (const float*)nullptr, w.cand_val, w.cand_idx, topg,
                                   w.work, w.klive, K, V, step, max_prefix > 0 ? con->prefix : (const int*)nullptr, prefix_len, max_prefix, w.vals, w.inds);
                SAT_TRY(launch_ok("beam_select"));
            }
        } else {
            hipLaunchKernelGGL(beam_scores_kernel, dim3(N), dim3(256), 0, st, z, V, inv_temp, step == 0 ? w.mask_first : w.mask_rest, step == 0 ? 4 : 2, parent, w.scores);
            SAT_TRY(launch_ok("beam_scores"));
            if (method == SAT_SAMPLE_ANCESTRAL) {          // beamk == 1: every step, the first included, is one draw from the row's own distribution
                hipLaunchKernelGGL(beam_ancestral_keys_kernel, dim3(N), dim3(256), 0, st, w.scores, w.klive, K, V, (unsigned long long)smp->seed,
                                   (unsigned long long)step, smp->gumbel ? smp->gumbel + (long)step * N * V : (const float*)nullptr, w.keys);
                SAT_TRY(launch_ok("beam_ancestral_keys"));
            } else if (drawn) {                            // model.py:360-379: draw the continuing hypotheses (Gumbel-top-k == multinomial without replacement)
                SAT_TRY(launch_sample_keys(st, w.scores, w.klive, N, K, V, *smp, step, w.keys));
            }
            const bool keyed = drawn || method == SAT_SAMPLE_ANCESTRAL;
            hipLaunchKernelGGL(beam_topk_kernel, dim3(B), dim3(1024), 0, st, keyed ? w.keys : w.scores, w.work, w.klive, K, V, !keyed && step == 0 ? 1 : 0, w.vals,
                               w.inds);
            SAT_TRY(launch_ok(keyed ? "beam_topk (keys)" : "beam_topk"));
        }
        if (drawn || method == SAT_SAMPLE_ANCESTRAL) {     // the kept hypotheses carry their scores, not their keys
            hipLaunchKernelGGL(beam_take_scores_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, w.scores, w.inds, w.klive, B, K, V, w.vals);
            SAT_TRY(launch_ok("beam_take_scores"));
        }
        hipLaunchKernelGGL(beam_update_kernel, dim3(cdiv(Bv, 64)), dim3(64), 0, st, w.vals, w.inds, w.klive, Bv, Kv, V, step, max_gen_length, END, prefix_len, max_prefix,
                           tok_in + (long)(step + 1) * N, prev_row + (long)(step + 1) * N, w.top, w.gmap, f_count, f_step, f_row, f_score, f_mean);
        SAT_TRY(launch_ok("beam_update"));
        if (hist_on && step < max_gen_length) {
            hipLaunchKernelGGL(beam_history_advance_kernel, dim3(cdiv((long)N * (step + 1), 256)), dim3(256), 0, st, hcur, hnext, tok_in + (long)(step + 1) * N,
                               prev_row + (long)(step + 1) * N, w.klive, Bv, Kv, hist_stride, step);
            SAT_TRY(launch_ok("beam_history_advance"));
            int* t0 = hcur; hcur = hnext; hnext = t0;
        }
        if (step < max_gen_length)
            for (int i = 0; i < M; ++i)
                SAT_TRY(beam_member_gather(*mem[i].d, w.gmap, w.klive, Bv, Kv, N, mem[i].w.h, mem[i].w.c, mem[i].w.h2, mem[i].w.c2, st));
    }
    if (G > 1) {                                           // group-local parents and per-group finished lists -> the caller's image-level layout
        const long n_prev = (long)(max_gen_length + 1) * N;
        hipLaunchKernelGGL(beam_group_merge_kernel, dim3(cdiv(n_prev > Bv ? n_prev : (long)Bv, 256)), dim3(256), 0, st, prev_row + N, n_prev, B, K, G, w.g_count,
                           w.g_step, w.g_row, w.g_score, w.g_mean, fin_count, fin_step, fin_row, fin_score, fin_mean);
        SAT_TRY(launch_ok("beam_group_merge"));
    }
    if (req) {                                             // the finished lists keep the hypotheses that contain the most required words
        hipLaunchKernelGGL(beam_required_finish_kernel, dim3(B), dim3(256), 0, st, tok_in, prev_row, fin_count, fin_step, fin_row, fin_score, fin_mean,
                           req->words, req->n_words, req->max_required, B, K, max_gen_length, V, o.req_met);
        SAT_TRY(launch_ok("beam_required_finish"));
    }
    return SAT_OK;
}

// The plan of a single-model search: which of the features are on, every refusal they have (in this order), and the workspace they need.
static int beam_plan_single(const sat_beam_search_desc& s, const BeamCall* call, BeamPlan& plan) {
    const sat_decoder_dims& d = *s.d;
    const int K = s.beamk, max_gen_length = s.max_gen_length;
    const sat_beam_sampling* smp = s.sampling; const sat_beam_constraints* con = s.constraints; const sat_beam_history* hist = s.history;
    const sat_beam_groups* grp = s.groups; const sat_beam_required* req = s.required;
    // no constraint at all: exactly the launches of the plain / sampled search
    if (con && con->topg == 0 && con->max_prefix == 0 && con->n_banned == 0) con = nullptr;
    const int method = smp ? smp->method : 0;
    SAT_TRY(beam_groups_check(grp, "beam_groups"));
    const int G = grp && grp->groups > 1 ? grp->groups : 1;        // 1: today's search, the same launches
    const float lambda = G > 1 ? grp->diversity_penalty : 0.f;
    if (G > 1) {                                           // the groups select in the constrained search's place ("Diverse beam search")
        SAT_REQUIRE(K >= 1 && K % G == 0, "beam_groups: beamk %d is not a multiple of groups %d", K, G);
        SAT_REQUIRE(K <= SAT_BEAM_GROUP_MAX_K && K / G <= d.V, "beam_groups: beamk %d above %d, or beamk / groups above V=%d", K, SAT_BEAM_GROUP_MAX_K, d.V);
        SAT_REQUIRE(method == SAT_SAMPLE_BEAM, "beam_groups: groups combine with \"beam\" sampling only (method %d)", method);
        SAT_REQUIRE(!smp || smp->decoder_noise == 0.f, "beam_groups: groups do not combine with decoder_noise");
        SAT_REQUIRE(!con || con->topg == 0, "beam_groups: groups do not combine with topg %d", con ? con->topg : 0);
        SAT_REQUIRE(!con || con->max_prefix == 0, "beam_groups: groups do not combine with a forced prefix (max_prefix %d)", con ? con->max_prefix : 0);
        if (call) SAT_TRY(not_capturing(call->st, "beam_groups"));
    }
    SAT_TRY(beam_required_check(req, K, max_gen_length, "beam_required"));
    if (req && req->max_required == 0) req = nullptr;      // off: today's search, the same launches
    if (req) {                                             // the words select in the constrained search's place ("Required words")
        SAT_REQUIRE(!call || call->o->req_met, "beam_required: null pointer (req_met with max_required %d)", req->max_required);
        SAT_REQUIRE(method == SAT_SAMPLE_BEAM, "beam_required: required words combine with \"beam\" sampling only (method %d)", method);
        SAT_REQUIRE(!smp || smp->decoder_noise == 0.f, "beam_required: required words do not combine with decoder_noise");
        SAT_REQUIRE(!con || con->topg == 0, "beam_required: required words do not combine with topg %d", con ? con->topg : 0);
        SAT_REQUIRE(!con || con->max_prefix == 0, "beam_required: required words do not combine with a forced prefix (max_prefix %d)", con ? con->max_prefix : 0);
        SAT_REQUIRE(G == 1, "beam_required: required words do not combine with groups %d", G);
        if (call) SAT_TRY(not_capturing(call->st, "beam_required"));
    }
    SAT_TRY(beam_history_check(hist, max_gen_length, "beam_history"));
    static const sat_beam_history no_rules = {};
    if (req && !beam_history_on(hist)) hist = &no_rules;   // the history tables are on, every rule off: the constrained search's scores
    const bool hist_on = req || beam_history_on(hist);
    static const sat_beam_constraints no_constraint = {};
    if (hist_on) {                                         // the history rules run in the constrained search's per-image selection
        SAT_REQUIRE(max_gen_length + 1 <= SAT_BEAM_HIST_MAX, "beam_history: max_gen_length %d is over the limit (max_gen_length + 1 <= %d)", max_gen_length,
                    SAT_BEAM_HIST_MAX);
        SAT_REQUIRE(method != SAT_SAMPLE_ANCESTRAL, "beam_history: ancestral sampling does not combine with the history rules");
        if (call) SAT_TRY(not_capturing(call->st, "beam_history"));
        if (!con) con = &no_constraint;
    }
    if (G > 1 && !con) con = &no_constraint;
    const int hist_stride = hist_on ? max_gen_length + 1 : 0;
    if (con) {
        SAT_REQUIRE(K <= 1024, "beam_constrained: beamk %d above 1024 (one thread per row in the forced steps)", K);
        SAT_REQUIRE(con->topg >= 0 && con->topg <= d.V, "beam_constrained: topg %d outside 1..V=%d (0 = off)", con->topg, d.V);
        SAT_REQUIRE(con->topg == 0 || method == 0, "beam_constrained: topg %d combines with \"beam\" sampling only (method %d)", con->topg, method);
        SAT_REQUIRE(con->max_prefix >= 0 && con->max_prefix <= max_gen_length, "beam_constrained: max_prefix %d outside 0..max_gen_length=%d", con->max_prefix,
                    max_gen_length);
        SAT_REQUIRE(con->n_banned >= 0 && con->n_banned <= d.V, "beam_constrained: n_banned %d outside 0..V=%d", con->n_banned, d.V);
        SAT_REQUIRE((con->max_prefix == 0 || (con->prefix && con->prefix_len)) && (con->n_banned == 0 || con->banned),
                    "beam_constrained: null pointer (prefix / prefix_len with max_prefix %d, banned with n_banned %d)", con->max_prefix, con->n_banned);
    }
    SAT_REQUIRE(method >= 0 && method <= SAT_SAMPLE_ANCESTRAL && (method != 2 || (smp->sample_topk >= 1 && smp->sample_topk <= d.V)),
                "beam_batched: sampling method %d, sample_topk %d", method, smp ? smp->sample_topk : 0);
    if (method == SAT_SAMPLE_ANCESTRAL) {
        SAT_REQUIRE(K == 1, "beam_batched: ancestral sampling is defined for beamk == 1 (beamk %d): samples are rows of the batch", K);
        SAT_REQUIRE(!con, "beam_batched: ancestral sampling does not combine with constraints (topg / prefix / banned ids)");
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (call && hipStreamIsCapturing(call->st, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
        SAT_REQUIRE(cap == hipStreamCaptureStatusNone, "beam_batched: ancestral sampling is not replayed from a graph (the stream is being captured)");
    }
    SAT_REQUIRE(method != SAT_SAMPLE_NUCLEUS || (smp->sample_topp > 0.f && smp->sample_topp <= 1.f),
                "beam_batched: sample_topp %g outside (0, 1] (nucleus sampling)", smp ? (double)smp->sample_topp : 0.0);
    plan = {smp, con, hist_on ? hist : nullptr, req, G, lambda, con ? con->topg : 0, hist_stride, 0};
    plan.total = beam_layout(d, K, nullptr, plan.topg, hist_stride, G).total;
    const size_t ws_bytes = call ? call->ws_bytes : plan.total;
    SAT_REQUIRE(ws_bytes >= plan.total && K >= 1 && max_gen_length >= 0 && s.n_temperatures >= 1, "beam_batched: workspace %zu < %zu, K=%d, max_gen_length=%d", ws_bytes,
                plan.total, K, max_gen_length);
    return SAT_OK;
}
static int decoder_beam_batched(const sat_beam_search_desc& s, const sat_beam_search_out& o, const BeamPlan& plan, char* ws, hipStream_t st) {
    BeamMember mem = {s.d, s.w, s.ann, beam_layout(*s.d, s.beamk, ws, plan.topg, plan.hist_stride, plan.G), o.alpha_hist, (long)s.d->B * s.beamk * s.d->L};
    return beam_search_loop(&mem, 1, nullptr, s, o, plan, st);
}
// sat_beam_required: well-formed for a search of K rows and max_gen_length steps?  (max_required 0 is "off" and asks nothing)
int beam_required_check(const sat_beam_required* r, int K, int max_gen_length, const char* what) {
    if (!r) return SAT_OK;
    SAT_REQUIRE(r->max_required >= 0 && r->max_required <= SAT_BEAM_REQUIRED_MAX, "%s: max_required %d outside 0..%d", what, r->max_required,
                SAT_BEAM_REQUIRED_MAX);
    if (r->max_required == 0) return SAT_OK;
    SAT_REQUIRE(r->words && r->n_words, "%s: null pointer (words / n_words with max_required %d)", what, r->max_required);
    SAT_REQUIRE(K <= SAT_BEAM_REQUIRED_MAX_K, "%s: beamk %d above %d", what, K, SAT_BEAM_REQUIRED_MAX_K);
    SAT_REQUIRE(r->max_required <= max_gen_length, "%s: max_required %d above max_gen_length %d", what, r->max_required, max_gen_length);
    SAT_REQUIRE(max_gen_length + 1 <= SAT_BEAM_HIST_MAX, "%s: max_gen_length %d is over the limit (max_gen_length + 1 <= %d)", what, max_gen_length,
                SAT_BEAM_HIST_MAX);
    return SAT_OK;
}
int beam_required_select(const float* scores, const int* klive, int B, int K, int V, const int* hist, int hist_stride, int hist_len, int first_step,
                         const sat_beam_required& req, int end_id, float* work, float* values, int* indices, hipStream_t st) {
    SAT_REQUIRE(B >= 1 && K >= 1 && V >= 1, "beam_required_select: non-positive size (B=%d beamk=%d V=%d)", B, K, V);
    SAT_REQUIRE(K <= SAT_BEAM_REQUIRED_MAX_K, "beam_required_select: beamk %d above %d", K, SAT_BEAM_REQUIRED_MAX_K);
    SAT_REQUIRE(req.max_required >= 0 && req.max_required <= SAT_BEAM_REQUIRED_MAX, "beam_required_select: max_required %d outside 0..%d", req.max_required,
                SAT_BEAM_REQUIRED_MAX);
    SAT_REQUIRE(hist_stride >= 0 && hist_stride <= SAT_BEAM_HIST_MAX, "beam_required_select: hist_stride %d outside 0..%d", hist_stride, SAT_BEAM_HIST_MAX);
    SAT_REQUIRE((req.max_required == 0 || (req.words && req.n_words)) && (hist_stride == 0 || hist),
                "beam_required_select: null pointer (words / n_words with max_required %d, hist with hist_stride %d)", req.max_required, hist_stride);
    hipLaunchKernelGGL(beam_required_select_kernel, dim3(B), dim3(1024), 0, st, scores, work, klive, hist, hist_stride, hist_len, req.words, req.n_words,
                       req.max_required, K, V, first_step & 3, end_id, values, indices);
    return launch_ok("beam_required_select");
}
// sat_beam_groups: well-formed?  (groups 0 and 1 are both "off")
int beam_groups_check(const sat_beam_groups* g, const char* what) {
    if (!g) return SAT_OK;
    SAT_REQUIRE(g->groups >= 0, "%s: groups %d is negative (0 or 1 = off)", what, g->groups);
    const float t = g->diversity_penalty;
    SAT_REQUIRE(t >= 0.f && t < INFINITY, "%s: diversity_penalty %g is not a finite number >= 0", what, (double)t);
    return SAT_OK;
}
int beam_group_select(const float* scores, const int* klive, int B, int K, int G, int V, int first_step, float lambda, float* work, float* values, int* indices,
                      hipStream_t st) {
    SAT_REQUIRE(B >= 1 && K >= 1 && G >= 1 && V >= 1 && K % G == 0, "beam_group_select: bad sizes (B=%d beamk=%d groups=%d V=%d; beamk %% groups == 0)", B, K, G, V);
    SAT_REQUIRE(K <= SAT_BEAM_GROUP_MAX_K && K / G <= V, "beam_group_select: beamk %d above %d, or beamk / groups above V=%d", K, SAT_BEAM_GROUP_MAX_K, V);
    SAT_REQUIRE(lambda >= 0.f && lambda < INFINITY, "beam_group_select: diversity_penalty %g is not a finite number >= 0", (double)lambda);
    hipLaunchKernelGGL(beam_group_select_kernel, dim3(B), dim3(1024), 0, st, scores, work, klive, K, G, V, first_step ? 1 : 0, lambda, values, indices);
    return launch_ok("beam_group_select");
}

int beam_scores(const float* logits, int K, int V, float temperature, const int* masked, int n_masked, const float* parent, float* scores, hipStream_t st) {
    SAT_REQUIRE(K > 0 && V > 0 && temperature > 0.f, "beam_scores: bad arguments");
    hipLaunchKernelGGL(beam_scores_kernel, dim3(K), dim3(256), 0, st, logits, V, 1.0f / temperature, masked, n_masked, parent, scores);
    return launch_ok("beam_scores");
}
// ------------------------------------------------------------------ ensemble decoding ("Ensemble decoding")
// weights and combine of an ensemble: well-formed?  (include/sat_hip.h, sat_beam_ensemble)
int beam_ensemble_check_weights(const float* weight, int members, int combine, const char* what) {
    SAT_REQUIRE(members >= 1 && members <= SAT_ENSEMBLE_MAX, "%s: members %d outside 1..%d", what, members, SAT_ENSEMBLE_MAX);
    SAT_REQUIRE(combine == SAT_ENSEMBLE_ARITHMETIC || combine == SAT_ENSEMBLE_GEOMETRIC, "%s: combine %d is neither arithmetic (%d) nor geometric (%d)", what,
                combine, SAT_ENSEMBLE_ARITHMETIC, SAT_ENSEMBLE_GEOMETRIC);
    double sum = 0.0;
    for (int i = 0; i < members; ++i) {
        SAT_REQUIRE(weight[i] >= 0.f && weight[i] < INFINITY, "%s: weight[%d] = %g is negative or not finite", what, i, (double)weight[i]);
        sum += weight[i];
    }
    SAT_REQUIRE(fabs(sum - 1.0) <= 1e-5, "%s: the weight entries sum to %.9g, not to 1 (within 1e-5)", what, sum);
    return SAT_OK;
}
int beam_ensemble_check(const sat_beam_ensemble* e, const char* what) {
    SAT_REQUIRE(e, "%s: null ensemble struct", what);
    SAT_REQUIRE(e->members >= 1 && e->members <= SAT_ENSEMBLE_MAX, "%s: members %d outside 1..%d", what, e->members, SAT_ENSEMBLE_MAX);
    for (int i = 0; i < e->members; ++i)
        SAT_REQUIRE(e->dims[i] && e->params[i] && e->ann[i], "%s: null pointer for member %d (dims / params / ann)", what, i);
    for (int i = 1; i < e->members; ++i)
        SAT_REQUIRE(e->dims[i]->B == e->dims[0]->B && e->dims[i]->V == e->dims[0]->V, "%s: member %d has B=%d V=%d, member 0 has B=%d V=%d (one batch, one vocabulary)",
                    what, i, e->dims[i]->B, e->dims[i]->V, e->dims[0]->B, e->dims[0]->V);
    return beam_ensemble_check_weights(e->weight, e->members, e->combine, what);
}
int beam_ensemble_scores(const float* const* logits, const float* weight, int members, int combine, int rows, int V, float temperature, float* combined,
                         hipStream_t st) {
    SAT_TRY(beam_ensemble_check_weights(weight, members, combine, "beam_ensemble_scores"));
    SAT_REQUIRE(rows > 0 && V > 0 && temperature > 0.f, "beam_ensemble_scores: bad arguments (rows=%d V=%d temperature=%g)", rows, V, (double)temperature);
    for (int i = 0; i < members; ++i) SAT_REQUIRE(logits[i], "beam_ensemble_scores: null logits pointer for member %d", i);
    hipLaunchKernelGGL(beam_ensemble_combine_kernel, dim3(rows), dim3(256), 0, st, ensemble_args(logits, weight, members), members,
                       combine == SAT_ENSEMBLE_GEOMETRIC ? 1 : 0, V, 1.0f / temperature, combined);
    return launch_ok("beam_ensemble_combine");
}
// the members' search workspaces one after the other (member 0's with the history tables), then the combined logits (N, V) and, for
// every member but the first, one step's attention maps (N, L_i): alpha_hist is member 0's, the members' L differ
struct EnsembleWs { size_t total; size_t member[SAT_ENSEMBLE_MAX], alpha[SAT_ENSEMBLE_MAX], combined; };
static EnsembleWs ensemble_layout(const sat_beam_ensemble& e, int K, int hist_stride) {
    EnsembleWs w; size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t N = (size_t)e.dims[0]->B * K;
    for (int i = 0; i < e.members; ++i) w.member[i] = take(beam_layout(*e.dims[i], K, nullptr, 0, i == 0 ? hist_stride : 0).total);
    w.combined = take(N * e.dims[0]->V * 4);
    for (int i = 0; i < e.members; ++i) w.alpha[i] = i == 0 ? 0 : take(N * e.dims[i]->L * 4);
    w.total = off;
    return w;
}
size_t decoder_beam_ensemble_workspace_bytes(const sat_beam_ensemble& e, int K, int hist_stride) { return ensemble_layout(e, K, hist_stride).total; }

// The plan of an ensemble search ("beam" sampling; banned ids, min_length and no_repeat_ngram): what does not combine with an ensemble,
// then the refusals of the features that do, in the single-model search's words.
static int beam_plan_ensemble(const sat_beam_search_desc& s, const BeamCall* call, BeamPlan& plan) {
    const sat_beam_ensemble& e = *s.ensemble;
    const int K = s.beamk, max_gen_length = s.max_gen_length, V = e.dims[0]->V;
    const sat_beam_constraints* con = s.constraints; const sat_beam_history* hist = s.history;
    const int method = s.sampling ? s.sampling->method : 0, G = s.groups ? s.groups->groups : 0, C = s.required ? s.required->max_required : 0;
    SAT_REQUIRE(!s.d && !s.w && !s.ann, "beam_ensemble: d / w / ann are set together with ensemble (all three are NULL with an ensemble)");
    SAT_REQUIRE(method == SAT_SAMPLE_BEAM, "beam_ensemble: sampling method %d does not combine with an ensemble (\"beam\" only)", method);
    SAT_REQUIRE(!s.sampling || s.sampling->decoder_noise == 0.f, "beam_ensemble: sampling decoder_noise %g does not combine with an ensemble",
                s.sampling ? (double)s.sampling->decoder_noise : 0.0);
    SAT_REQUIRE(G <= 1, "beam_ensemble: groups %d do not combine with an ensemble (0 or 1 = off)", G);
    SAT_REQUIRE(C <= 0, "beam_ensemble: required words (max_required %d) do not combine with an ensemble", C);
    SAT_REQUIRE(!con || con->topg == 0, "beam_ensemble: topg %d does not combine with an ensemble", con ? con->topg : 0);
    SAT_REQUIRE(!con || con->max_prefix == 0, "beam_ensemble: a forced prefix (max_prefix %d) does not combine with an ensemble", con ? con->max_prefix : 0);
    SAT_REQUIRE(!hist || hist->repetition_penalty == 0.f || hist->repetition_penalty == 1.0f,
                "beam_ensemble: repetition_penalty %g does not combine with an ensemble (0 or 1 = off)", hist ? (double)hist->repetition_penalty : 0.0);
    if (call) SAT_TRY(not_capturing(call->st, "beam_ensemble"));
    if (con && con->n_banned == 0) con = nullptr;
    SAT_TRY(beam_history_check(hist, max_gen_length, "beam_history"));
    const bool hist_on = beam_history_on(hist);
    static const sat_beam_constraints no_constraint = {};
    if (hist_on) {
        SAT_REQUIRE(max_gen_length + 1 <= SAT_BEAM_HIST_MAX, "beam_history: max_gen_length %d is over the limit (max_gen_length + 1 <= %d)", max_gen_length,
                    SAT_BEAM_HIST_MAX);
        if (!con) con = &no_constraint;
    }
    if (con) {
        SAT_REQUIRE(K <= 1024, "beam_constrained: beamk %d above 1024 (one thread per row in the forced steps)", K);
        SAT_REQUIRE(con->n_banned >= 0 && con->n_banned <= V && (con->n_banned == 0 || con->banned), "beam_constrained: n_banned %d outside 0..V=%d, or null banned",
                    con->n_banned, V);
    }
    plan = {nullptr, con, hist_on ? hist : nullptr, nullptr, 1, 0.f, 0, hist_on ? max_gen_length + 1 : 0, 0};
    plan.total = ensemble_layout(e, K, plan.hist_stride).total;
    const size_t ws_bytes = call ? call->ws_bytes : plan.total;
    SAT_REQUIRE(ws_bytes >= plan.total && K >= 1 && max_gen_length >= 0 && s.n_temperatures >= 1, "beam_ensemble: workspace %zu < %zu, K=%d, max_gen_length=%d", ws_bytes,
                plan.total, K, max_gen_length);
    return SAT_OK;
}
// decoder_beam_batched over M models: every member runs its own once-per-batch block, step and state gather (the three helpers above)
// on the shared tokens; the members' logits are combined, and the score kernels, the selection, beam_update and the history advance
// run ONCE, on the combined logits at temperature 1, in member 0's workspace.
static int decoder_beam_ensemble(const sat_beam_search_desc& s, const sat_beam_search_out& o, const BeamPlan& plan, char* ws, hipStream_t st) {
    const sat_beam_ensemble& e = *s.ensemble;
    const int M = e.members, K = s.beamk;
    const sat_decoder_dims& d0 = *e.dims[0];
    const EnsembleWs lay = ensemble_layout(e, K, plan.hist_stride);
    const size_t N = (size_t)d0.B * K;
    BeamMember mem[SAT_ENSEMBLE_MAX];
    const float* zs[SAT_ENSEMBLE_MAX];
    for (int i = 0; i < M; ++i) {              // alpha_hist is member 0's; the other members' maps (their L differ) are one step's scratch
        mem[i] = {e.dims[i], e.params[i], e.ann[i], beam_layout(*e.dims[i], K, ws + lay.member[i], 0, i == 0 ? plan.hist_stride : 0),
                  i == 0 ? o.alpha_hist : reinterpret_cast<float*>(ws + lay.alpha[i]), i == 0 ? (long)N * d0.L : 0L};
        zs[i] = mem[i].w.logits;
    }
    const BeamCombine comb = {ensemble_args(zs, e.weight, M), e.combine == SAT_ENSEMBLE_GEOMETRIC ? 1 : 0, reinterpret_cast<float*>(ws + lay.combined)};
    return beam_search_loop(mem, M, &comb, s, o, plan, st);
}

// One plan for the workspace query and the search (include/sat_hip.h, sat_beam_search_desc): the query is the figure the search
// compares its workspace against, and refuses what the search refuses.
static int beam_plan(const sat_beam_search_desc& s, const BeamCall* call, BeamPlan& plan) {
    return s.ensemble ? beam_plan_ensemble(s, call, plan) : beam_plan_single(s, call, plan);
}
int beam_search_workspace_bytes(const sat_beam_search_desc& s, size_t& total) {
    BeamPlan plan;
    SAT_TRY(beam_plan(s, nullptr, plan));
    total = plan.total;
    return SAT_OK;
}
int beam_search(const sat_beam_search_desc& s, const sat_beam_search_out& o, char* ws, size_t ws_bytes, hipStream_t st) {
    BeamPlan plan;
    const BeamCall call = {&o, ws_bytes, st};
    SAT_TRY(beam_plan(s, &call, plan));
    return s.ensemble ? decoder_beam_ensemble(s, o, plan, ws, st) : decoder_beam_batched(s, o, plan, ws, st);
}

int beam_history_scores(const float* logits, int rows, int V, float temperature, const int* masked, int n_masked, const float* parent, const int* hist,
                        const int* hist_len, int hist_stride, const sat_beam_history& rules, int step, int end_id, float* scores, hipStream_t st) {
    SAT_TRY(not_capturing(st, "beam_history_scores"));
    const float theta = rules.repetition_penalty != 0.f ? rules.repetition_penalty : 1.0f;
    hipLaunchKernelGGL(beam_history_scores_kernel, dim3(rows), dim3(256), 0, st, logits, 1, V, 1.0f / temperature, masked, n_masked, masked, n_masked, step,
                       (const int*)nullptr, 0, (const int*)nullptr, 0, parent, hist, hist_len, hist_stride, rules.no_repeat_ngram, rules.min_length, theta, end_id,
                       scores);
    return launch_ok("beam_history_scores");
}
int nucleus_keys(const float* scores, int rows, int V, float topp, float step, unsigned long long seed, unsigned long long stream, const float* gumbel,
                 float* keys, int* nucleus_size, hipStream_t st) {
    hipLaunchKernelGGL(beam_nucleus_keys_kernel, dim3(rows), dim3(256), 0, st, scores, (const int*)nullptr, 1, V, topp, step, seed, stream, gumbel, keys,
                       nucleus_size);
    return launch_ok("beam_nucleus_keys");
}
int topk(const float* x, float* work, long n, int k, float* values, int* indices, hipStream_t st) {
    SAT_REQUIRE(n > 0 && k > 0 && k <= n, "topk: bad arguments (n=%ld k=%d)", n, k);
    hipLaunchKernelGGL(topk_kernel, dim3(1), dim3(1024), 0, st, x, work, n, k, values, indices);
    return launch_ok("topk");
}

}  // namespace sat
