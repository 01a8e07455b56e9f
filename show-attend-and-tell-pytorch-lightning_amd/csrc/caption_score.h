// Internal C++ entry points of the on-device caption scoring (caption_score.hip; wrapped by the C ABI in api.hip).
#pragma once
#include "common.h"

namespace sat {
constexpr int kCaptionMaxLen = 128;      // SAT_CAPTION_MAX_LEN
constexpr int kCaptionMaxRefs = 16;      // SAT_CAPTION_MAX_REFS
constexpr int kCaptionMaxEmbed = 2048;   // SAT_CAPTION_MAX_EMBED
constexpr int kChrfMaxOrder = 6;         // SAT_CHRF_MAX_ORDER
constexpr int kChrfMaxChars = 2048;      // SAT_CHRF_MAX_CHARS
int beam_select(const int* tok_in, const int* prev_row, const int* fin_count, const int* fin_step, const int* fin_row, const float* fin_score,
                const float* fin_mean, const float* alpha_hist, int B, int K, int S, int L, int method, float reward, int pad_id, int* cap_tokens,
                int* cap_len, float* cap_score, float* cap_raw, int* cap_step, float* cap_alpha, hipStream_t st);
int beam_select_at(const int* tok_in, const int* prev_row, const int* fin_count, const int* fin_step, const int* fin_row, const float* fin_score,
                   const float* alpha_hist, const int* pick, const double* pick_score, int B, int K, int S, int L, int pad_id, int* cap_tokens, int* cap_len,
                   float* cap_score, float* cap_raw, int* cap_step, float* cap_alpha, hipStream_t st);
int beam_hypotheses(const int* tok_in, const int* prev_row, const int* fin_count, const int* fin_step, const int* fin_row, int B, int K, int S, int pad_id,
                    int* hyp_tokens, int* hyp_len, hipStream_t st);
int caption_stats(const int* cap_tokens,const int* cap_len, int W, const int* refs, const int* ref_len, int B, int R, int T, int* stats, hipStream_t st);
int caption_cosine(const int* cap_tokens, const int* cap_len, int W, const int* refs, const int* ref_len, int B, int R, int T, const float* embedding,
                   int V, int m, float* best, hipStream_t st);
// caption_consensus.hip: the n-gram document-frequency table and CIDEr-D / ROUGE-L against it
size_t ngram_table_bytes(long capacity);
int ngram_table_clear(void* table, long capacity, hipStream_t st);
int ngram_table_add(const int* refs, const int* ref_len, int B, int R, int T, void* table, long capacity, int* error_flag, hipStream_t st);
int caption_consensus(const int* cap_tokens, const int* cap_len, int W, const int* refs, const int* ref_len, int B, int R, int T, const void* table,
                      long capacity, long n_images, double sigma, double* scores, hipStream_t st);
// caption_mbr.hip: consensus (minimum-Bayes-risk) utilities of an image's hypotheses against each other
constexpr int kMbrMaxHyps = 32;          // SAT_MBR_MAX_HYPS
int caption_mbr(const int* hyp_tokens, const int* hyp_len, const int* hyp_count, const float* hyp_logp, int B, int K, int W, const void* table, long capacity,
                long n_images, double sigma, double w_cider, double w_rouge, double alpha, double* utilities, int* winner, hipStream_t st);
// caption_diversity.hip: the integers of distinct-n / mBLEU / unique captions over an image's hypotheses; the vocabulary captions use
constexpr int kDiversityStats = 20;      // SAT_DIVERSITY_STATS
int caption_diversity(const int* hyp_tokens, const int* hyp_len, const int* hyp_count, int B, int K, int W, int* stats, int* per_hyp, hipStream_t st);
int caption_vocab_usage(const int* cap_tokens, const int* cap_len, int W, int B, int V, int* counts, hipStream_t st);
// caption_chrf.hip: chrF over the characters of the vocabulary's spelling
int caption_chrf(const int* cap_tokens, const int* cap_len, int W, const int* refs, const int* ref_len, int B, int R, int T, const int* word_offsets,
                 const int* word_chars, int V, int max_word_chars, double beta, double* scores, int* stats, hipStream_t st);
}  // namespace sat
