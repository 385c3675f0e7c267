// Host-side launchers of the families that have no header of their own, declared once: the file that defines a launcher and
// every file that calls it include this header, so a definition whose parameters drift from its callers no longer links as an
// overload of its own.  The other families declare theirs beside their geometry: gemv_v3.h,
// gemv_v3_dispatch.h, decode_rows.h, decode_kv8.h, prefill_attn.h, attn_train.h, train_glue.h, gemm_w4.h, and the round-1 decode
// GEMV with its plan: gemv_w4.h.  Host only.
#pragma once
#include "qeft_common.h"      // hipError_t, hipStream_t

namespace qeft {

// ---- decode_aux.hip
hipError_t token_begin_launch(const void* embed, const void* tok, const void* rope_tab, const int* pos, void* h,
                              void* rope_row, int hidden, int vocab, int max_seq, hipStream_t st);
int token_begin_norm_blocks(int hidden);
hipError_t token_begin_norm_launch(const void* embed, const void* tok, const void* rope_tab, const int* pos, void* h,
                                   void* rope_row, const void* gamma, void* hnorm, float* ssq_out, int hidden, int vocab,
                                   int max_seq, hipStream_t st);
hipError_t token_end_launch(const void* logits, void* tok, int* pos, int vocab, int greedy, hipStream_t st);
hipError_t residual_norm_launch(const void* h, const void* add, const void* gamma, void* h_out, void* hnorm, float* ssq_out,
                                int hidden, hipStream_t st);
hipError_t rmsnorm_launch(const void* x, const void* add, const void* gamma, void* res_out, void* y, int m, int H,
                          float eps, hipStream_t st);
hipError_t rmsnorm_f32_launch(const void* x, const void* gamma, void* y, int m, int H, float eps, hipStream_t st);
hipError_t rope_rows_launch(void* x, const void* cs, const void* sn, int T, int H, int row_stride, hipStream_t st);
hipError_t silu_mul_launch(const void* gate, const void* up, void* out, int n, hipStream_t st);
hipError_t lm_head_f16_launch(const void* h32, const void* gamma, const void* W, void* logits, int H, int vocab, float eps,
                              hipStream_t st);
size_t attn_workspace_bytes(int n_heads, int S);
hipError_t rope_attn_decode_launch(const void* q, const void* k, const void* v, const void* cs, const void* sn, void* kc,
                                   void* vc, const int* pos, const int* out_pos, void* out, void* ws, int n_heads,
                                   int n_kv, int max_seq, int S, int tab_rows, hipStream_t st, bool k_ft_layout = false,
                                   const float* alibi_slopes = nullptr);
hipError_t sqa_generic_launch(const void* q, const void* k, const void* v, void* kc, void* vc, const int* pos, const float* alibi,
                              void* out, int n_heads, int n_kv, int max_seq, int head_dim, hipStream_t st);
extern unsigned long long* g_attn_dbg;

// ---- decode_sample.hip
hipError_t sample_launch(const void* logits, int vocab, int m, const int* params, const int* positions, void* tokens,
                         hipStream_t st);
hipError_t token_end_sample_launch(const void* logits, void* tok, int* pos, const int* params, int vocab, hipStream_t st);
hipError_t verify_sample_launch(const void* logits, const void* tokens, int m, int vocab, const int* params, int* work, void* out_tokens,
                                int* n_acc, void* tok, int* pos, hipStream_t st);
hipError_t token_end_sample_b_launch(const void* logits, const int* slot_tab, void* tok, int* pos_tab, const int* limit, const int* eos,
                                     int* done, void* out, int* ctr, const int* params, int vocab, int out_cap, int n_slots, int m,
                                     hipStream_t st);

// ---- aux_w4.hip
hipError_t dequant_w4_launch(const void* qw, const void* scales, const void* zeros, const void* ow, void* out, int N,
                             int K, int G, int n_out, hipStream_t st);
hipError_t pack_oweight_launch(const void* ow, void* il, int N, int R, hipStream_t st);
hipError_t pack_scales_launch(const void* scales, const void* zeros, void* out, int N, int ngroups, hipStream_t st);

// ---- gemm_ws.hip
bool gemm_ws_supported(int m, int n, int k, int group_size, int n_out);
hipError_t gemm_ws_launch(const void* x, const void* qweight, const void* scales, const void* zeros, const void* oweight, const void* bias,
                          void* y, int m, int n, int k, int n_out, hipStream_t st);

// ---- lm_head_nll.hip, lm_head_nll_grad.hip
size_t lm_head_nll_workspace_bytes(int t, int vocab);
hipError_t lm_head_nll_launch(const void* x, const void* w, const int* targets, float* lse, float* tgt_logit, int* argmax, void* ws,
                              int x_stride, int t, int hidden, int vocab, hipStream_t st);
long long lm_head_nll_count_out_of_range(int x_stride, int t, int hidden, int vocab);
int lm_head_nll_grad_chunk_rows();
size_t lm_head_nll_grad_workspace_bytes(int t, int vocab);
hipError_t lm_head_nll_grad_launch(const void* x, const void* w, const int* targets, const float* lse, const float* grad_nll, void* dx,
                                   void* ws, int x_stride, int dx_stride, int dx_fp32, int t, int hidden, int vocab, hipStream_t st);
long long lm_head_nll_grad_count_out_of_range(int x_stride, int dx_stride, int t, int hidden, int vocab);

}  // namespace qeft
