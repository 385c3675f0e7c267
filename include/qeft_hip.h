/*
 * qeft_hip.h — C ABI of the MI355X (gfx950) packed-weight quantized linear.
 *
 * Drop-in boundary for the one hot path of xvyaward/qeft: the functions the
 * reference binds in its `qeft_cuda` torch extension (qeft/kernel/qeft_cuda.cpp:10-27)
 * for the W4 group-quantised linear with retained fp16 outlier columns.
 * Plain pointers and sizes only; every pointer is a DEVICE pointer unless
 * noted; `stream` is a hipStream_t passed as void*.  No allocation, no
 * synchronisation and no host<->device copy happens inside any entry point,
 * so every call may be captured into a hipGraph.
 *
 * Buffers (reference checkpoint layout, qeft/qlinear.py:143-173):
 *   qweight       int16 [N/4, K]      4 rows interleaved per 64-k tile, nibble order of
 *                                     pack_intweight (qlinear.py:81-121)
 *   scales        fp16  [K/g, N]
 *   scaled_zeros  fp16  [K/g, N]      = -(zero * scale)
 *   oweight       fp16  [N, r]        retained outlier columns (the LAST r input columns)
 *   oweight_il    fp16  [N/2, 2r]     pack_oweight interleave (qlinear.py:70-79)
 *   x             fp16  [m, K] row-major contiguous;  y fp16 [m, N]
 *
 * Every function returns QEFT_OK (0) or a QEFT_ERR_* code; qeft_error_string()
 * gives the message.  Kernel-launch failures return QEFT_ERR_LAUNCH and the
 * hipError_t is available from qeft_last_hip_error().
 * Which kernel a call ran: qeft_last_variant(), and for the v3 decode GEMV the instance itself, qeft_gemv_v3_last_plan().
 */
#ifndef QEFT_HIP_H
#define QEFT_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define QEFT_OK 0
#define QEFT_ERR_BATCH 1  /* m outside 1..7 on a gemv entry: "Unsupported batch size for gemv kernel."
                             (gemv_cuda_qeft.cu:466, gemv_cuda.cu:466) */
#define QEFT_ERR_SHAPE 2  /* N % 4, K % 64, n_out % 32 ... */
#define QEFT_ERR_GROUP 3  /* group size not a multiple of 32 dividing K */
#define QEFT_ERR_NULL 4   /* required pointer is NULL */
#define QEFT_ERR_LAUNCH 5 /* hip launch error, see qeft_last_hip_error() */
#define QEFT_ERR_ALIGN 6  /* pointer not 16-byte aligned */

typedef void* qeft_stream_t;

int qeft_abi_version(void);
const char* qeft_error_string(int code);
int qeft_last_hip_error(void);
/* Name of the kernel variant the calling thread's most recent compute entry point launched, e.g. "gemv_mfma",
 * "gemm_v2_128x256", "gemm_v2_128x128+splitk", "gemv_smallm", "dx128", "dx64+split", "grad_oweight_mfma",
 * "grad_oweight_mfma_n64".  Static storage;
 * diagnostic only (the parity tests assert it so that every routing tier keeps its coverage). */
const char* qeft_last_variant(void);

/* Kernel reached by the three gemv entries below (qeft_last_variant() names it):
 *   "gemv_v3" (m = 1) / "gemv_v3_mb" (m = 2..7): the round-2 MFMA GEMV of csrc/gemv_v3.h, taken when n % 16 == 0, k % 128 == 0,
 *       group_size in {128, k}, n_out in {0, 128}, no fp16 `residual`, operands 16-byte aligned.  It consumes the operands as the
 *       checkpoint holds them: scales / scaled_zeros [k/g][n] (or the sz_packed shadow when given), oweight_interleaved,
 *       reorder_ids gathered inside the launch.  Batches whose x rows exceed the block's LDS run as several launches.
 *   "gemv_mfma" / "gemv_valu": the round-1 kernels, for every other accepted shape (group sizes 32 / 64 / 256, n_out 32 / 64 /
 *       96, n % 16 != 0, k % 128 != 0, a residual).  QEFT_GEMV_V3=0 in the environment forces them everywhere.
 *
 * Decode GEMV, m in 1..7, no outlier slice.
 * Replaces gemv_4bit(in_feats, kernel, scaling_factors, zeros, m, n, k, group_size)
 * (qeft/kernel/quantization_new/gemv/gemv_cuda.cu:358-525). */
int qeft_gemv_w4(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                 void* y, int m, int n, int k, int group_size, qeft_stream_t stream);

/* Decode GEMV with the fp16 outlier slice taken from the interleaved buffer.
 * Replaces gemv_4bit_qeft(in_feats, kernel, scaling_factors, zeros, oweight_interleaved, m, n, k, group_size)
 * (qeft/kernel/quantization_new/gemv/gemv_cuda_qeft.cu:392-513); n_out = oweight_il.size(1)/2 (:424). */
int qeft_gemv_w4_qeft(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                      const void* oweight_il, void* y, int m, int n, int k, int group_size, int n_out,
                      qeft_stream_t stream);

/* Fused decode GEMV: everything QuantLinear.forward_* does around the kernel in one launch
 * (qeft/qlinear.py:244-330): optional input gather x[:, reorder_ids] (:275, int32 ids, NULL = none),
 * optional bias add (:268, NULL = none), optional residual add into y (y = acc + residual; NULL = none).
 * oweight_il may be NULL when n_out == 0; sz_packed (see qeft_pack_scales) may be NULL. */
int qeft_gemv_w4_fused(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                       const void* oweight_il, const void* bias, const int* reorder_ids,
                       const void* residual, const void* sz_packed, void* y, int m, int n, int k, int group_size,
                       int n_out, qeft_stream_t stream);

/* Optional derived buffer for the decode GEMV (never part of the checkpoint): sz_packed int32 [N/16][K/g][16] with
 * scale | scaled_zero << 16 per (row, group), so the scales of a 16-row block are one contiguous run.  Built once at
 * load time (QuantLinear.set_kernel); entries that take `sz_packed` accept NULL and then read scales / scaled_zeros
 * in their checkpoint layout.  group_size must be 128 or k; n % 16 == 0. */
int qeft_pack_scales(const void* scales, const void* scaled_zeros, void* sz_packed, int n, int k, int group_size,
                     qeft_stream_t stream);

/* Prefill / fine-tune GEMM  y[M,N] = x[M,K] . Wdeq[N,K]^T  on MFMA, fp32 accumulate, fp16 out.
 * Replaces gemm_4bit(in_feats, kernel, scales, zeros) (qeft/kernel/quantization_new/gemm/gemm_cuda.cu:929-1033).
 * With oweight == NULL the INT4 nibbles are used for every column (exactly gemm_4bit);
 * with oweight != NULL the last n_out columns come from the fp16 slice inside the same launch — the fusion
 * gemm_cuda_qeft.cu:1003 intended and qlinear.py:266 does with a second F.linear.  bias may be NULL. */
int qeft_gemm_w4(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                 const void* oweight, const void* bias, void* y, int m, int n, int k, int group_size,
                 int n_out, qeft_stream_t stream);

/* qeft_gemm_w4 with the MLP's activation in its epilogue:  y = silu(gate) * (x . Wdeq^T + bias), gate fp16 [m, n] -- the
 * reference's up_proj GEMM followed by act_fn(gate) * up (modeling_llama's LlamaMLP around qlinear.py:244-271) in one
 * launch on the 256-row tier (variant "gemm_v3_256x128+silu"), the GEMM plus qeft_silu_mul in place on the others; the
 * same rounding either way (the product is rounded to fp16 before the activation).  n % 8 == 0; y may not alias gate. */
int qeft_gemm_w4_silu_mul(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                          const void* oweight, const void* bias, const void* gate, void* y, int m, int n, int k,
                          int group_size, int n_out, qeft_stream_t stream);

/* gate_proj and up_proj of the MLP as ONE launch: qweight / scales / scaled_zeros / oweight / bias hold the two linears'
 * rows interleaved in blocks of 64 (rows 128 b .. 128 b + 63 = gate rows 64 b .., rows 128 b + 64 .. = up rows 64 b ..: a
 * permutation of whole checkpoint rows, built at load time by qeft_amd/fuse.py, never saved), n2 = both linears' rows;
 * y [m, n2 / 2] = silu(x . Wgate^T + bgate) * (x . Wup^T + bup), the two products rounded to fp16 first (bit-equal to the
 * separate launches).  qeft_gemm_w4_gateup_supported() says whether a shape is taken (n2 % 128 == 0, K >= 384,
 * group a power of two >= 64, n_out % 64 == 0); otherwise use the two linears and qeft_gemm_w4_silu_mul. */
int qeft_gemm_w4_gateup_supported(int m, int n2, int k, int group_size, int n_out);
int qeft_gemm_w4_gateup(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                        const void* oweight, const void* bias, void* y, int m, int n2, int k, int group_size, int n_out,
                        qeft_stream_t stream);

/* The same with a scratch buffer for mid-size m: when the 128x128 tiling of [m, n] leaves most of the chip idle the
 * K loop is cut into S parts (fp32 partial tiles in `workspace`, summed in a fixed order by a second small launch --
 * deterministic).  qeft_gemm_w4_workspace_bytes() is the size that enables it for a shape (0: no split would be
 * used); a smaller or NULL workspace silently means fewer parts / none.  16-byte aligned device memory, contents
 * irrelevant, must not be shared by launches that may overlap. */
long long qeft_gemm_w4_workspace_bytes(int m, int n, int k, int n_out);
int qeft_gemm_w4_ws(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                    const void* oweight, const void* bias, void* y, void* workspace, long long workspace_bytes, int m,
                    int n, int k, int group_size, int n_out, qeft_stream_t stream);

/* Backward wrt the input: dx[M,K] = dy[M,N] . Wdeq[N,K]; columns K-n_out.. use oweight (SURVEY.md §8a row 7;
 * the mathematically correct form of QuantMatMulQEFT.backward, qlinear.py:30-44). */
int qeft_gemm_w4_dx(const void* dy, const void* qweight, const void* scales, const void* scaled_zeros,
                    const void* oweight, void* dx, int m, int n, int k, int group_size, int n_out,
                    qeft_stream_t stream);
/* The same with a scratch buffer (as qeft_gemm_w4_ws): few output tiles and a long contraction over n -> the n loop is
 * cut into parts, fp32 partials in `workspace`, summed in a fixed order. */
long long qeft_gemm_w4_dx_workspace_bytes(int m, int n, int k);
int qeft_gemm_w4_dx_ws(const void* dy, const void* qweight, const void* scales, const void* scaled_zeros,
                       const void* oweight, void* dx, void* workspace, long long workspace_bytes, int m, int n, int k,
                       int group_size, int n_out, qeft_stream_t stream);

/* Gradient of the trainable outlier slice: d_oweight[N, r] (fp32) = dy[M,N]^T . x[M, K-r:]  (qlinear.py:41-42). */
int qeft_grad_oweight(const void* dy, const void* x, void* d_oweight_f32, int m, int n, int k, int n_out,
                      qeft_stream_t stream);

/* What the launchers behind qeft_gemm_w4* / qeft_gemm_w3 (forward), qeft_gemm_w4_dx* / qeft_gemm_w3_dx and qeft_grad_oweight
 * would do for a shape: host arithmetic only, no GPU needed.  The forward entries route few rows (m <= 64) to the GEMV and
 * weight-stationary tiers before their launcher is asked; these plans are the launcher's alone.
 * out[QEFT_GEMM_PLAN_INTS] = { tier id, grid x, y, z, threads per block, dynamic LDS bytes, split factor S, 1 if the reduce
 * launch follows, 1 if silu(gate) * y is fused into the epilogue, 1 if the shape is supported }; qeft_gemm_tier_name(tier id) is
 * the name qeft_last_variant reports for the tier ("" for an id that is none).  n_out: the outlier width in effect (0 without
 * oweight); bits 4 or 3; gate 0 none, 1 a gate tensor (qeft_gemm_w4_silu_mul), 2 the paired halves (qeft_gemm_w4_gateup);
 * workspace_bytes 0: none.  overrides: NULL for the process's environment, else 8 ints in place of it -- QEFT_GEMM_V3, _V3M, _V3S
 * (-1 unset), QEFT_GEMM_NWV, QEFT_DX_V3 (-1 unset), QEFT_DOW_BN, QEFT_GEMM_ABL (0 unset), and whether QEFT_GEMM_V1 is set.
 * Return QEFT_OK, QEFT_ERR_NULL without `out`, QEFT_ERR_SHAPE for m, n < 1, k < 64, group_size < 1, n_out < 0 or another gate. */
#define QEFT_GEMM_PLAN_INTS 10
int qeft_gemm_w4_plan(int m, int n, int k, int group_size, int n_out, int bits, int gate, long long workspace_bytes,
                      const int* overrides, int* out);
int qeft_gemm_w4_dx_plan(int m, int n, int k, int group_size, int n_out, int bits, long long workspace_bytes,
                         const int* overrides, int* out);
int qeft_grad_oweight_plan(int n, int k, int n_out, const int* overrides, int* out);
const char* qeft_gemm_tier_name(int tier);

/* What the round-1 decode GEMV launchers behind qeft_gemv_w4 / _qeft / _fused / qeft_gemv_w3 (kind 0, rows), the few-row route of
 * qeft_gemm_w4 (kind 1, small-M), qeft_gemv_w4_group / qeft_gemv_w3_group (kind 2) and qeft_gemv_w4_silu / qeft_gemv_w3_silu
 * (kind 3) would do for a shape: host arithmetic only, no GPU needed.  The entries hand a shape the v3 kernel takes to it before
 * these launchers are asked; the plan is the launcher's alone.  n_parts[nparts]: the layer's n (nparts 1) or the group's parts
 * (1..3); m: batch rows (kinds 0 and 1; >= 0); bits 4 or 3; flags: 1 x is gathered through reorder_ids (kind 0), 2 the group's
 * RMSNorm gamma is given (kind 2).  overrides: NULL for the process's environment, else 2 ints in place of it --
 * QEFT_GEMV_BLOCKS (0 unset) and the ring depth QEFT_GEMV_DEPTH stands for (0 unset, 4 or 6).
 * out[QEFT_GEMV_W4_PLAN_INTS] = { hipError_t of a refusal (0: planned; 801 not supported, 1 invalid value: the rest is 0),
 *   variant id (qeft_gemv_w4_variant_name: what qeft_last_variant reports, "" for 0: nothing launched), 1 MFMA / 0 VALU family,
 *   the template selectors BITS, D, RGI (0: MFMA), OUTL, XG, XT, threads per block, blk_end[0..2] of the last launch,
 *   then the body launch { count, batch rows, M (1..7 fixed, 16 run-time), blocks, dynamic LDS bytes, rs_cap (0: VALU) } and
 *   the tail launch likewise (count 0 or 1) }: the m rows go as `count` body launches and then the tail, on consecutive rows.
 * Return QEFT_OK, QEFT_ERR_NULL without n_parts or out, QEFT_ERR_SHAPE for another kind, bits or nparts (kinds other than 2: 1),
 * m < 0, a part that is not a positive multiple of 4, k % 64 != 0, group_size < 1 or not dividing k, n_out < 0 or >= k at 4 bits, an overrides depth other than 0, 4 or 6. */
#define QEFT_GEMV_W4_PLAN_INTS 25
int qeft_gemv_w4_plan(int kind, int bits, int m, int nparts, const int* n_parts, int k, int group_size, int n_out, int flags,
                      const int* overrides, int* out);
const char* qeft_gemv_w4_variant_name(int variant);

/* Dense dequantisation Wdeq[N,K] fp16 (validation / backward helper; the role of the uncompiled
 * dequantize_weight_4bit_qeft, qeft/kernel/quantization_new/dequantize/dequantize_cuda_qeft.cu:38-118).
 * oweight (plain [N, r]) may be NULL. */
int qeft_dequant_w4(const void* qweight, const void* scales, const void* scaled_zeros, const void* oweight,
                    void* w_out, int n, int k, int group_size, int n_out, qeft_stream_t stream);

/* Re-derive the interleaved outlier buffer from oweight on device (pack_oweight, qlinear.py:70-79);
 * used after fine-tuning so the GEMV never reads a stale copy (modelutils.py:192 quirk). */
int qeft_pack_oweight(const void* oweight, void* oweight_il, int n, int n_out, qeft_stream_t stream);

/* ---- decode-step helpers (SURVEY.md section 8f "next" rows 1, 3, 4; not part of the packed-weight path) ---- */

/* Up to 3 quantized linears that read the SAME x (q/k/v or gate/up) in one launch, batch 1.
 * Host arrays of `nparts` device pointers; oweight_il / bias entries may be NULL (all-or-none for oweight_il).
 * Equivalent to nparts calls of gemv_4bit_qeft (gemv_cuda_qeft.cu:392-513) on identical in_feats.
 * norm_gamma != NULL: the input is RMS-normalised while it is staged (x * rsqrt(mean x^2 + norm_eps) * gamma, the
 * arithmetic of qeft_rmsnorm / layernorm.cu:26-76), i.e. the decoder's input_layernorm / post_attention_layernorm
 * fused into the projection that consumes it (K <= 16384). */
int qeft_gemv_w4_group(const void* x, const void* norm_gamma, float norm_eps, int nparts,
                       const void* const* qweight, const void* const* scales, const void* const* scaled_zeros,
                       const void* const* oweight_il, const void* const* bias, const void* const* sz_packed,
                       void* const* y, const int* n, int k, int group_size, int n_out, qeft_stream_t stream);

/* down_proj of the decode step in one launch: y = W . (silu(gate) * up) (+ bias) (+ residual), batch 1.
 * The activation is formed while x is staged, rounded to fp16 exactly like qeft_silu_mul (K <= 16384). */
int qeft_gemv_w4_silu(const void* gate, const void* up, const void* qweight, const void* scales,
                      const void* scaled_zeros, const void* oweight_il, const void* bias, const void* residual,
                      const void* sz_packed, void* y, int n, int k, int group_size, int n_out, qeft_stream_t stream);

/* y = rmsnorm(x (+ add)) * gamma, fp32 statistics (role of layernorm_forward_cuda, qeft/kernel/layernorm/layernorm.cu:26-76).
 * If add != NULL the sum x + add is normalised and, if res_out != NULL, also written there (fused residual). */
int qeft_rmsnorm(const void* x, const void* add, const void* gamma, void* res_out, void* y, int m, int hidden,
                 float eps, qeft_stream_t stream);

/* out = silu(gate) * up, n elements (n % 8 == 0). */
int qeft_silu_mul(const void* gate, const void* up, void* out, int n, qeft_stream_t stream);

/* One decode token of one sequence: rotary on q/k at position *pos (device int), append k/v to the caches
 * [n_kv][max_seq][128] and compute softmax(q.K^T/sqrt(128)).V (role of single_query_attention,
 * qeft/kernel/attention/ft_attention.cpp:110-181, neox rotary).  head_dim is 128, max_seq % 16 == 0 and
 * 16 <= max_seq <= 32768 (QEFT_ERR_SHAPE otherwise): the kernel keeps one raw fp32 score per cache row in LDS,
 * (max_seq + 16) * 4 + 9232 bytes, 140 368 at 32768 of the 160 KiB a gfx950 CU has (above 64 KiB, max_seq >= 14064, the
 * launch raises the kernel's dynamic-LDS limit first).  qeft_single_query_attention[_alibi], qeft_rope_attn_decode_m and
 * qeft_rope_attn_decode_batch share the ceiling, so that a cache one of them serves can be served by all.
 * cos/sin: fp32 [tab_rows][64], tab_rows >= max_seq (row *pos is used), or tab_rows == 1: the caller has already
 * selected the row of this position (the kernel then has no load that waits for *pos before the rotary).
 * out_pos (optional int32 [n_heads*128]): element i of the attention output is stored at out[out_pos[i]].  With
 * out_pos = inverse of o_proj's reorder_ids the o_proj input gather (qlinear.py:275) costs nothing.
 * n_split in {1, 2, 4, 8}: blocks per head (the context is dealt over them; the last block to finish merges the
 * head, in a fixed order).  n_split > 1 needs `workspace`: qeft_attn_workspace_bytes(n_heads, n_split) bytes of
 * device memory, 16-byte aligned, ZERO before the first call and not shared by launches that may overlap; the
 * kernel leaves it ready for the next call.  A workspace sized for n_split = 8 serves every n_split, in any order (the
 * arrival counters sit in front of the records, where no split's records reach). */
int qeft_attn_workspace_bytes(int n_heads, int n_split);   /* 0 for n_split == 1 or bad arguments */
int qeft_rope_attn_decode(const void* q, const void* k, const void* v, const void* cos_tab, const void* sin_tab,
                          int tab_rows, void* k_cache, void* v_cache, const int* pos, const int* out_pos, void* out,
                          void* workspace, int n_split, int n_heads, int n_kv_heads, int max_seq, qeft_stream_t stream);

/* The same step on the REFERENCE's cache layout, for the `qeft_cuda.single_query_attention` boundary
 * (qeft/kernel/qeft_cuda.cpp:23-26, ft_attention.cpp:110-181; caller ftllama_modeling.py:139-153):
 *   k_cache_ft  fp16 [n_kv][128/8][max_seq][8]   (FasterTransformer key layout, ft_attention.cpp:131-133)
 *   v_cache     fp16 [n_kv][max_seq][128]
 * one sequence, head_dim 128, neox rotary from the cos/sin table (tab_rows as above), one block per head, natural output
 * order, max_seq % 16 == 0 and at most 32768 as above.  The Python shim loops over the batch; it sends ALiBi to
 * qeft_single_query_attention_alibi and the other head sizes to qeft_single_query_attention_generic (both below), and rotates
 * q / k itself, in front of a launch with an identity table, for a partial or an interleaved (GPT-J) rotary.  It raises for
 * fp32 / bf16 and for head sizes that are no multiple of 8 or above 256. */
int qeft_single_query_attention(const void* q, const void* k, const void* v, const void* cos_tab, const void* sin_tab,
                                int tab_rows, void* k_cache_ft, void* v_cache, const int* pos, void* out, int n_heads,
                                int n_kv_heads, int max_seq, qeft_stream_t stream);
/* qeft_single_query_attention_alibi: the same with the reference's alibi_slopes_ (fp32 [n_heads], ft_attention.cpp:149-154): the
 * head's linear position bias slope * (key position - query position) is added to the scaled score
 * (decoder_masked_multihead_attention_template.hpp:1335-1345). */
int qeft_single_query_attention_alibi(const void* q, const void* k, const void* v, const void* cos_tab, const void* sin_tab,
                                      int tab_rows, void* k_cache_ft, void* v_cache, const int* pos, void* out, int n_heads,
                                      int n_kv_heads, int max_seq, const float* alibi_slopes, qeft_stream_t stream);

/* qeft_single_query_attention_generic (round 4): the same boundary for the other head sizes the reference instantiates
 * (ft_attention.cpp:110-181: 32 .. 256): any head_dim % 8 == 0 in [8, 256], caches k [n_kv][head_dim/8][max_seq][8],
 * v [n_kv][max_seq][head_dim], NO rotary inside (the shim rotates q / k first), optional alibi_slopes (NULL: none). */
int qeft_single_query_attention_generic(const void* q, const void* k, const void* v, void* k_cache_ft, void* v_cache, const int* pos,
                                        void* out, int n_heads, int n_kv_heads, int max_seq, int head_dim, const float* alibi_slopes,
                                        qeft_stream_t stream);

/* ---- v3 decode linear (batch 1): the decode engine's production GEMV (csrc/gemv_v3.h) ------------------------------
 *     y[n] = Wdeq . x (+ bias)                                          (gemv_4bit_qeft, gemv_cuda_qeft.cu:392-513, m = 1)
 * reads the fp16 vector x[k] AS IT IS (no transform of x inside); the decoder's element-wise neighbours sit in the EPILOGUE
 * of the producing launch instead of the prologue of the consuming one (every block stages x by LDS-DMA and starts its
 * weight stream at once):
 *   ssq_in != NULL    x is (v * gamma) of some vector v whose producer also stored n_ssq_in (<= 512) partial sums of v^2
 *                     (readable up to a multiple of 4 floats): y *= rsqrt(sum(ssq_in) / k + eps) -- together the RMSNorm of
 *                     layernorm.cu:26-76 in front of W
 *   mode 1 (PAIR)     the operand's rows are pair-interleaved -- rows [16g, 16g+8) are gate_proj rows [8g, 8g+8), rows
 *                     [16g+8, 16g+16) the same rows of up_proj (a derived buffer, see qeft_amd/fuse.py):
 *                     y[8g + i] = silu(fp16 gate_i) * fp16 up_i, n/2 outputs (the arithmetic of qeft_silu_mul)
 *   residual != NULL  (mode 0) the fp32 residual stream: `residual` and `y` are FLOAT vectors, y = Wx + residual (in place is fine)
 *   gamma_out != NULL (with residual) additionally y_norm = fp16(y * gamma_out) and ssq_out[b] = the sum of y^2 over the rows
 *                     of block b, b < qeft_decode_linear_blocks(n): what the NEXT launch takes as x / ssq_in.
 * Operands: qweight int16 [n/4, k]; sz_packed from qeft_pack_scales (required); oweight PLAIN fp16 [n, 128] (the `oweight`
 * buffer of the checkpoint, not the interleaved copy; NULL when n_out == 0); bias optional.  Several linears that read the
 * same x (q|k|v) are ONE operand: their buffers concatenated along n at load time.
 * Requirements: k % 128 == 0, n_out in {0, 128}, group 128 or k, n % 16 == 0.
 * qeft_gemv_v3_check_extents: CPU-only self-check -- enumerates every address the kernel would form for the configuration
 * and returns how many leave their operand (0 = none; -1 = configuration not accepted); shrink_rows > 0 is the negative
 * control (operands that many rows shorter than the geometry: the count must be positive). */
int qeft_decode_linear_blocks(int n_rows);
int qeft_decode_linear(const void* x, const void* qweight, const void* sz_packed, const void* oweight, const void* bias,
                       void* y, int n, int k, int group_size, int n_out, int mode, const void* residual,
                       const float* ssq_in, int n_ssq_in, float eps, const void* gamma_out, void* y_norm, float* ssq_out,
                       qeft_stream_t stream);
/* qeft_decode_linear_w3: qeft_decode_linear on the 3-bit EXTENSION layout (qweight3 int32 [n/16, ((k - n_out)/128) * 192],
 * see below): 12 bytes per lane and step, every 3-bit field shifted down to bits 0..2 in registers (x stays raw). */
int qeft_decode_linear_w3(const void* x, const void* qweight3, const void* sz_packed, const void* oweight, const void* bias,
                          void* y, int n, int k, int group_size, int n_out, int mode, const void* residual,
                          const float* ssq_in, int n_ssq_in, float eps, const void* gamma_out, void* y_norm, float* ssq_out,
                          qeft_stream_t stream);
/* qeft_decode_linear_hnorm: the same launch with the WHOLE RMSNorm on the consumer -- x is the fp32 vector h [k]; the launch
 * stages fp16(h * gamma_x) (the producers' rounding) and multiplies its row sums by rsqrt(mean(h^2) + eps).  For inputs that
 * no GEMV epilogue produced: the tensor-parallel path's h comes out of an all-reduce (qeft_amd/llama.py).  y fp16 (mode 0: [n],
 * mode 1: [n/2]); no residual / gamma_out forms. */
int qeft_decode_linear_hnorm(const void* h32, const void* gamma_x, const void* qweight, const void* sz_packed, const void* oweight,
                             const void* bias, void* y, int n, int k, int group_size, int n_out, int mode, float eps,
                             qeft_stream_t stream);
long long qeft_gemv_v3_check_extents(int n, int k, int group_size, int n_out, int n_ssq_in, int shrink_rows);
/* The same self-check for the launches the reference's gemv entries make on the CHECKPOINT-layout operands (qeft_gemv_w4,
 * qeft_gemv_w4_qeft, qeft_gemv_w4_fused): scales / scaled_zeros fp16 [k/g][n] staged raw, oweight_interleaved, m = 1..7 batch
 * rows, optional reorder_ids gather; also checks every LDS destination of the staging against the block's LDS carve-up. */
long long qeft_gemv_v3_check_extents_ckpt(int n, int k, int group_size, int n_out, int m, int gather, int shrink_rows);
/* Which instance of the v3 decode GEMV a launch runs (csrc/gemv_v3.hip gemv_v3_plan).  qeft_last_variant
 * says "gemv_v3" for some 170 instances of one kernel template; these two entries say which one.
 * out[QEFT_GEMV_V3_PLAN_INTS] = { blocks, row sets per block (RSC), nsets / blocks, nsets % blocks (that many blocks hold RSC
 * sets, the others one fewer; 0: all hold RSC), waves per block, ring depth D, 1 with an outlier step (OUTL), mode 0 PLAIN / 1 PAIR,
 * bits 4 / 3, 1 for the half with the run-time flag paths (0: the flag-free half), MB (1: one batch row, 2: several), 1 if the
 * batch rows' x is read from global memory (xg), dynamic LDS bytes }.
 * qeft_gemv_v3_plan: host arithmetic only, no GPU needed.  m batch rows (>= 1); flags: the QEFT_V3_F_* bits below the operands
 *   would set (per-channel follows from group_size == k and need not be given).  Returns QEFT_OK, QEFT_ERR_NULL without `out`,
 *   and -1 for what the launcher refuses: a shape outside the requirements above, m > 16, a block that does not fit the LDS,
 *   several rows in PAIR mode / with 3 bits / with XN, XG with one row or with GATHER, XN with SZN, an unknown or contradictory flag.
 *   With QEFT_V3_F_ENGINE_M it answers for qeft_decode_linear_m's m-row launches (flag-free half, MB 2, PLAIN or PAIR) and refuses
 *   m outside 2..8, 3 bits and every flag but XG; that entry asks without XG and, where the x rows do not fit the LDS, with it.
 *   The lab overrides QEFT_GEMV_BLOCKS / _NW / _NW12 / _DEPTH of the process's environment act on it as on the launcher.
 * qeft_gemv_v3_last_plan: what the calling thread's last v3 launch through qeft_decode_linear / _w3 / _hnorm / _m, the gemv
 *   entries or the GEMM entries' few-row route ran (all zero before the first). */
#define QEFT_GEMV_V3_PLAN_INTS 13
#define QEFT_V3_F_PERCH (1u << 24)  /* one group per row (group_size == k) */
#define QEFT_V3_F_XN (1u << 25)     /* qeft_decode_linear_hnorm: the whole RMSNorm in the launch */
#define QEFT_V3_F_SZN (1u << 26)    /* scales / scaled_zeros in the checkpoint layout (the gemv and GEMM entries without sz_packed) */
#define QEFT_V3_F_OWIL (1u << 27)   /* outlier slice from oweight_interleaved (the gemv entries) */
#define QEFT_V3_F_XG (1u << 28)     /* several rows whose x does not fit the LDS: fragments from global memory */
#define QEFT_V3_F_ENGINE_M (1u << 29) /* qeft_gemv_v3_plan only: the plan of qeft_decode_linear_m's m-row launches (m = 2..8) */
#define QEFT_V3_F_GATHER (1u << 31) /* reorder_ids gathered inside the launch */
int qeft_gemv_v3_plan(int n, int k, int group_size, int n_out, int m, int mode, int bits, int flags, int* out);
int qeft_gemv_v3_last_plan(int* out);
/* Compile-time K.  The instances that the decode engine's Llama-2-7B / -13B launches run (q|k|v, o_proj, gate|up at K = 4096 /
 * 5120, down at K = 11008 / 13824; flag-free half, one row, 4 bits, outlier step) are built a second time with K as a template
 * argument: same loads, same arithmetic, same bits, a shorter scalar prologue.  The 13 integers above and
 * qeft_last_variant are the same for both; these two entries say which one a launch takes.
 * qeft_gemv_v3_plan_kct: the K compiled into the instance the plan names, 0 for the run-time-K instance, -1 where
 *   qeft_gemv_v3_plan refuses.  QEFT_GEMV_CTK=0 in the process's environment sends every launch to the run-time-K instance.
 * qeft_gemv_v3_last_kct: the same of the calling thread's last v3 launch (0 before the first). */
int qeft_gemv_v3_plan_kct(int n, int k, int group_size, int n_out, int m, int mode, int bits, int flags);
int qeft_gemv_v3_last_kct(void);

/* Producer-form helpers for the same scheme.
 * qeft_token_begin_norm: qeft_token_begin + h32 = float(embed[*tok]), h_norm = fp16(embed[*tok] * gamma),
 *                        ssq_out[b] (b < qeft_token_begin_norm_blocks(hidden)) = partial sums of squares.
 * qeft_residual_norm:    h_out(fp32) = h(fp32) (+ add(fp16)); with gamma: h_norm = fp16(h_out * gamma), ssq_out[b] likewise
 *                        (tensor-parallel path: the residual add follows an all-reduce; also the stand-alone reference form
 *                        the fused epilogues are tested against). */
int qeft_token_begin_norm_blocks(int hidden);
int qeft_token_begin_norm(const void* embed, const void* tok, const void* rope_tab, const int* pos, void* h32, void* rope_row,
                          const void* gamma, void* h_norm, float* ssq_out, int hidden, int vocab, int max_seq,
                          qeft_stream_t stream);
int qeft_rmsnorm_f32(const void* x32, const void* gamma, void* y, int m, int hidden, float eps, qeft_stream_t stream); /* qeft_rmsnorm on an fp32 input */
/* qeft_rope_rows (prefill helper): NeoX rotary of the first n_heads heads of every row of x (fp16, rows row_stride elements
 * apart, a head = 128 consecutive elements; row_stride = n_heads * 128 for a plain [t][n_heads][128] tensor, the width of the
 * fused q|k|v output for its q and k heads) in place, cos_tab / sin_tab fp32 [t][64]. */
int qeft_rope_rows(void* x, const void* cos_tab, const void* sin_tab, int t, int n_heads, int row_stride,
                   qeft_stream_t stream);
/* qeft_lm_head_f16 (decode harness, token tail): logits[vocab] (fp16) = weight[vocab][hidden] (fp16, the unquantized lm_head)
 * . fp16(rmsnorm(h32) * gamma) -- the final norm of qeft_rmsnorm_f32 and the head GEMV in one launch, fp32 accumulation.
 * hidden in {512, 1024, 2048, 4096, 5120, 8192}. */
int qeft_lm_head_f16(const void* h32, const void* gamma, const void* weight, void* logits, int hidden, int vocab, float eps,
                     qeft_stream_t stream);
int qeft_residual_norm(const void* h32, const void* add, const void* gamma, void* h32_out, void* h_norm, float* ssq_out,
                       int hidden, qeft_stream_t stream);

/* GEMM forward / dX of a 3-bit layer ON the 3-bit stream (round 3): the loader-wave tiers (256 x 128 tiles from 224 tiles and
 * M >= 1024, the forward also 128 x 128 tiles from 112 tiles and M > 128) stage / load the 12-byte lane records and unpack them in
 * registers -- no 3 -> 4-bit expansion pass.  qeft_gemm_w3[_dx]_supported says whether a shape is taken (k % 128 == 0,
 * n_out % 128 == 0, group a power of two >= 64 (dX: a multiple of 128), n % 16 == 0 (dX: n % 64 == 0, n >= 256)); other shapes
 * go through qeft_expand_w3 and the 4-bit entries.  Arguments as qeft_gemm_w4 / qeft_gemm_w4_dx with qweight3 int32
 * [n/16, ((k - n_out)/128) * 192]. */
int qeft_gemm_w3_supported(int m, int n, int k, int group_size, int n_out);
int qeft_gemm_w3(const void* x, const void* qweight3, const void* scales, const void* scaled_zeros, const void* oweight,
                 const void* bias, void* y, int m, int n, int k, int group_size, int n_out, qeft_stream_t stream);
int qeft_gemm_w3_dx_supported(int m, int n, int k, int group_size, int n_out);
int qeft_gemm_w3_dx(const void* dy, const void* qweight3, const void* scales, const void* scaled_zeros, const void* oweight,
                    void* dx, int m, int n, int k, int group_size, int n_out, qeft_stream_t stream);

/* ---- 3-bit EXTENSION (BASELINE config 5).  The reference cannot pack or run 3 bits (QuantLinear asserts
 * bits == 4, qlinear.py:127; its quantiser can produce them, quant.py:8-10 with maxq = 7), so the layout is this
 * library's own, shaped by the decode GEMV (oracle/qeft_oracle.py: pack_w3 / w3_position):
 *   qweight3  int32 [N/16, ((K - n_out)/128) * 192]   12 bytes per (row, 32-k chunk), 16 rows x 128 k contiguous;
 *                                                      the fp16 outlier columns have no 3-bit fields
 * scales / scaled_zeros / oweight / oweight_il / sz_packed are as for 4 bits.
 * Requirements: N % 16 == 0, K % 128 == 0, n_out % 128 == 0, n_out < K, group size 128 or K.
 * qeft_gemv_w3        y[m,N] = x[m,K] . W^T (+ bias, + residual), any m >= 1 (16 rows per weight pass)
 * qeft_gemv_w3_group / qeft_gemv_w3_silu   as their w4 namesakes
 * qeft_expand_w3      rewrites the stream into the 4-bit checkpoint layout int16 [N/4, K] (dead zero nibbles under
 *                     the fp16 columns) so that qeft_gemm_w4 / qeft_gemm_w4_dx / qeft_dequant_w4 serve 3-bit layers:
 *                     reads 3/8 byte and writes 1/2 byte per weight. */
int qeft_gemv_w3(const void* x, const void* qweight3, const void* scales, const void* scaled_zeros,
                 const void* oweight_il, const void* bias, const void* residual, const void* sz_packed, void* y, int m,
                 int n, int k, int group_size, int n_out, qeft_stream_t stream);
int qeft_gemv_w3_group(const void* x, const void* norm_gamma, float norm_eps, int nparts,
                       const void* const* qweight3, const void* const* scales, const void* const* scaled_zeros,
                       const void* const* oweight_il, const void* const* bias, const void* const* sz_packed,
                       void* const* y, const int* n, int k, int group_size, int n_out, qeft_stream_t stream);
int qeft_gemv_w3_silu(const void* gate, const void* up, const void* qweight3, const void* scales,
                      const void* scaled_zeros, const void* oweight_il, const void* bias, const void* residual,
                      const void* sz_packed, void* y, int n, int k, int group_size, int n_out, qeft_stream_t stream);
int qeft_expand_w3(const void* qweight3, void* qweight4, int n, int k, int n_out, qeft_stream_t stream);

/* Token boundary of the decode loop (main.py:340-371, benchmark.py:293-338).
 * begin: h[hidden] = embed[*tok] (tok: device int64, clamped to the vocabulary) and, if rope_row != NULL,
 *        rope_row[128] = rope_tab[*pos] (rope_tab fp32 [max_seq][cos 64 | sin 64]) for qeft_rope_attn_decode(tab_rows = 1).
 * end:   if greedy: *tok = argmax(logits[vocab]) (lowest index among equal maxima); always *pos += 1. */
int qeft_token_begin(const void* embed, const void* tok, const void* rope_tab, const int* pos, void* h, void* rope_row,
                     int hidden, int vocab, int max_seq, qeft_stream_t stream);
int qeft_token_end(const void* logits, void* tok, int* pos, int vocab, int greedy, qeft_stream_t stream);

/* Verify pass of the decode engine (DecodeEngine.verify, assisted decoding): m = 1..8 tokens of ONE sequence at positions
 * *pos .. *pos + m - 1 in one launch sequence of m-row launches (csrc/gemv_v3_multi.hip, csrc/decode_verify.hip).  Rows are
 * contiguous; every entry rejects m outside 1..8 (QEFT_ERR_BATCH) and bad shapes before it touches the device.
 * qeft_decode_linear_m: qeft_decode_linear on m rows -- x [m][k], y [m][n] (mode 1: [m][n/2]), residual / y (fp32) [m][n],
 *   ssq_in [m][n_ssq_in], y_norm [m][n], ssq_out [m][qeft_decode_linear_blocks(n)].  The weights stream once for all rows;
 *   m == 1 is the qeft_decode_linear launch itself.
 * qeft_gemv_v3_check_extents_m: the host-side address enumeration of such a launch (count of out-of-range accesses, -1 for a
 *   configuration the entry rejects; shrink_rows > 0: the negative control).
 * qeft_token_begin_norm_m: qeft_token_begin_norm for tokens[m] (int64) at positions *pos + i: h32 [m][hidden], h_norm [m][hidden],
 *   ssq_out [m][qeft_token_begin_norm_blocks(hidden)], rope_rows [m][128] (cos 64 | sin 64 of position *pos + i).
 * qeft_rope_attn_decode_m: rotary + KV append of m rows + causal attention, query i over keys [0, *pos + i].  q / k / v rows are
 *   qkv_stride elements apart, out rows out_stride; cos / sin: tab_rows == m -> row i (tab_stride floats apart) is position
 *   *pos + i, tab_rows >= max_seq -> indexed by position.  n_split 1 / 2 / 4 / 8 blocks per kv head; n_split > 1 needs a
 *   zeroed workspace of qeft_attn_m_workspace_bytes(n_heads, n_split, m) bytes (its counters re-arm themselves).
 *   max_seq % 16 == 0, 16 <= max_seq <= 32768 (the ceiling of qeft_rope_attn_decode, QEFT_ERR_SHAPE above it).
 * qeft_lm_head_f16_m: qeft_lm_head_f16 on m rows: logits [m][vocab] from h32 [m][hidden]; the head streams once.
 * qeft_verify_greedy: greedy: argmax a[i] of every logits row (lowest index among equal maxima), n = longest prefix with
 *   a[i] == tokens[i + 1]; out_tokens[0..n] = tokens[1..n], a[n]; *n_accepted = n; *tok = a[n]; *pos += n + 1.
 *   greedy == 0: *pos += m only. */
int qeft_decode_linear_m(const void* x, const void* qweight, const void* sz_packed, const void* oweight, const void* bias,
                         void* y, int n, int k, int group_size, int n_out, int mode, const void* residual,
                         const float* ssq_in, int n_ssq_in, float eps, const void* gamma_out, void* y_norm, float* ssq_out,
                         int m, qeft_stream_t stream);
long long qeft_gemv_v3_check_extents_m(int n, int k, int group_size, int n_out, int m, int mode, int n_ssq_in, int shrink_rows);
int qeft_token_begin_norm_m(const void* embed, const void* tokens, const void* rope_tab, const int* pos, void* h, void* rope_rows,
                            const void* gamma, void* h_norm, float* ssq_out, int hidden, int vocab, int max_seq, int m,
                            qeft_stream_t stream);
int qeft_attn_m_workspace_bytes(int n_heads, int n_split, int m);
int qeft_rope_attn_decode_m(const void* q, const void* k, const void* v, int qkv_stride, const void* cos_tab, const void* sin_tab,
                            int tab_stride, int tab_rows, void* k_cache, void* v_cache, const int* pos, const int* out_pos,
                            void* out, int out_stride, void* workspace, int n_split, int n_heads, int n_kv_heads, int max_seq,
                            int m, qeft_stream_t stream);
int qeft_lm_head_f16_m(const void* h32, const void* gamma, const void* weight, void* logits, int hidden, int vocab, float eps,
                       int m, qeft_stream_t stream);
int qeft_verify_greedy(const void* logits, const void* tokens, int m, int vocab, int greedy, void* out_tokens, int* n_accepted,
                       void* tok, int* pos, qeft_stream_t stream);

/* Batched decoding (qeft_amd/batch.py, BatchDecodeEngine): m = 1..8 rows of m DIFFERENT sequences per launch (csrc/decode_batch.hip);
 * the linears and the head are the verify pass's m-row entries above.  Row r serves cache slot slots[r] (device int32 [m]; the
 * slots of one launch are distinct); per slot, on the device: pos, limit, eos, done (int32 [n_slots] each).  KV caches per layer:
 * [n_slots][n_kv_heads][max_seq][128] fp16.  Every entry rejects m outside 1..8 (QEFT_ERR_BATCH) and bad shapes before it
 * touches the device; a row whose slot lies outside [0, n_slots) is left alone.
 * qeft_token_begin_norm_batch: qeft_token_begin_norm_m with row r's rotary row taken at pos[slots[r]] (clamped to the table).
 * qeft_rope_attn_decode_batch: row r, slot s = slots[r], p = pos[s]: rotary of q and k, k / v appended to slot s at p, attention
 *   over keys [0, p] of slot s.  A row with done[s] != 0 (done may be NULL) or p outside [0, max_seq) writes nothing to the cache
 *   and zeros to its output.  q / k / v / out / rotary rows as qeft_rope_attn_decode_m (tab_rows == m: row r; tab_rows >= max_seq:
 *   indexed by p).  n_split 1 / 2 / 4 / 8 blocks per (row, kv head); n_split > 1 needs a zeroed workspace of
 *   qeft_attn_batch_workspace_bytes(n_heads, n_split, m) bytes (its counters re-arm themselves).  max_seq % 16 == 0,
 *   16 <= max_seq <= 32768 (the ceiling of qeft_rope_attn_decode, QEFT_ERR_SHAPE above it).
 * qeft_token_end_batch: k = counter[0] (counter: device int32 [2], zeroed; counter[1] is the launch's own arrival count).  Row r,
 *   slot s: done[s] != 0 -> out[r][k] = -1 only.  Otherwise a = argmax(logits[r]) (lowest index among equal maxima),
 *   tokens[r] = a (int64), out[r][k] = a (int64, out rows out_cap apart, written for k < out_cap), pos[s] += 1, and done[s] = 1 if
 *   a == eos[s] >= 0, else 2 if pos[s] >= limit[s].  counter[0] += 1. */
int qeft_token_begin_norm_batch(const void* embed, const void* tokens, const void* rope_tab, const int* slots, const int* pos, void* h,
                                void* rope_rows, const void* gamma, void* h_norm, float* ssq_out, int hidden, int vocab, int max_seq,
                                int n_slots, int m, qeft_stream_t stream);
int qeft_attn_batch_workspace_bytes(int n_heads, int n_split, int m);
int qeft_rope_attn_decode_batch(const void* q, const void* k, const void* v, int qkv_stride, const void* cos_tab, const void* sin_tab,
                                int tab_stride, int tab_rows, void* k_cache, void* v_cache, const int* slots, const int* pos,
                                const int* done, const int* out_pos, void* out, int out_stride, void* workspace, int n_split,
                                int n_slots, int n_heads, int n_kv_heads, int max_seq, int m, qeft_stream_t stream);
int qeft_token_end_batch(const void* logits, const int* slots, void* tokens, int* pos, const int* limit, const int* eos, int* done,
                         void* out, int* counter, int vocab, int out_cap, int n_slots, int m, qeft_stream_t stream);

/* FP8 KV cache (csrc/decode_attn_kv8.hip; DecodeEngine / BatchDecodeEngine with kv_dtype="fp8").  Per layer and slot:
 *   K codes, V codes   uint8 [n_kv_heads][max_seq][128], OCP e4m3fn (not fnuz)
 *   K scales, V scales fp32  [n_kv_heads][max_seq], one per (kv head, position) row
 * with [n_slots] in front of each for the batch entry.  132 bytes per row where the fp16 cache has 256.
 * THE RECIPE for a row x[128] -- the fp16 values an fp16 cache would hold: K after rotary and rounding to fp16, V the fp16
 * projection -- in fp32 arithmetic:
 *   1. amax = max |x_i|.
 *   2. amax == 0: scale = 0 and every code is 0.
 *   3. otherwise inv = 448.0f / amax and scale = amax / 448.0f (correctly rounded fp32 divides; the build uses no fast-math), and
 *      code_i = e4m3fn, round to nearest even, of clamp(x_i * inv, -448, 448).
 * The value of an element is float(code) * scale.  Both entries below run this recipe through one device function.
 * qeft_rope_attn_decode_kv8: qeft_rope_attn_decode_batch over such a cache, same arguments and rules (row r in slot slots[r] at
 *   p = pos[slots[r]]; a row with a bad slot, done != 0 or p outside [0, max_seq) writes nothing to the cache and zeros to its
 *   output; n_split 1 / 2 / 4 / 8 with a zeroed workspace of qeft_attn_kv8_workspace_bytes(n_heads, n_split, m) bytes, whose
 *   counters re-arm themselves and which, sized for 8, serves every split in any order; head_dim 128, max_seq % 16 == 0,
 *   16 <= max_seq <= 32768).  The launch quantises the new K / V row, appends codes and scale at p, and attends over rows [0, p]
 *   AS THE CACHE HOLDS THEM, its own row included (dequantised), so a token contributes the same whether prefill or a decode step
 *   wrote it.  m = 1, n_slots = 1, slots = {0} serves a single sequence.  Codes 16-byte aligned, scales 4-byte aligned.
 * qeft_kv8_store_rows: quantise n_rows already rotated K rows and V rows (fp16 [n_rows][>= n_kv_heads * 128], rows row_stride
 *   elements apart: views of a fused q|k|v GEMM output) into ONE cache (no slot dimension) at positions p0 .. p0 + n_rows - 1;
 *   p0 >= 0, n_rows >= 1, p0 + n_rows <= max_seq (QEFT_ERR_SHAPE otherwise). */
int qeft_attn_kv8_workspace_bytes(int n_heads, int n_split, int m);   /* 0 for n_split == 1 or bad arguments */
int qeft_rope_attn_decode_kv8(const void* q, const void* k, const void* v, int qkv_stride, const void* cos_tab, const void* sin_tab,
                              int tab_stride, int tab_rows, void* k_codes, void* v_codes, void* k_scales, void* v_scales,
                              const int* slots, const int* pos, const int* done, const int* out_pos, void* out, int out_stride,
                              void* workspace, int n_split, int n_slots, int n_heads, int n_kv_heads, int max_seq, int m,
                              qeft_stream_t stream);
int qeft_kv8_store_rows(const void* k_rows, const void* v_rows, int row_stride, void* k_codes, void* v_codes, void* k_scales,
                        void* v_scales, int n_kv_heads, int max_seq, int p0, int n_rows, qeft_stream_t stream);

/* The verify pass over an FP8 KV cache (csrc/decode_verify_kv8.hip; DecodeEngine with kv_dtype="fp8", kv8_verify=True).
 * qeft_rope_attn_decode_m_kv8: qeft_rope_attn_decode_m over the cache above (ONE sequence: no slot dimension, no slot table), same
 *   arguments and rules: m rows at positions *pos .. *pos + m - 1, query i over keys [0, *pos + i]; *pos < 0 or *pos + m > max_seq
 *   touches nothing; q / k / v / out / rotary rows, out_pos and n_split as there, with a zeroed workspace of
 *   qeft_attn_m_kv8_workspace_bytes(n_heads, n_split, m) bytes whose counters re-arm themselves and which, sized for (8, 8),
 *   serves every (m, n_split) in any order.  The launch quantises the m new K / V rows by THE RECIPE, appends their codes and
 *   scales, and attends over every row AS THE CACHE HOLDS IT, the m new rows included.  Codes 16-byte aligned, scales 4-byte
 *   aligned; head_dim 128, max_seq % 16 == 0, 16 <= max_seq <= 32768. */
int qeft_attn_m_kv8_workspace_bytes(int n_heads, int n_split, int m);   /* 0 for n_split == 1 or bad arguments */
int qeft_rope_attn_decode_m_kv8(const void* q, const void* k, const void* v, int qkv_stride, const void* cos_tab, const void* sin_tab,
                                int tab_stride, int tab_rows, void* k_codes, void* v_codes, void* k_scales, void* v_scales,
                                const int* pos, const int* out_pos, void* out, int out_stride, void* workspace, int n_split,
                                int n_heads, int n_kv_heads, int max_seq, int m, qeft_stream_t stream);

/* Causal prompt attention over the KV cache (csrc/prefill_attn.hip; llama.prefill with attn="own", DecodeEngine.extend, chunked
 * prompts).  t fp16 query rows, already rotated, at positions start .. start + t - 1: row i holds n_heads x 128 elements at
 * q + i * q_stride and attends the cache rows 0 .. start + i inclusive.  k_cache / v_cache: fp16 [n_kv_heads][kv_rows][128], the
 * decode engines' layout, holding positions [0, start + t) -- the caller stores the chunk's own rows BEFORE the launch; rows from
 * start + t on are never used (whatever they hold, NaN included).  out: fp16 [t][n_heads * 128] at out_stride, heads in natural
 * order; head h reads kv head h / (n_heads / n_kv_heads).  Scores are scaled by 128^-0.5 in fp32, the softmax is the online form
 * in fp32 over key tiles of 64 at absolute multiples of 64, P is rounded to fp16 for the P V product (fp32 accumulation): row i's
 * result depends on that row, start + i and the cache alone, bit for bit -- not on how a prompt was cut into chunks.  Strides
 * in elements, multiples of 8 and >= n_heads * 128 (q may be a view of a fused q|k|v output); all four pointers 16-byte
 * aligned; start and t are host integers (not graph-capturable state); no workspace.  QEFT_ERR_SHAPE for t < 1, start < 0,
 * start + t > kv_rows, n_heads % n_kv_heads != 0 or a bad stride, before any pointer is looked at.
 * qeft_attn_prefill_check_extents: CPU-only -- enumerates every global address such a launch would form and returns the largest
 * number of bytes by which one passes the end of its operand, 0 when none does (-1 for arguments the entry refuses). */
int qeft_attn_prefill(const void* q, int q_stride, const void* k_cache, const void* v_cache, int kv_rows, void* out, int out_stride,
                      int start, int t, int n_heads, int n_kv_heads, qeft_stream_t stream);
long long qeft_attn_prefill_check_extents(int q_stride, int kv_rows, int out_stride, int start, int t, int n_heads, int n_kv_heads);

/* The same attention with the past in an FP8 KV cache (csrc/prefill_attn_kv8.hip; llama.prefill / DecodeEngine.extend /
 * BatchDecodeEngine.admit(chunk=) on kv_dtype="fp8").  q, out, start, t, the head layout and every rule as qeft_attn_prefill.
 * Keys [0, start): ONE sequence's cache as laid out above, read in place -- k_codes / v_codes uint8 [n_kv_heads][kv_rows][128]
 * e4m3fn, k_scales / v_scales fp32 [n_kv_heads][kv_rows]; a row's fp16 value is float(code) * scale in fp32, rounded once to
 * fp16 (nearest even, subnormals kept).  Keys [start, start + t): the chunk's own rotated K rows and its V rows in fp16, k_new /
 * v_new [t][>= n_kv_heads * 128], rows new_stride elements apart (views of the fused q|k|v output), attended UNQUANTISED.  The
 * cache's rows at positions >= start are never read (the caller may store the chunk before or after the launch), and with
 * start == 0 no cache value is read at all.  The result is bit-identical to qeft_attn_prefill over the fp16 image
 * [decoded rows 0 .. start - 1 | the new rows].  new_stride % 8 == 0 and >= n_kv_heads * 128 (QEFT_ERR_SHAPE otherwise, with
 * qeft_attn_prefill's shape rules, before any pointer is looked at); q, out, codes and new rows 16-byte aligned, scales 4-byte
 * aligned; no workspace.
 * qeft_attn_prefill_kv8_check_extents: CPU-only, as qeft_attn_prefill_check_extents, over all eight operands. */
int qeft_attn_prefill_kv8(const void* q, int q_stride, const void* k_codes, const void* v_codes, const void* k_scales,
                          const void* v_scales, int kv_rows, const void* k_new, const void* v_new, int new_stride, void* out,
                          int out_stride, int start, int t, int n_heads, int n_kv_heads, qeft_stream_t stream);
long long qeft_attn_prefill_kv8_check_extents(int q_stride, int kv_rows, int new_stride, int out_stride, int start, int t, int n_heads,
                                              int n_kv_heads);

/* Causal attention of the training step (csrc/attn_train.hip; qeft_amd/attention.py: causal_attention; finetune.causal_lm_loss
 * with attn="own").  n_seq sequences of t rows each, every one from position 0 and attending itself
 * alone; sequence b is rows b * t .. b * t + t - 1 of every operand.  q, out, dout, dq: fp16 [n_seq * t][>= n_heads * 128], rows
 * q_stride / out_stride / dout_stride / dq_stride elements apart; k, v (already rotated) and dk, dv: fp16
 * [n_seq * t][>= n_kv_heads * 128] at kv_stride (k and v) and dkv_stride (dk and dv) -- q, k, v may be views of one fused q|k|v
 * buffer, grouped-query layouts are read in place, head h reads kv head h / (n_heads / n_kv_heads); lse: fp32
 * [n_seq * t][n_heads], contiguous.
 * qeft_attn_train_fwd: `out` is, bit for bit, what qeft_attn_prefill gives at start = 0 over a cache holding the same K / V (the
 * same body); lse[row][head] = m + log(l) of the row's online softmax over the scaled scores.
 * qeft_attn_train_bwd: from q, k, v, the forward's out and lse, and dout, three launches -- delta[row][head] = sum_d dout * out in
 * fp32 into `workspace` (qeft_attn_train_bwd_workspace_bytes = 4 * n_seq * t * n_heads, no initialisation, nothing kept); dK / dV,
 * one workgroup per 128 keys of one (sequence, kv head), which sweeps the group's query heads and the query tiles in ascending
 * order with its accumulators on chip; dQ, one workgroup per (sequence, head, 128 rows), which walks the key tiles in ascending
 * order.  p = exp(s * 128^-0.5 - lse) in fp32, P rounded to fp16 for dV, dS = p * (dP - delta) in fp32 rounded once to fp16 (the
 * same value in both launches), 128^-0.5 applied to dK and dQ in fp32 at the end.  No atomics and no workgroup waits on another:
 * every output element is written exactly once (the outputs need no initialisation), and a sequence's out, lse, dq, dk, dv do
 * not depend on n_seq, on its index or on any stride, bit for bit; out / lse / dq row i depend on rows <= i alone.
 * QEFT_ERR_SHAPE, before any pointer is looked at: t < 1, n_seq < 1, n_seq * t > 2^20, n_heads % n_kv_heads != 0, a stride that is
 * no multiple of 8 or narrower than its heads, a workspace shorter than qeft_attn_train_bwd_workspace_bytes; then QEFT_ERR_NULL
 * (every pointer is required); then QEFT_ERR_ALIGN (16 bytes; 4 for lse).  n_seq and t are host integers; no host
 * synchronisation, capturable into a graph.  Rows past a sequence's end are read from its clamped last row and never stored.
 * qeft_attn_train_bwd_workspace_bytes: 0 for arguments the entries refuse.
 * qeft_attn_train_bwd_part: ONE of the three launches alone under the same rules and arguments -- part 0 delta (writes the
 * workspace), 1 dK / dV, 2 dQ (both read the workspace a part 0 call left there); QEFT_ERR_SHAPE for any other part.  For timing
 * a launch on its own and for tests that name the kernel that ran; parts 0, 1, 2 in this order are qeft_attn_train_bwd.
 * qeft_attn_train_check_extents / qeft_attn_train_bwd_check_extents: CPU-only -- enumerate every global address the forward /
 * the three backward launches would form and return the largest number of bytes by which one passes the end of its operand or
 * runs in front of it, 0 when none does (-1 for arguments the entries refuse). */
int qeft_attn_train_fwd(const void* q, int q_stride, const void* k, const void* v, int kv_stride, void* out, int out_stride, float* lse,
                        int n_seq, int t, int n_heads, int n_kv_heads, qeft_stream_t stream);
long long qeft_attn_train_check_extents(int q_stride, int kv_stride, int out_stride, int n_seq, int t, int n_heads, int n_kv_heads);
long long qeft_attn_train_bwd_workspace_bytes(int n_seq, int t, int n_heads, int n_kv_heads);
int qeft_attn_train_bwd(const void* q, int q_stride, const void* k, const void* v, int kv_stride, const void* out, int out_stride,
                        const void* dout, int dout_stride, const float* lse, void* dq, int dq_stride, void* dk, void* dv,
                        int dkv_stride, void* workspace, long long workspace_bytes, int n_seq, int t, int n_heads, int n_kv_heads,
                        qeft_stream_t stream);
int qeft_attn_train_bwd_part(const void* q, int q_stride, const void* k, const void* v, int kv_stride, const void* out, int out_stride,
                             const void* dout, int dout_stride, const float* lse, void* dq, int dq_stride, void* dk, void* dv,
                             int dkv_stride, void* workspace, long long workspace_bytes, int n_seq, int t, int n_heads, int n_kv_heads,
                             int part, qeft_stream_t stream);
long long qeft_attn_train_bwd_check_extents(int q_stride, int kv_stride, int out_stride, int dout_stride, int dq_stride, int dkv_stride,
                                            int n_seq, int t, int n_heads, int n_kv_heads);

/* The same attention over PACKED sequences of unequal length (the varlen kernels of csrc/attn_train.hip; qeft_amd/attention.py:
 * causal_attention_packed; finetune.causal_lm_loss(seq_lens=...)).  The operands are those above over R
 * rows; `n_seq, t` give way to `seq_rows, n_seq`: seq_rows is a HOST array of n_seq + 1 ints, the prefix of the lengths --
 * seq_rows[0] = 0, strictly increasing, seq_rows[n_seq] = R -- and sequence i is rows seq_rows[i] .. seq_rows[i + 1] - 1 of every
 * operand, from position 0, attending itself alone.  The prefix is copied into the launches' arguments during the call (nothing
 * on the device, nothing read after the call returns; capturable into a graph, which then holds these lengths).  The bodies are
 * those of the fixed-length kernels: a sequence's out, lse, dq, dk, dv are, bit for bit, what qeft_attn_train_fwd / _bwd give
 * for that sequence alone, whatever is packed around it, in whatever order and at whatever strides.  Grids (blocks of the
 * longest sequence, n_seq); the delta launch runs over the R rows as it is.  Workspace: 4 * R * n_heads bytes.
 * QEFT_ERR_SHAPE: n_seq outside 1 .. 128, the head and stride rules above; then QEFT_ERR_NULL for seq_rows (it is read here);
 * then QEFT_ERR_SHAPE for a prefix that does not start at 0, is not strictly increasing or ends above 2^20, and for a short
 * workspace -- all before any device pointer is looked at; then QEFT_ERR_NULL, then QEFT_ERR_ALIGN as above.
 * _bwd_workspace_bytes: 0 for what the entries refuse; _bwd_part, _check_extents, _bwd_check_extents: as their namesakes above. */
int qeft_attn_train_varlen_fwd(const void* q, int q_stride, const void* k, const void* v, int kv_stride, void* out, int out_stride,
                               float* lse, const int* seq_rows, int n_seq, int n_heads, int n_kv_heads, qeft_stream_t stream);
long long qeft_attn_train_varlen_check_extents(int q_stride, int kv_stride, int out_stride, const int* seq_rows, int n_seq, int n_heads,
                                               int n_kv_heads);
long long qeft_attn_train_varlen_bwd_workspace_bytes(const int* seq_rows, int n_seq, int n_heads, int n_kv_heads);
int qeft_attn_train_varlen_bwd(const void* q, int q_stride, const void* k, const void* v, int kv_stride, const void* out, int out_stride,
                               const void* dout, int dout_stride, const float* lse, void* dq, int dq_stride, void* dk, void* dv,
                               int dkv_stride, void* workspace, long long workspace_bytes, const int* seq_rows, int n_seq, int n_heads,
                               int n_kv_heads, qeft_stream_t stream);
int qeft_attn_train_varlen_bwd_part(const void* q, int q_stride, const void* k, const void* v, int kv_stride, const void* out,
                                    int out_stride, const void* dout, int dout_stride, const float* lse, void* dq, int dq_stride,
                                    void* dk, void* dv, int dkv_stride, void* workspace, long long workspace_bytes, const int* seq_rows,
                                    int n_seq, int n_heads, int n_kv_heads, int part, qeft_stream_t stream);
long long qeft_attn_train_varlen_bwd_check_extents(int q_stride, int kv_stride, int out_stride, int dout_stride, int dq_stride,
                                                   int dkv_stride, const int* seq_rows, int n_seq, int n_heads, int n_kv_heads);

/* The glue of the training step (csrc/train_glue.hip; qeft_amd/glue.py: add_rmsnorm, swiglu; finetune.causal_lm_loss
 * with glue="fused"): forwards over a batch of rows and a backward for each.  Memory-bound row kernels:
 * 16-byte accesses, fp32 math, every output rounded to fp16 exactly once, no atomics, no workspace.  A row's results depend on
 * that row's operands alone, bit for bit -- not on the number of rows, the row's index, a stride or the grid.
 * Common rules: hidden, n and every stride are multiples of 8, a stride is at least the row's width (and at most 2^24), the row
 * count m is 1 .. 2^20.  QEFT_ERR_SHAPE for anything else, before any pointer is looked at; then QEFT_ERR_NULL; then
 * QEFT_ERR_ALIGN (16 bytes).  No host synchronisation, capturable.
 *
 * qeft_add_rmsnorm_fwd: h, add, sum_out, y fp16 [m][hidden] dense, gamma fp16 [hidden].  s = fp16(h + add), written to sum_out
 *   (add == NULL: s = h, and sum_out must be NULL too; one without the other is QEFT_ERR_NULL); y = fp16(s * rsqrt(mean s^2 +
 *   eps) * gamma).  The bits of sum_out and y are qeft_rmsnorm's on the same operands.
 * qeft_add_rmsnorm_bwd: gamma is frozen -- no d(gamma), no reduction across rows.  With r = rsqrt(mean s^2 + eps) recomputed
 *   from s (no statistics are saved), xhat = s r and c = (1 / hidden) sum_k gamma_k dy_k xhat_k:
 *   dsum_j = fp16(float(dres_j) + r (gamma_j dy_j - xhat_j c)), the gradient of h and of add alike.  dres is the gradient that
 *   reaches s along the residual stream, dy the one of y; a NULL one is zero, both NULL is QEFT_ERR_SHAPE.  One launch: each row
 *   is read once per pass (two passes) and stays in fp32 from the reductions to the store.
 * qeft_swiglu_fwd: out[m][n] (dense) = fp16(silu(gate) * up), the bits of qeft_silu_mul; gate, up [m][>= n] at their strides.
 * qeft_swiglu_bwd: with sigma = 1 / (1 + e^-g): dup = fp16(dact g sigma), dgate = fp16(dact u sigma (1 + g (1 - sigma))); sigma
 *   and 1 - sigma come from one __expf(-|g|) and one hardware reciprocal without cancellation or overflow, so the results are
 *   finite for every finite fp16 gate.  dact, dgate, dup [m][>= n] at their own strides.
 * qeft_train_glue_check_extents: CPU-only -- enumerates every global address the launch of `op` would form and returns the
 *   largest number of bytes by which one passes the end of its operand or runs in front of it, 0 when none does (-1 for
 *   arguments the entry refuses or an unknown op).  rows = m, width = hidden / n; strides: SwiGLU forward gate_stride,
 *   up_stride; SwiGLU backward gate_stride, up_stride, dact_stride, dgate_stride, dup_stride; the rest ignored. */
#define QEFT_GLUE_ADD_RMSNORM_FWD 0
#define QEFT_GLUE_ADD_RMSNORM_BWD 1
#define QEFT_GLUE_SWIGLU_FWD 2
#define QEFT_GLUE_SWIGLU_BWD 3
int qeft_add_rmsnorm_fwd(const void* h, const void* add, const void* gamma, void* sum_out, void* y, int m, int hidden, float eps,
                         qeft_stream_t stream);
int qeft_add_rmsnorm_bwd(const void* s, const void* gamma, const void* dy, const void* dres, void* dsum, int m, int hidden, float eps,
                         qeft_stream_t stream);
int qeft_swiglu_fwd(const void* gate, const void* up, void* out, int m, int n, int gate_stride, int up_stride, qeft_stream_t stream);
int qeft_swiglu_bwd(const void* gate, const void* up, const void* dact, void* dgate, void* dup, int m, int n, int gate_stride,
                    int up_stride, int dact_stride, int dgate_stride, int dup_stride, qeft_stream_t stream);
long long qeft_train_glue_check_extents(int op, int rows, int width, int stride0, int stride1, int stride2, int stride3, int stride4);

/* The rotary of the training step (csrc/train_glue.hip; qeft_amd/glue.py: rope_qk; finetune.causal_lm_loss with rope="fused";
 * DESIGN.md section 4.17): every head of q and of k in one launch, and the same kernel as its own backward.
 *   q fp16 [rows][n_heads][128], rows q_stride elements apart; k fp16 [rows][n_kv_heads][128], rows k_stride apart (a [B T] view
 *   of a fused q|k|v buffer passes as it lies); q_out, k_out the same shapes, dense, not overlapping the inputs; cos_tab, sin_tab
 *   fp32 [t_len][64].  Row r is at position r % t_len: every sequence starts at 0, rows % t_len == 0.
 * NeoX pairs (a, b) = (x[i], x[i + 64]), c = cos[pos][i], s = sin[pos][i]:
 *   inverse = 0:  lo = a c - b s,  hi = b c + a s
 *   inverse = 1:  lo = a c + b s,  hi = b c - a s   -- the transpose: the backward, applied to the gradients of q_out and k_out; it
 *                 needs the tables alone, not the forward's inputs.  Bit for bit inverse = 0 with a negated sin table, except
 *                 that a result of -0 is returned as +0: autograd sums the gradients of the two half-slices of x, each padded
 *                 with +0, so the torch route never hands on a -0, and the inverse adds the same +0 to its fp16 results.
 * The arithmetic is pinned: each of the two products is rounded to fp32 on its own, their sum or difference is rounded to fp32,
 * and that value is converted to fp16 (round to nearest even); nothing is contracted into an FMA.  This is what the torch
 * expression of finetune._rope and its autograd compute, one rounding per torch op, so rope="fused" equals the torch route bit
 * for bit in both directions, and a head's bits depend on its 128 values and its position alone -- not on the head counts, the
 * row count, a stride or the grid.  Bit parity with qeft_rope_rows is NOT a goal and does not hold: that kernel rounds some
 * heads once and some twice, depending on how many heads its operand has; both meet the same fp64 bound.
 * Memory-bound: 16-byte accesses of q and k, fp32 math, no LDS, no atomics, no workspace, no host synchronisation, capturable.
 * rows 1 .. 2^20, t_len >= 1 and rows % t_len == 0, n_heads and n_kv_heads 1 .. 256, strides multiples of 8, at least heads x 128
 * (and at most 2^24), inverse 0 or 1: QEFT_ERR_SHAPE otherwise, before any pointer is looked at; then QEFT_ERR_NULL for any of
 * the six pointers; then QEFT_ERR_ALIGN (16 bytes).
 * qeft_rope_qk_check_extents: CPU-only, in the manner of qeft_train_glue_check_extents -- the largest number of bytes by which
 *   any address that any thread of any block of that launch forms (q, k, q_out, k_out, both tables) leaves its operand, 0 when
 *   none does, -1 for arguments the entry refuses. */
int qeft_rope_qk(const void* q, const void* k, const void* cos_tab, const void* sin_tab, void* q_out, void* k_out, int rows, int t_len,
                 int n_heads, int n_kv_heads, int q_stride, int k_stride, int inverse, qeft_stream_t stream);
long long qeft_rope_qk_check_extents(int rows, int t_len, int n_heads, int n_kv_heads, int q_stride, int k_stride);

/* The update of the training step (csrc/oweight_optim.hip, csrc/oweight_optim.h; qeft_amd/optim.py: OWeightAdamW;
 * finetune.train_step): loss-scale removal, overflow detection, global-norm clipping and AdamW in two
 * launches over ONE flat fp32 arena.  p, g, m, v: fp32 [n], the parameters, their (loss-scaled) gradients and the two moments;
 * n % 64 == 0, 0 < n <= 2^31 - 2^20.  No atomics, no host synchronisation, nothing read back, capturable.
 * The state is a 32-byte record in device memory, 16-byte aligned, 8 words in this order:
 *   float scale; int step; int good_steps; int skipped_last; int n_skipped; float grad_norm; float clip_coef; int reserved
 * (step counts applied updates only).  A step reads state_in and writes state_out, which must be another record: every block
 * reads the one, block 0 writes the other, and the caller swaps them afterwards.
 * Geometry: 256 threads, 16-byte accesses, U = 2 chunks per thread per iteration, min(ceil(n / 4 / (256 U)), 2048) blocks at a
 * fixed grid stride; which thread takes which element depends on n alone, so the results do not depend on the device.
 * qeft_oweight_grad_stats: x = g * (1 / scale) (one rounding), each thread adds x * x in fp32 in program order, the block folds its
 *   256 sums through a fixed tree and stores ONE fp32 partial: partials fp32 [qeft_oweight_optim_blocks(n)].  An inf or NaN
 *   gradient makes its partial non-finite; that is the overflow signal.
 * qeft_oweight_adamw: every block adds all partials in double in index order (the same bits in every block) and takes
 *   norm = sqrt(sum).  A non-finite sum skips the step: no element of p, m, v is touched; state_out = state_in with
 *   skipped_last = 1, n_skipped + 1, good_steps = 0 and, when dynamic, scale * backoff_factor.  Otherwise
 *   coef = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1 (torch's clip_grad_norm_; 0 turns clipping off), t = step + 1,
 *   bc1 = 1 - beta1^t, bc2 = 1 - beta2^t (double), and per element, in fp32 with one rounding per operation and no FMA:
 *     gh = g * (1 / scale) * coef;   p1 = p * (1 - lr * weight_decay);   m' = m + (gh - m) * (1 - beta1);
 *     v' = beta2 * v + (1 - beta2) * (gh * gh);   p' = p1 - float(lr / bc1) * (m' / (sqrt(v') / float(sqrt(bc2)) + eps))
 *   (csrc/oweight_optim.h states the order of every operation).  g is left as it is.  state_out: step = t, good_steps + 1,
 *   skipped_last = 0, grad_norm = norm, clip_coef = coef; when dynamic and good_steps reaches growth_interval, scale *
 *   growth_factor and good_steps = 0.  An element whose p, g, m, v are all zero stays zero, so zero padding stays zero.
 * Both refuse, before any HIP call and in this order: QEFT_ERR_SHAPE (n <= 0, n % 64 != 0, n above the ceiling; for the update
 *   also a beta outside [0, 1), eps <= 0, a scale factor <= 0, a negative lr, weight_decay or max_norm, growth_interval < 1, dynamic
 *   other than 0 or 1), then QEFT_ERR_NULL (every pointer is required; state_out == state_in counts as a missing record), then
 *   QEFT_ERR_ALIGN (16 bytes).
 * qeft_oweight_optim_blocks: CPU-only, the grid of both launches and the length of partials (0 for a refused n).
 * qeft_oweight_optim_thread_elems: CPU-only, the most elements one thread adds into its sum (0 for a refused n).
 * qeft_oweight_optim_check_extents: CPU-only -- walks every address both launches form and returns how many fall outside
 *   [0, n), plus the number of 16-byte chunks of the arena not visited exactly once; 0 when all is well, -1 for a refused n.
 * qeft_oweight_optim_lab: for measurement (tools/bench_oweight_optim.py): u = 1, 2 or 4 chunks per thread per iteration (0: the
 *   built-in choice), nontemporal_g = 1: launch 2 loads g, its last use, non-temporally.  Process-wide; the three functions
 *   above follow it.  The results' bits depend on u (the order of a thread's sum), not on nontemporal_g. */
int qeft_oweight_optim_lab(int u, int nontemporal_g);
int qeft_oweight_optim_blocks(long long n);
long long qeft_oweight_optim_thread_elems(long long n);
long long qeft_oweight_optim_check_extents(long long n);
int qeft_oweight_grad_stats(const void* g, long long n, const void* state_in, void* partials, qeft_stream_t stream);
int qeft_oweight_adamw(void* p, const void* g, void* m, void* v, long long n, const void* state_in, void* state_out,
                       const void* partials, float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm,
                       float growth_factor, float backoff_factor, int growth_interval, int dynamic, qeft_stream_t stream);

/* Fused lm_head + cross-entropy pieces (csrc/lm_head_nll.hip; qeft_amd/scoring.py: lm_head_nll, score, eval_nll; DESIGN.md
 * section 4.13).  x: fp16 [t][hidden], the final-norm output rows, x_stride elements apart; weight: fp16 [vocab][hidden]
 * contiguous, the checkpoint's lm_head.weight; targets: int32 [t], or NULL.  logit_ij = sum_k x_ik w_jk is accumulated in fp32 by
 * MFMA and never rounded to fp16 or stored: no [t][vocab] array exists.  Per row i:
 *   lse[i]       = log sum_j exp(logit_ij)   (fp32; max-shifted, so finite for any finite logits);
 *   tgt_logit[i] = logit at targets[i]; a target outside [0, vocab) (-100, the reference's IGNORE_INDEX, among them) is ignored
 *                  and gives 0.0; with NULL targets tgt_logit is not touched and may be NULL;
 *   argmax[i]    = the lowest index among equal maxima, as qeft_token_end's (int32); argmax may be NULL.
 * A row's three results depend on that row and the weight alone, bit for bit: not on t, on the row's index in the launch, on
 * x_stride or on the grid.  The vocabulary is cut into column tiles at absolute multiples of 128; each (row, tile) leaves one
 * partial {max, sum exp(l - max), first argmax} in `workspace` (12 bytes x t x ceil(vocab / 128), qeft_lm_head_nll_workspace_bytes)
 * and a second launch folds a row's partials in ascending tile order; no atomics, no arrival order.  The workspace needs no
 * initialisation and holds nothing between calls.
 * t >= 1, hidden % 64 == 0, hidden >= 64, vocab >= 1, x_stride % 8 == 0, x_stride >= hidden, a workspace of at least
 * qeft_lm_head_nll_workspace_bytes(t, vocab) bytes (t <= 2^20, vocab <= 2^24, hidden <= 2^16): QEFT_ERR_SHAPE otherwise, before any
 * pointer is looked at; then QEFT_ERR_NULL (x, weight, lse, workspace; tgt_logit when targets is given), then QEFT_ERR_ALIGN
 * (x, weight, workspace 16-byte aligned; targets and the outputs 4-byte aligned).  t is a host integer; no host synchronisation,
 * capturable into a graph.  Rows >= t and columns >= vocab of the last tiles are read from the clamped row / column, never past
 * an operand's end, and never stored.
 * qeft_lm_head_nll_workspace_bytes: 0 for a t or vocab the entry refuses.
 * qeft_lm_head_nll_check_extents: CPU-only -- enumerates every global address the two launches would form and returns the largest
 * number of bytes by which one passes the end of its operand, 0 when none does (-1 for arguments the entry refuses). */
long long qeft_lm_head_nll_workspace_bytes(int t, int vocab);
int qeft_lm_head_nll(const void* x, int x_stride, const void* weight, const int* targets, float* lse, float* tgt_logit, int* argmax,
                     void* workspace, long long workspace_bytes, int t, int hidden, int vocab, qeft_stream_t stream);
long long qeft_lm_head_nll_check_extents(int x_stride, int t, int hidden, int vocab);

/* Backward of the fused head with respect to x (csrc/lm_head_nll_grad.hip; qeft_amd/scoring.py: lm_head_nll_loss;
 * qeft_amd/finetune.py: causal_lm_loss).  x, weight, targets as in qeft_lm_head_nll (targets required);
 * lse: fp32 [t], qeft_lm_head_nll's own output; grad_nll: fp32 [t], the gradient arriving at nll_i = lse_i - tgt_logit_i;
 * dx: [t][hidden], rows dx_stride elements apart, fp16, or fp32 when dx_fp32 != 0.  For a row with a target in [0, vocab)
 *   dx[i][k] = grad_nll[i] * sum_j (p_ij - [j == targets[i]]) * weight[j][k],   p_ij = exp(logit_ij - lse[i]);
 * a row with an ignored target gets +0.0 in every element whatever grad_nll[i] holds.  The lm_head is frozen in QEFT: there is
 * no d(weight).  Rows are taken in chunks of R = qeft_lm_head_nll_grad_chunk_rows (1024); per chunk launch A recomputes the
 * forward's fp32 logits (the same loop, bit for bit) and writes g = fp16(p - onehot), rounded once, as [rows][vocab rounded up
 * to 128] into `workspace`; launch B forms g W with fp32 MFMA accumulators over the whole vocabulary in ascending order, reading
 * weight where it lies (no transposed copy), multiplies by grad_nll in fp32 and writes fp32 or rounds once to fp16: the fp16
 * output is the rounding of the fp32 output, bit for bit.  No atomics, no arrival order: a row of dx depends on that row of x,
 * its lse, target and grad_nll and on the weight alone, bit for bit -- not on t, the row's index or chunk, a stride or the grid.
 * The forward's shape rules, dx_stride % 8 == 0, dx_stride >= hidden and a workspace of at least
 * qeft_lm_head_nll_grad_workspace_bytes(t, hidden, vocab) = 2 * min(t, R) * round_up(vocab, 128) bytes: QEFT_ERR_SHAPE otherwise,
 * before any pointer is looked at; then QEFT_ERR_NULL (every pointer is required), then QEFT_ERR_ALIGN (x, weight, dx, workspace
 * 16-byte aligned; targets, lse, grad_nll 4-byte aligned).  The workspace needs no initialisation and holds nothing between
 * calls.  No host synchronisation, capturable into a graph.  Rows and columns past an operand's end are read from the clamped
 * row / column and never stored.
 * qeft_lm_head_nll_grad_workspace_bytes: 0 for arguments the entry refuses.
 * qeft_lm_head_nll_grad_check_extents: CPU-only, as qeft_lm_head_nll_check_extents, in elements, over every launch of every
 * chunk (-1 for arguments the entry refuses). */
int qeft_lm_head_nll_grad_chunk_rows(int hidden, int vocab);
long long qeft_lm_head_nll_grad_workspace_bytes(int t, int hidden, int vocab);
int qeft_lm_head_nll_grad(const void* x, int x_stride, const void* weight, const int* targets, const float* lse,
                          const float* grad_nll, void* dx, int dx_stride, int dx_fp32, void* workspace, long long workspace_bytes,
                          int t, int hidden, int vocab, qeft_stream_t stream);
long long qeft_lm_head_nll_grad_check_extents(int x_stride, int dx_stride, int t, int hidden, int vocab);

/* Calibration (csrc/calib.hip, csrc/calib.h; qeft_amd/calibrate.py).
 * qeft_hessian_accum: H <- beta * H + alpha * X^T X.  x fp16 [t][k] row-major, h fp32 [k][k], both 16-byte aligned, k % 64 == 0,
 *   64 <= k <= 32768, 1 <= t <= 2^24 (QEFT_ERR_SHAPE otherwise).  MFMA on the fp16 operands (their products are exact in fp32),
 *   fp32 accumulation over the rows in ONE fixed ascending order that depends on neither the grid nor the device; no atomics.
 *   Epilogue with S the fp32 sum: fl(fl(beta * H[i][j]) + fl(alpha * S)), nothing contracted.  H[i][j] is read for i <= j only
 *   (not at all with beta == 0: the term is +0) and the result is stored to H[i][j] AND H[j][i]: the triangles agree bit for bit.
 * qeft_hessian_accum_check_extents: CPU-only -- walks every address a launch forms and returns how many leave x or h, plus the
 *   elements of h not written exactly once (0 = none; -1 for arguments the entry refuses and for k > 4096: the walk keeps a
 *   byte per element of h and visits every thread).
 * qeft_gptq_block: `count` (1..128) columns of the GPTQ error-feedback loop for n rows in one launch, fp32 throughout.
 *   w1 [n][ld_w] (the block's columns in place inside the working matrix; updated), hinv1 [count][ld_h] (the diagonal block of
 *   the upper Cholesky factor of the inverse Hessian, in place; the upper triangle is read), scale / zero fp32 [n], maxq 7 or 15,
 *   q1 / err1 fp32 [n][count] (written).  Per row, for i = 0 .. count - 1, every operation rounded once, nothing contracted,
 *   IEEE division, rint = round half to even:
 *     x = w_i / scale;  c = min(max(rint(x) + zero, 0), maxq);  q1_i = scale * (c - zero);  err1_i = (w_i - q1_i) / hinv1[i][i];
 *     w_j = w_j - fl(err1_i * hinv1[i][j])  for j = i .. count - 1.
 *   A row's results do not depend on n, the row's index or the grid.  QEFT_ERR_SHAPE: n < 1, count outside 1..128, ld_w or ld_h
 *   below count, another maxq.  Pointers 4-byte aligned. */
int qeft_hessian_accum(const void* x, void* h, int t, int k, float alpha, float beta, qeft_stream_t stream);
long long qeft_hessian_accum_check_extents(int t, int k);
int qeft_gptq_block(void* w1, int ld_w, const void* hinv1, int ld_h, const void* scale, const void* zero, void* q1, void* err1, int n,
                    int count, int maxq, qeft_stream_t stream);

/* Sampled token end (csrc/decode_sample.hip, qeft_amd/sampling.py). A parameter record is int32 [8] in device memory:
 * temperature (fp32 bits), top_k, top_p (fp32 bits), seed lo, seed hi, 3 reserved zeros.  Per row, in HF's warper order:
 *   temperature T == 0: the argmax (lowest index among equal maxima), bit-identical to qeft_token_end / qeft_token_end_batch;
 *     otherwise weights w = exp((l - max l) / T) in fp32 (NaN: weight 0, never drawn; -0 == +0);
 *   top_k (0 or >= vocab: off): keep every logit >= the k-th largest (ties at the boundary kept);
 *   top_p (1: off): keep token j iff the top-k survivors' weight above l_j (strictly greater logits) is below top_p * Z, Z their
 *     total weight;
 *   draw: x0 = word 0 of Philox4x32-10 at counter (p, 0, 0, 0), key (seed lo, seed hi), u = x0 / 2^32; the token is the first
 *     kept token in index order whose inclusive cumulative weight exceeds u * Z_kept.  p is the position the drawn token will
 *     occupy.  The result depends only on (row, record, p): not on m, the row index, the slot or a replay.
 * Records live on the device, so a captured graph picks up new parameters without a recapture.  logits, params 16-byte aligned.
 * qeft_sample: m >= 1 rows, row r uses params[r] and p = positions[r] (int32 [m]); tokens_out int64 [m].
 * qeft_token_end_sample: qeft_token_end(greedy = 1)'s contract (*tok = the token, *pos += 1) with p = *pos + 1.
 * qeft_token_end_sample_batch: qeft_token_end_batch's contract exactly, with row r drawing with params[slots[r]] (params: records
 *   [n_slots][8]) at p = pos[slots[r]] + 1.
 * qeft_verify_sample: qeft_verify_greedy(greedy = 1)'s contract for m = 1..8 rows of ONE sequence with the argmax replaced by the
 *   draw: a[i] = the token of logits row i with the record params (one record) at p = *pos + i + 1, i.e. what
 *   qeft_token_end_sample would draw there; n = longest prefix with a[i] == tokens[i + 1]; out_tokens[0..n] = tokens[1..n], a[n];
 *   *n_accepted = n; *tok = a[n]; *pos += n + 1.  T == 0 gives qeft_verify_greedy's outputs bit for bit.  One block per row;
 *   work: QEFT_VERIFY_SAMPLE_WORK int32 in device memory, zeroed once by the caller: work[0..m) = a[i] of the last call,
 *   work[8] the launch's arrival count (0 again after every call, so graph replays need no memset), the rest unused. */
#define QEFT_VERIFY_SAMPLE_WORK 16
int qeft_sample(const void* logits, int vocab, int m, const int* params, const int* positions, void* tokens_out,
                qeft_stream_t stream);
int qeft_token_end_sample(const void* logits, void* tok, int* pos, int vocab, const int* params, qeft_stream_t stream);
int qeft_token_end_sample_batch(const void* logits, const int* slots, void* tokens, int* pos, const int* limit, const int* eos,
                                int* done, void* out, int* counter, const int* params, int vocab, int out_cap, int n_slots, int m,
                                qeft_stream_t stream);
int qeft_verify_sample(const void* logits, const void* tokens, int m, int vocab, const int* params, int* work, void* out_tokens,
                       int* n_accepted, void* tok, int* pos, qeft_stream_t stream);

/* One-shot all-reduce of the tensor-parallel decode path (csrc/oneshot.hip; no reference counterpart --
 * the reference places whole layers on GPUs, qeft/utils/modelutils.py:21-57).  In-place fp32 sum of t[n] over `world` ranks
 * (one process per GPU) by ONE kernel per rank: every rank writes its partial as 8-byte {value, tag} granules into slot `rank`
 * of every rank's MAILBOX (device memory of the owning rank, mapped into the peers through hipIpcMemHandle: the export / open /
 * close wrappers below), polls its own mailbox and sums the slots in rank order -- bit-identical on every rank.
 *   boxes:  HOST array of `world` device pointers, box[r] = rank r's mailbox as mapped in THIS process (box[rank] = the local
 *           allocation from qeft_oneshot_mailbox_alloc); each qeft_oneshot_mailbox_bytes(world, n) bytes, zeroed once;
 *   seq:    one zeroed uint32 in device memory (the call counter: every rank must make the same sequence of calls);
 *   status: two zeroed uint32 in device memory; status[0] != 0 after a call = a wait gave up (a peer never wrote).
 * hipGraph-capturable (no host state changes per call); world <= qeft_oneshot_max_world(). */
long long qeft_oneshot_mailbox_bytes(int world, int n);
int qeft_oneshot_max_world(void);
/* set-up helpers -- the ONLY entry points that allocate / synchronise: the mailbox is a zeroed hipMalloc block of its own (an
 * IPC handle exports the whole allocation its pointer lives in; a caching allocator's sub-block would arrive at an unknown offset) */
int qeft_oneshot_mailbox_alloc(int world, int n, void** dev_ptr_out);
int qeft_oneshot_mailbox_free(void* dev_ptr);
int qeft_oneshot_ipc_export(void* dev_ptr, void* handle_out /* 64 bytes, host */);
int qeft_oneshot_ipc_open(const void* handle /* 64 bytes, host */, void** dev_ptr_out);
int qeft_oneshot_ipc_close(void* dev_ptr);
int qeft_oneshot_allreduce_f32(void* t, int n, void* const* boxes, int rank, int world, void* seq, void* status,
                               qeft_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* QEFT_HIP_H */
