// Device code that the m-row launches of the verify pass (decode_verify.hip) and of batched decoding (decode_batch.hip) share.
//   token_begin_norm_row   the body of token_begin_norm_m / token_begin_norm_b (they differ in the rotary row's position)
//   block_argmax_1024      the argmax of verify_greedy / token_end_b
//   row_slot, attn_b_ctr_floats   the slot table and the workspace layout of the batched attention kernels (fp16 cache:
//                          decode_batch.hip; e4m3 cache: decode_attn_kv8.hip)
//   attn_m_ctr_floats      the workspace layout of the m-row same-sequence attention kernels
// The two attention kernels (rope_attn_m / rope_attn_b) are the same algorithm too, but stay written out in their files: moved
// into shared device functions their R = 32 instantiation compiles to other code (profiles/attn_rows_refactor.log).  The e4m3
// pair (rope_attn_m_kv8 / rope_attn_kv8, R <= 8) stays written out as well and shares its host side only (decode_kv8.h): every
// cut of shared device code made the one-row kernel slower (profiles/kv8_attn_core_refactor.log).
#pragma once
#include "qeft_common.h"

namespace qeft {

// slot of row `row`, or -1 for a slot outside [0, n_slots) (such a row is left alone)
__device__ __forceinline__ int row_slot(const int* __restrict__ slot_tab, int row, int n_slots) {
    const int s = slot_tab[row];
    return s >= 0 && s < n_slots ? s : -1;
}

// floats in front of the split records of a batched attention workspace: the arrival counters, one per (row, kv head, chunk)
__host__ __device__ constexpr size_t attn_b_ctr_floats(int n_heads) { return ((size_t)8 * n_heads + 15) / 16 * 16; }

// floats in front of the split records of an m-row same-sequence attention workspace (fp16 cache: decode_verify.hip; e4m3 cache:
// decode_verify_kv8.hip): the arrival counters, one per (kv head, chunk), at an offset that does not depend on (m, S)
__host__ __device__ constexpr size_t attn_m_ctr_floats(int n_heads) { return ((size_t)n_heads + 15) / 16 * 16; }

// ---- token begin of one row (grid = (pieces of 2048 elements, rows), block 256): embedding of toks[row] -> h32 row, the first
// norm's producer form, the piece's sum of squares; block 0 copies the rotary row of position row_pos() (clamped to the table).
template <class RowPos>
__device__ __forceinline__ void token_begin_norm_row(const f16* __restrict__ embed, const long long* __restrict__ toks,
                                                     const float* __restrict__ rope_tab, float* __restrict__ h,
                                                     float* __restrict__ rope_rows, const f16* __restrict__ gamma,
                                                     f16* __restrict__ hnorm, float* __restrict__ ssq_out, int hidden, int vocab,
                                                     int max_seq, RowPos row_pos) {
    __shared__ float sm[4];
    const int row = blockIdx.y, nb = gridDim.x;
    const long long tk = min(max(toks[row], 0ll), (long long)vocab - 1);
    const int i = (blockIdx.x * 256 + threadIdx.x) * 8;
    float* const hr = h + (size_t)row * hidden;
    float ss = 0.f;
    if (i < hidden) {
        const h8 v = *(const h8*)(embed + (size_t)tk * hidden + i), g = *(const h8*)(gamma + i);
        h8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            ss += (float)v[j] * (float)v[j];
            o[j] = mul_f32_to_f16((float)v[j], (float)g[j]);
            hr[i + j] = (float)v[j];
        }
        *(h8*)(hnorm + (size_t)row * hidden + i) = o;
    }
    ss = wave_sum(ss);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sm[wave] = ss;
    __syncthreads();
    if (threadIdx.x == 0) ssq_out[(size_t)row * nb + blockIdx.x] = sm[0] + sm[1] + sm[2] + sm[3];
    if (blockIdx.x == 0 && threadIdx.x < 128) {
        const int p = min(max(row_pos(row), 0), max_seq - 1);
        rope_rows[(size_t)row * 128 + threadIdx.x] = rope_tab[(size_t)p * 128 + threadIdx.x];
    }
}

// ---- argmax of lg[0 .. vocab) by a block of 1024: the lowest index among equal maxima (0 when nothing compares greater than
// -inf), as token_end.  bv / bi: [16] LDS.  Thread 0 holds the result; the caller owns the barrier before bv / bi are reused.
__device__ __forceinline__ int block_argmax_1024(const f16* lg, int vocab, float* bv, int* bi) {
    const int t = threadIdx.x;
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int i = t * 8; i < vocab; i += 1024 * 8) {
        if (i + 8 <= vocab && (vocab & 7) == 0) {
            const h8 v = *(const h8*)(lg + i);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if ((float)v[j] > best) { best = (float)v[j]; idx = i + j; }
        } else {
            for (int j = i; j < min(i + 8, vocab); ++j)
                if ((float)lg[j] > best) { best = (float)lg[j]; idx = j; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(idx, o);
        if (ob > best || (ob == best && oi < idx)) { best = ob; idx = oi; }
    }
    if ((t & 63) == 0) { bv[t >> 6] = best; bi[t >> 6] = idx; }
    __syncthreads();
    if (t == 0)
        for (int w = 1; w < 16; ++w)
            if (bv[w] > best || (bv[w] == best && bi[w] < idx)) { best = bv[w]; idx = bi[w]; }
    return idx == 0x7fffffff ? 0 : idx;
}

// ---- host side
// Operands of one row-wise attention launch, by name, as the C ABI entry hands them to rope_attn_m_launch / rope_attn_b_launch
// (fp16 cache) and rope_attn_kv8_launch / rope_attn_m_kv8_launch (e4m3 cache, decode_kv8.h).  Host only: the kernels take
// their arguments one by one.  A launcher reads what its kernel has: ks / vs with an e4m3 cache, slot_tab / done / n_slots
// with rows of different sequences; the others stay zero.
struct AttnRowsArgs {
    const void *q, *k, *v;          // the new rows, qkv_stride apart
    const void *cs, *sn;            // rotary tables, tab_stride apart, tab_rows of them
    void *kc, *vc;                  // the cache (fp16, or e4m3 codes)
    void *ks, *vs;                  // e4m3 cache: its scales
    const int *slot_tab, *pos, *done, *out_pos;
    void *out, *ws;
    int qkv_stride, tab_stride, tab_rows, out_stride;
    int n_slots, n_heads, n_kv, max_seq, S, m;      // S: the split
};

// decode_verify.hip: m rows of one sequence
hipError_t token_begin_norm_m_launch(const void* embed, const void* toks, const void* rope_tab, const int* pos, void* h,
                                     void* rope_rows, const void* gamma, void* hnorm, float* ssq_out, int hidden, int vocab,
                                     int max_seq, int m, hipStream_t st);
size_t attn_m_workspace_bytes(int n_heads, int S, int m);
hipError_t rope_attn_m_launch(const AttnRowsArgs& a, hipStream_t st);
hipError_t lm_head_m_launch(const void* h32, const void* gamma, const void* W, void* logits, int H, int vocab, float eps, int m,
                            hipStream_t st);
hipError_t verify_greedy_launch(const void* logits, const void* tokens, int m, int vocab, int greedy, void* out_tokens, int* n_acc,
                                void* tok, int* pos, hipStream_t st);
// decode_batch.hip: m rows of m sequences
hipError_t token_begin_norm_b_launch(const void* embed, const void* toks, const void* rope_tab, const int* slot_tab,
                                     const int* pos_tab, void* h, void* rope_rows, const void* gamma, void* hnorm, float* ssq_out,
                                     int hidden, int vocab, int max_seq, int n_slots, int m, hipStream_t st);
size_t attn_b_workspace_bytes(int n_heads, int S, int m);
hipError_t rope_attn_b_launch(const AttnRowsArgs& a, hipStream_t st);
hipError_t token_end_b_launch(const void* logits, const int* slot_tab, void* tok, int* pos_tab, const int* limit, const int* eos,
                              int* done, void* out, int* ctr, int vocab, int out_cap, int n_slots, int m, hipStream_t st);

}  // namespace qeft
