// Geometry and index arithmetic of the training glue (train_glue.hip; DESIGN.md sections 4.16, 4.17): RMSNorm with its fused
// residual add and SiLU(gate) * up, each with its backward, and the rotary of q and k (one kernel, both directions).  Shared by the kernels and by the host-side address
// enumeration behind qeft_train_glue_check_extents: every global address a launch forms comes out of one of the tg_*_off
// functions below (tg_rope_* for the rotary), in elements, at 16-byte chunks of 8 fp16 (4 fp32 for the rotary's tables).
//
//   norm      h, add, sum_out, y, s, dy, dres, dsum   [m][hidden] fp16, dense;  gamma [hidden] fp16
//   SwiGLU    gate, up, dact, dgate, dup  [m][>= n] fp16, each at its own stride; the forward's out [m][n] dense
//   rotary    q [rows][n_heads][128], k [rows][n_kv_heads][128] fp16 at their row strides; q_out, k_out the same, dense;
//             cos, sin [t_len][64] fp32, row r at position r % t_len
#pragma once
#include <hip/hip_runtime.h>

namespace qeft {

constexpr int TG_THREADS = 256;

struct TgNorm {
    int m, hidden;
};
struct TgSwiglu {
    int m, n, gate_stride, up_stride, dact_stride, dgate_stride, dup_stride;
};

// ---- norm: one block per row; thread `tid` takes chunks tid, tid + 256, ...
__host__ __device__ inline int tg_norm_chunks(const TgNorm& G) { return G.hidden / 8; }
__host__ __device__ inline long long tg_norm_off(const TgNorm& G, int row, int chunk) { return (long long)row * G.hidden + chunk * 8; }
__host__ __device__ inline int tg_gamma_off(int chunk) { return chunk * 8; }

// ---- SwiGLU: one 16-byte chunk per thread, chunk = block * 256 + tid over m * (n / 8) chunks in row-major order
__host__ __device__ inline long long tg_swiglu_chunks(const TgSwiglu& G) { return (long long)G.m * (G.n / 8); }
__host__ __device__ inline long long tg_swiglu_blocks(const TgSwiglu& G) { return (tg_swiglu_chunks(G) + TG_THREADS - 1) / TG_THREADS; }
__host__ __device__ inline long long tg_swiglu_chunk(long long block, int tid) { return block * TG_THREADS + tid; }
__host__ __device__ inline long long tg_swiglu_off(const TgSwiglu& G, long long chunk, int stride) {
    const int per_row = G.n / 8;
    return chunk / per_row * stride + chunk % per_row * 8;
}

// ---- rotary: 8 threads per head (thread `lane` of them owns chunk `lane` of the low half and of the high half), `slots`
// such groups per row (a power of two <= 32: the smallest that holds every head of q and k, 32 from 32 heads on), 32 / slots
// rows per block.  A group walks heads slot, slot + slots, ... of its row, q's heads first, then k's.
struct TgRope {
    int rows, t_len, n_heads, n_kv_heads, q_stride, k_stride;
};
constexpr int TG_ROPE_GROUPS = TG_THREADS / 8;
__host__ __device__ inline int tg_rope_heads(const TgRope& G) { return G.n_heads + G.n_kv_heads; }
__host__ __device__ inline int tg_rope_slots(const TgRope& G) {
    int s = 1;
    while (s < TG_ROPE_GROUPS && s < tg_rope_heads(G)) s *= 2;
    return s;
}
__host__ __device__ inline int tg_rope_blocks(const TgRope& G) {
    const int per_block = TG_ROPE_GROUPS / tg_rope_slots(G);
    return (G.rows + per_block - 1) / per_block;
}
__host__ __device__ inline int tg_rope_lane(int tid) { return tid & 7; }
__host__ __device__ inline int tg_rope_slot(int tid, int slots) { return (tid >> 3) & (slots - 1); }
__host__ __device__ inline int tg_rope_row(int block, int tid, int slots) { return block * (TG_ROPE_GROUPS / slots) + (tid >> 3) / slots; }
// tables: the 8 fp32 of chunk `lane` as two loads of 4, part = 0, 1
__host__ __device__ inline int tg_rope_tab_off(const TgRope& G, int row, int lane, int part) { return row % G.t_len * 64 + lane * 8 + part * 4; }
// head `head` (< n_heads: of q, else head - n_heads of k) of `row`, chunk `lane` of half `half`, in an operand at `stride`
__host__ __device__ inline long long tg_rope_off(int row, int head_in_operand, int lane, int half, int stride) {
    return (long long)row * stride + head_in_operand * 128 + half * 64 + lane * 8;
}

// ---- host side: train_glue.hip
hipError_t add_rmsnorm_fwd_launch(const void* h, const void* add, const void* gamma, void* sum_out, void* y, const TgNorm& G, float eps,
                                  hipStream_t st);
hipError_t add_rmsnorm_bwd_launch(const void* s, const void* gamma, const void* dy, const void* dres, void* dsum, const TgNorm& G,
                                  float eps, hipStream_t st);
hipError_t swiglu_fwd_launch(const void* gate, const void* up, void* out, const TgSwiglu& G, hipStream_t st);
hipError_t swiglu_bwd_launch(const void* gate, const void* up, const void* dact, void* dgate, void* dup, const TgSwiglu& G,
                             hipStream_t st);
hipError_t rope_qk_launch(const void* q, const void* k, const void* cos_tab, const void* sin_tab, void* q_out, void* k_out,
                          const TgRope& G, bool inverse, hipStream_t st);
long long train_glue_rope_count_out_of_range(const TgRope& G);
long long train_glue_norm_count_out_of_range(const TgNorm& G);
long long train_glue_swiglu_count_out_of_range(const TgSwiglu& G, bool backward);

}  // namespace qeft
