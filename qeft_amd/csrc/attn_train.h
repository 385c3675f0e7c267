// Geometry and index arithmetic of the training attention (attn_train.hip), shared by the kernels and by
// the host-side address enumerations behind qeft_attn_train_check_extents and qeft_attn_train_bwd_check_extents: every global
// address a launch forms comes out of one of the at_*_off functions below (the forward: of prefill_attn.h's, behind a
// per-sequence base), with its row already clamped into the sequence.
//
// n_seq sequences of t rows each, every one from position 0; sequence b is rows b t .. b t + t - 1 of every operand:
//   q, out, dout, dq  [n_seq t][>= n_heads 128]  fp16 at q_stride / out_stride / dout_stride / dq_stride
//   k, v              [n_seq t][>= n_kv 128]     fp16 at kv_stride (both)            dk, dv the same at dkv_stride (both)
//   lse, delta        [n_seq t][n_heads]         fp32, contiguous
//
// The variable-length launches take the same operands over R rows with sequence i at rows
// cu[i] .. cu[i + 1] - 1: a block builds the AtGeom of its own sequence alone (at_var_seq) and offsets every pointer by
// at_var_base, and everything behind that is the code above, at seq = 0.
#pragma once
#include "prefill_attn.h"

namespace qeft {

constexpr int AT_KB = 128;                  // keys per block of the dK / dV launch: 4 waves of 32 keys
constexpr int AT_QT = 64;                   // query rows per tile of the dK / dV launch, at absolute multiples of 64
constexpr int AT_THREADS = 256;
constexpr int AT_DELTA_PAIRS = AT_THREADS / 16;     // (row, head) pairs per block of the delta launch, 16 lanes each

struct AtGeom {
    Pa8Geom f;                              // f.g: q_stride, kv_rows = t, out_stride, start = 0, t, n_heads, n_kv; f.new_stride = kv_stride
    int dout_stride, dq_stride, dkv_stride, n_seq;
};

__host__ __device__ inline long long at_seq_base(const AtGeom& A, int seq, int stride) { return (long long)seq * A.f.g.t * stride; }
__host__ __device__ inline int at_row(const AtGeom& A, int row) {            // a row clamped into its sequence
    const int last = A.f.g.t - 1;
    return row < last ? (row > 0 ? row : 0) : last;
}
// element offsets; `chunk` counts 8 elements (16 bytes); `row` is a row of sequence `seq`
__host__ __device__ inline long long at_q_off(const AtGeom& A, int seq, int row, int head, int chunk) {
    return at_seq_base(A, seq, A.f.g.q_stride) + (long long)row * A.f.g.q_stride + head * PA_HD + chunk * 8;
}
__host__ __device__ inline long long at_out_off(const AtGeom& A, int seq, int row, int head, int chunk) {
    return at_seq_base(A, seq, A.f.g.out_stride) + (long long)row * A.f.g.out_stride + head * PA_HD + chunk * 8;
}
__host__ __device__ inline long long at_dout_off(const AtGeom& A, int seq, int row, int head, int chunk) {
    return at_seq_base(A, seq, A.dout_stride) + (long long)row * A.dout_stride + head * PA_HD + chunk * 8;
}
__host__ __device__ inline long long at_kv_off(const AtGeom& A, int seq, int row, int kvh, int chunk) {
    return at_seq_base(A, seq, A.f.new_stride) + (long long)row * A.f.new_stride + kvh * PA_HD + chunk * 8;
}
__host__ __device__ inline long long at_dq_off(const AtGeom& A, int seq, int row, int head, int d) {
    return at_seq_base(A, seq, A.dq_stride) + (long long)row * A.dq_stride + head * PA_HD + d;
}
__host__ __device__ inline long long at_dkv_off(const AtGeom& A, int seq, int row, int kvh, int d) {
    return at_seq_base(A, seq, A.dkv_stride) + (long long)row * A.dkv_stride + kvh * PA_HD + d;
}
__host__ __device__ inline long long at_lse_off(const AtGeom& A, int seq, int row, int head) {
    return ((long long)seq * A.f.g.t + row) * A.f.g.n_heads + head;
}

// ---- forward and dQ launches: one block per (sequence, head, 128-row Q tile), prefill_attn.h's order inside a sequence
__host__ __device__ inline int at_q_blocks_per_seq(const AtGeom& A) { return pa_q_tiles(A.f.g) * A.f.g.n_heads; }
__host__ __device__ inline long long at_q_blocks(const AtGeom& A) { return (long long)A.n_seq * at_q_blocks_per_seq(A); }

// ---- delta launch: pair = global row * n_heads + head, 16 lanes (one 16-byte chunk each) per pair
__host__ __device__ inline long long at_delta_pairs(const AtGeom& A) { return (long long)A.n_seq * A.f.g.t * A.f.g.n_heads; }
__host__ __device__ inline long long at_delta_blocks(const AtGeom& A) { return (at_delta_pairs(A) + AT_DELTA_PAIRS - 1) / AT_DELTA_PAIRS; }
__host__ __device__ inline long long at_delta_pair(const AtGeom& A, long long block, int slot) {     // clamped: loaded, not stored
    const long long pair = block * AT_DELTA_PAIRS + slot, last = at_delta_pairs(A) - 1;
    return pair < last ? pair : last;
}

// ---- dK / dV launch: one block per (sequence, key block, kv head); key block 0 (the one with the most queries) first
__host__ __device__ inline int at_kblocks(const AtGeom& A) { return (A.f.g.t + AT_KB - 1) / AT_KB; }
__host__ __device__ inline long long at_dkv_blocks(const AtGeom& A) { return (long long)A.n_seq * at_kblocks(A) * A.f.g.n_kv; }
__host__ __device__ inline int at_dkv_seq(const AtGeom& A, int block) { return block / (at_kblocks(A) * A.f.g.n_kv); }
__host__ __device__ inline int at_dkv_kblock(const AtGeom& A, int block) { return block % (at_kblocks(A) * A.f.g.n_kv) / A.f.g.n_kv; }
__host__ __device__ inline int at_dkv_kvh(const AtGeom& A, int block) { return block % A.f.g.n_kv; }
// the query tiles a key block sweeps: from its own diagonal to the sequence's last row
__host__ __device__ inline int at_dkv_first_tile(int kblock) { return kblock * (AT_KB / AT_QT); }
__host__ __device__ inline int at_dkv_end_tile(const AtGeom& A) { return (A.f.g.t - 1) / AT_QT + 1; }

// ---- variable-length launches: n_seq <= AT_MAX_SEQ sequences of cu[i + 1] - cu[i] >= 1 rows, the prefix by value in the kernel
// arguments (no device-side table: what the host validated is what the kernel reads)
constexpr int AT_MAX_SEQ = 128;
struct AtVarGeom {
    AtGeom a;                               // strides and heads; a.f.g.t = a.f.g.kv_rows = the LONGEST sequence (the grids), a.n_seq
    int cu[AT_MAX_SEQ + 1];                 // cu[0] = 0 < cu[1] < ... < cu[n_seq] = R; the rest unused
};
__host__ __device__ inline int at_var_rows(const AtVarGeom& V) { return V.cu[V.a.n_seq]; }
__host__ __device__ inline long long at_var_base(const AtVarGeom& V, int seq, int stride) { return (long long)V.cu[seq] * stride; }
// sequence `seq` as one sequence of its own length: the geometry every at_* / pa_* function above takes, at seq = 0
__host__ __device__ inline AtGeom at_var_seq(const AtVarGeom& V, int seq) {
    AtGeom A = V.a;
    A.f.g.t = A.f.g.kv_rows = V.cu[seq + 1] - V.cu[seq];
    A.n_seq = 1;
    return A;
}
// all R rows as one sequence: the delta launch is row-wise over global rows
__host__ __device__ inline AtGeom at_var_all(const AtVarGeom& V) {
    AtGeom A = V.a;
    A.f.g.t = A.f.g.kv_rows = at_var_rows(V);
    A.n_seq = 1;
    return A;
}
// grids (x, y = n_seq): x covers the longest sequence; a block whose x is past its own sequence's count returns at once.  Within
// a sequence x is the block index of the fixed-length launches: the heaviest Q tile first, key block 0 first.
__host__ __device__ inline int at_dkv_blocks_per_seq(const AtGeom& A) { return at_kblocks(A) * A.f.g.n_kv; }
__host__ __device__ inline int at_var_q_grid_x(const AtVarGeom& V) { return at_q_blocks_per_seq(V.a); }
__host__ __device__ inline int at_var_dkv_grid_x(const AtVarGeom& V) { return at_dkv_blocks_per_seq(V.a); }

// ---- host side: attn_train.hip
hipError_t attn_train_fwd_launch(const void* q, const void* k, const void* v, void* out, float* lse, const AtGeom& A, hipStream_t st);
hipError_t attn_train_bwd_launch(const void* q, const void* k, const void* v, const void* out, const void* dout, const float* lse,
                                 void* dq, void* dk, void* dv, float* delta, const AtGeom& A, int parts, hipStream_t st);
long long attn_train_fwd_count_out_of_range(const AtGeom& A);
long long attn_train_bwd_count_out_of_range(const AtGeom& A);
hipError_t attn_train_varlen_fwd_launch(const void* q, const void* k, const void* v, void* out, float* lse, const AtVarGeom& V,
                                        hipStream_t st);
hipError_t attn_train_varlen_bwd_launch(const void* q, const void* k, const void* v, const void* out, const void* dout,
                                        const float* lse, void* dq, void* dk, void* dv, float* delta, const AtVarGeom& V, int parts,
                                        hipStream_t st);
long long attn_train_varlen_fwd_count_out_of_range(const AtVarGeom& V);
long long attn_train_varlen_bwd_count_out_of_range(const AtVarGeom& V);

}  // namespace qeft
