// Geometry and index arithmetic of the training glue (train_glue.hip): RMSNorm with its fused residual
// add and SiLU(gate) * up, each with its backward.  Shared by the kernels and by the host-side address
// enumeration behind qeft_train_glue_check_extents: every global address a launch forms comes out of one of the tg_*_off
// functions below, in elements, at 16-byte chunks of 8 fp16.
//
//   norm      h, add, sum_out, y, s, dy, dres, dsum   [m][hidden] fp16, dense;  gamma [hidden] fp16
//   SwiGLU    gate, up, dact, dgate, dup  [m][>= n] fp16, each at its own stride; the forward's out [m][n] dense
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

// ---- host side: train_glue.hip
hipError_t add_rmsnorm_fwd_launch(const void* h, const void* add, const void* gamma, void* sum_out, void* y, const TgNorm& G, float eps,
                                  hipStream_t st);
hipError_t add_rmsnorm_bwd_launch(const void* s, const void* gamma, const void* dy, const void* dres, void* dsum, const TgNorm& G,
                                  float eps, hipStream_t st);
hipError_t swiglu_fwd_launch(const void* gate, const void* up, void* out, const TgSwiglu& G, hipStream_t st);
hipError_t swiglu_bwd_launch(const void* gate, const void* up, const void* dact, void* dgate, void* dup, const TgSwiglu& G,
                             hipStream_t st);
long long train_glue_norm_count_out_of_range(const TgNorm& G);
long long train_glue_swiglu_count_out_of_range(const TgSwiglu& G, bool backward);

}  // namespace qeft
