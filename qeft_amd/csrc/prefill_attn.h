// Geometry and index arithmetic of the prompt attention (prefill_attn.hip), shared by the kernel and by the host-side address
// enumeration behind qeft_attn_prefill_check_extents: every global address the kernel forms comes out of one of the pa_*_off
// functions below, with its row already clamped into the operand by pa_q_row / pa_key_row.
#pragma once
#include <hip/hip_runtime.h>

namespace qeft {

constexpr int PA_HD = 128;                  // head size
constexpr int PA_WAVES = 4;                 // waves per block, 32 query rows each
constexpr int PA_QT = 32 * PA_WAVES;        // query rows per block
constexpr int PA_KT = 64;                   // keys per tile; tiles sit at absolute multiples of 64 from position 0
constexpr int PA_THREADS = 64 * PA_WAVES;
constexpr int PA_CHUNKS = PA_KT * PA_HD / 8;                 // 16-byte pieces of one K (or V) tile
constexpr int PA_STAGE = PA_CHUNKS / PA_THREADS;             // pieces per thread

struct PaGeom {
    int q_stride, kv_rows, out_stride, start, t, n_heads, n_kv;
};

__host__ __device__ inline int pa_q_tiles(const PaGeom& G) { return (G.t + PA_QT - 1) / PA_QT; }
// key tiles a Q tile walks: through the diagonal of its last real row
__host__ __device__ inline int pa_key_tiles(const PaGeom& G, int qtile) {
    const int last = qtile * PA_QT + PA_QT - 1 < G.t ? qtile * PA_QT + PA_QT - 1 : G.t - 1;
    return (G.start + last) / PA_KT + 1;
}
// the launch order: the heaviest (last) Q tiles first, the heads of one kv group next to each other
__host__ __device__ inline int pa_block_qtile(const PaGeom& G, int block) { return pa_q_tiles(G) - 1 - block / G.n_heads; }
__host__ __device__ inline int pa_block_head(const PaGeom& G, int block) { return block % G.n_heads; }
__host__ __device__ inline int pa_kv_head(const PaGeom& G, int head) { return head / (G.n_heads / G.n_kv); }

// query row of lane row r of wave `wave`; rows past the chunk repeat its last row (computed, never stored)
__host__ __device__ inline int pa_q_row(const PaGeom& G, int qtile, int wave, int r) {
    const int row = qtile * PA_QT + wave * 32 + r;
    return row < G.t ? row : G.t - 1;
}
// cache row of row `row` of key tile `tile`; rows past the context repeat its last row (K: masked; V: zeroed at staging)
__host__ __device__ inline int pa_key_row(const PaGeom& G, int tile, int row) {
    const int key = tile * PA_KT + row, len = G.start + G.t;
    return key < len ? key : len - 1;
}
// element offsets; `chunk` counts 8 elements (16 bytes)
__host__ __device__ inline long long pa_q_off(const PaGeom& G, int row, int head, int chunk) {
    return (long long)row * G.q_stride + head * PA_HD + chunk * 8;
}
__host__ __device__ inline long long pa_kv_off(const PaGeom& G, int kvh, int key, int chunk) {
    return ((long long)kvh * G.kv_rows + key) * PA_HD + chunk * 8;
}
__host__ __device__ inline long long pa_out_off(const PaGeom& G, int row, int head, int d) {
    return (long long)row * G.out_stride + head * PA_HD + d;
}
// lse of the training forward: fp32 [t][n_heads], contiguous
__host__ __device__ inline long long pa_lse_off(const PaGeom& G, int row, int head) { return (long long)row * G.n_heads + head; }

// ---- the same attention with K / V of the past read from an e4m3 cache (prefill_attn_kv8.hip): keys [0, start) are rows of the
// codes uint8 [n_kv][kv_rows][128] and scales fp32 [n_kv][kv_rows], keys [start, start + t) rows of the chunk's own fp16 K / V,
// [t][>= n_kv * 128] at new_stride.  The source is chosen per key row; each row index is clamped into its own operand.
struct Pa8Geom {
    PaGeom g;
    int new_stride;
};
__host__ __device__ inline bool pa8_from_cache(const PaGeom& G, int key) { return key < G.start; }
__host__ __device__ inline int pa8_cache_row(const PaGeom& G, int key) {
    const int row = key < G.start - 1 ? key : G.start - 1;
    return row > 0 ? row : 0;
}
__host__ __device__ inline int pa8_new_row(const PaGeom& G, int key) {
    const int row = key - G.start < G.t - 1 ? key - G.start : G.t - 1;
    return row > 0 ? row : 0;
}
// byte offset of a chunk's codes (`chunk` as above: 8 elements; the kernel loads the aligned 16 bytes of chunk pair
// pa8_code_pair(chunk)), element offset of the row's scale, element offset into the new rows
__host__ __device__ inline int pa8_code_pair(int chunk) { return chunk & ~1; }
__host__ __device__ inline long long pa8_code_off(const PaGeom& G, int kvh, int row, int chunk) {
    return ((long long)kvh * G.kv_rows + row) * PA_HD + chunk * 8;
}
__host__ __device__ inline long long pa8_scale_off(const PaGeom& G, int kvh, int row) { return (long long)kvh * G.kv_rows + row; }
__host__ __device__ inline long long pa8_new_off(const Pa8Geom& G8, int row, int kvh, int chunk) {
    return (long long)row * G8.new_stride + kvh * PA_HD + chunk * 8;
}

// head dimension of accumulator register e of d-block db in lane half h (the 32x32 C/D map), first of a group of four
__host__ __device__ inline int pa_acc_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// ---- host side: prefill_attn.hip, prefill_attn_kv8.hip
hipError_t prefill_attn_launch(const void* q, const void* kc, const void* vc, void* out, const PaGeom& G, hipStream_t st);
long long prefill_attn_count_out_of_range(const PaGeom& G);
hipError_t prefill_attn_kv8_launch(const void* q, const void* kq, const void* vq, const void* ksc, const void* vsc, const void* kn,
                                   const void* vn, void* out, const Pa8Geom& G8, hipStream_t st);
long long prefill_attn_kv8_count_out_of_range(const Pa8Geom& G8);

}  // namespace qeft
