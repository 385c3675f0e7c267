// Causal prompt attention over the decode engines' KV cache (qeft_attn_prefill).
//
// t already rotated fp16 query rows at positions start .. start + t - 1 attend the cache rows [0, start + i]; the caller has
// stored the chunk's own K / V rows before the launch.  The attention itself is pa_attend (prefill_attn_body.h); this file is
// its staging step over an fp16 cache: K and V tiles copied as they lie, 16 bytes per thread and piece.
// No workspace, no atomics, no split over keys.  Every global address comes from prefill_attn.h, clamped into its operand;
// prefill_attn_count_out_of_range walks the same functions on the CPU.
#include "prefill_attn_body.h"

namespace qeft {

// K and V tiles from the fp16 cache, as they lie: 16-byte pieces, the V rows past the context zeroed
struct PaStageF16 {
    const f16* __restrict__ kc;
    const f16* __restrict__ vc;
    const PaGeom& G;
    int kvh, tid, kv_len;
    u32x4 kst[PA_STAGE], vst[PA_STAGE];

    __device__ __forceinline__ void load(int tile) {
#pragma unroll
        for (int i = 0; i < PA_STAGE; ++i) {
            const int c = tid + PA_THREADS * i, row = c >> 4, ch = c & 15;
            const long long off = pa_kv_off(G, kvh, pa_key_row(G, tile, row), ch);
            kst[i] = *(const u32x4*)(kc + off);
            const u32x4 v = *(const u32x4*)(vc + off);
            vst[i] = tile * PA_KT + row < kv_len ? v : u32x4{0u, 0u, 0u, 0u};
        }
    }
    __device__ __forceinline__ void store(int, unsigned char* lds_k, unsigned char* lds_v) {
#pragma unroll
        for (int i = 0; i < PA_STAGE; ++i) {
            const int c = tid + PA_THREADS * i, row = c >> 4, ch = c & 15;
            *(u32x4*)(lds_k + pa_k_lds(row, ch)) = kst[i];
            *(u32x4*)(lds_v + pa_v_lds(row, ch)) = vst[i];
        }
    }
};

__global__ __launch_bounds__(PA_THREADS) void prefill_attn_kernel(const f16* __restrict__ q, const f16* __restrict__ kc,
                                                                  const f16* __restrict__ vc, f16* __restrict__ out, PaGeom G) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_k[PA_KT * PA_HD * 2];
    __shared__ __attribute__((aligned(16))) unsigned char lds_v[PA_KT * PA_HD * 2];
    PaStageF16 stage{kc, vc, G, pa_kv_head(G, pa_block_head(G, blockIdx.x)), (int)threadIdx.x, G.start + G.t};
    pa_attend(q, out, G, stage, lds_k, lds_v, blockIdx.x);
}

hipError_t prefill_attn_launch(const void* q, const void* kc, const void* vc, void* out, const PaGeom& G, hipStream_t st) {
    g_last_variant = "attn_prefill";
    hipLaunchKernelGGL(prefill_attn_kernel, dim3(pa_q_tiles(G) * G.n_heads), dim3(PA_THREADS), 0, st, (const f16*)q, (const f16*)kc,
                       (const f16*)vc, (f16*)out, G);
    return hipGetLastError();
}

// Every global address the launch forms, on the CPU: the largest number of bytes by which one of them passes the end of its
// operand (q: t rows at q_stride, the last n_heads * 128 wide; K, V: [n_kv][kv_rows][128]; out: t rows at out_stride), or
// runs in front of it; 0 when none does.
long long prefill_attn_count_out_of_range(const PaGeom& G) {
    const long long kv_bytes = 2 * (long long)G.n_kv * G.kv_rows * PA_HD;
    long long worst = 0;
    auto touch = [&](long long b, int bytes, long long operand_bytes) {
        if (b < 0 && -b > worst) worst = -b;
        if (b + bytes - operand_bytes > worst) worst = b + bytes - operand_bytes;
    };
    const int blocks = pa_q_tiles(G) * G.n_heads;
    for (int block = 0; block < blocks; ++block) {
        const int qtile = pa_block_qtile(G, block), kvh = pa_kv_head(G, pa_block_head(G, block));
        pa_walk_q_out(G, block, touch);
        const int n_tiles = pa_key_tiles(G, qtile);
        for (int tile = 0; tile < n_tiles; ++tile)
            for (int c = 0; c < PA_CHUNKS; ++c)                    // K and V share the offset
                touch(2 * pa_kv_off(G, kvh, pa_key_row(G, tile, c >> 4), c & 15), 16, kv_bytes);
    }
    return worst;
}

}  // namespace qeft
