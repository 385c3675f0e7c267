// Causal prompt attention of a chunk over an e4m3 KV cache (qeft_attn_prefill_kv8).
//
// prefill_attn.hip with another K / V source: keys [0, start) are read from the FP8 cache where it lies (codes and fp32 row
// scales, include/qeft_hip.h), keys [start, start + t) from the chunk's own rotated fp16 K / V rows, views of the fused q|k|v
// output.  The source is chosen per key ROW (a 64-key tile can straddle start); cache rows >= start are never read, and at
// start == 0 no cache value is.  Decoding happens on the way into LDS: code -> fp32 (v_cvt_pk_f32_fp8), times the row scale in
// fp32, rounded ONCE to fp16, nearest even, subnormals kept -- llama.kv8_decode_rows' recipe, so the LDS images hold the bits
// qeft_attn_prefill would find in cat(kv8_decode_rows(past), chunk rows), and pa_attend (prefill_attn_body.h) behind them gives
// that launch's output bit for bit.  The scales are NOT folded into the scores or the exp weights (as the decode kernels do):
// that changes bits.
// A staged piece of a tile is, in the same registers, 8 fp16 of a new row or the codes of a cache row with its scale; which one
// follows from the key's position, at load and again at store.  No workspace, no atomics, no scratch.  Every global address
// comes from prefill_attn.h, clamped into its operand; prefill_attn_kv8_count_out_of_range walks the same functions on the CPU.
#include "prefill_attn_body.h"

namespace qeft {

typedef float pa_f2 __attribute__((ext_vector_type(2)));

// 8 codes and their row's scale -> 8 fp16.  The scale arrives as a scalar of its own, never as __builtin_bit_cast(float, v[2]) of a
// staged vector's element: hipcc takes element 0 there, which here multiplied by the codes.
__device__ __forceinline__ u32x4 pa8_decode(uint32_t c0, uint32_t c1, float s) {
    const pa_f2 sc = {s, s};
    const pa_f2 f0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)c0, false) * sc, f1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)c0, true) * sc;
    const pa_f2 f2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)c1, false) * sc, f3 = __builtin_amdgcn_cvt_pk_f32_fp8((int)c1, true) * sc;
    return u32x4{__builtin_bit_cast(uint32_t, __builtin_convertvector(f0, h2)), __builtin_bit_cast(uint32_t, __builtin_convertvector(f1, h2)),
                 __builtin_bit_cast(uint32_t, __builtin_convertvector(f2, h2)), __builtin_bit_cast(uint32_t, __builtin_convertvector(f3, h2))};
}

// Every thread issues the same four loads per piece, whatever the source -- 16 bytes for K, 16 for V and a dword next to each --
// with the source chosen per lane in the ADDRESS: a new row's piece and (unused) its first dword, or the aligned 16 codes that
// hold the piece's 8 and the row's scale.  So the loads of a tile carry no branch and nothing waits between their issue and
// the store after the next barrier, as in prefill_attn.hip; a lane whose key lies in the new rows forms no cache address.
struct PaStageKv8 {
    const uint8_t* __restrict__ kq;
    const uint8_t* __restrict__ vq;
    const float* __restrict__ ksc;
    const float* __restrict__ vsc;
    const f16* __restrict__ kn;
    const f16* __restrict__ vn;
    const Pa8Geom& G8;
    int kvh, tid, kv_len;
    u32x4 kst[PA_STAGE], vst[PA_STAGE];      // 8 fp16 of a new row, or 16 codes of a cache row
    uint32_t ksr[PA_STAGE], vsr[PA_STAGE];   // the cache row's scale (bits)

    __device__ __forceinline__ void load(int tile) {
        const PaGeom& G = G8.g;
#pragma unroll
        for (int i = 0; i < PA_STAGE; ++i) {
            const int c = tid + PA_THREADS * i, row = c >> 4, ch = c & 15, key = tile * PA_KT + row;
            const bool cached = pa8_from_cache(G, key);
            const int cr = pa8_cache_row(G, key);
            const long long noff = 2 * pa8_new_off(G8, pa8_new_row(G, key), kvh, ch);           // bytes, as the two below
            const long long coff = pa8_code_off(G, kvh, cr, pa8_code_pair(ch)), soff = 4 * pa8_scale_off(G, kvh, cr);
            const unsigned char* kp = cached ? kq + coff : (const unsigned char*)kn + noff;
            const unsigned char* vp = cached ? vq + coff : (const unsigned char*)vn + noff;
            const unsigned char* ksp = cached ? (const unsigned char*)ksc + soff : (const unsigned char*)kn + noff;
            const unsigned char* vsp = cached ? (const unsigned char*)vsc + soff : (const unsigned char*)vn + noff;
            kst[i] = *(const u32x4*)kp;
            vst[i] = *(const u32x4*)vp;
            ksr[i] = *(const uint32_t*)ksp;
            vsr[i] = *(const uint32_t*)vsp;
        }
    }
    __device__ __forceinline__ void store(int tile, unsigned char* lds_k, unsigned char* lds_v) {
#pragma unroll
        for (int i = 0; i < PA_STAGE; ++i) {
            const int c = tid + PA_THREADS * i, row = c >> 4, ch = c & 15, key = tile * PA_KT + row;
            u32x4 k = kst[i], v = vst[i];
            if (pa8_from_cache(G8.g, key)) {
                const bool hi = ch & 1;                            // the piece's 8 codes: the upper half of the 16
                k = pa8_decode(hi ? k[2] : k[0], hi ? k[3] : k[1], __builtin_bit_cast(float, ksr[i]));
                v = pa8_decode(hi ? v[2] : v[0], hi ? v[3] : v[1], __builtin_bit_cast(float, vsr[i]));
            } else if (key >= kv_len) {
                v = u32x4{0u, 0u, 0u, 0u};                          // V rows past the context: zeros (their K is masked)
            }
            *(u32x4*)(lds_k + pa_k_lds(row, ch)) = k;
            *(u32x4*)(lds_v + pa_v_lds(row, ch)) = v;
        }
    }
};

__global__ __launch_bounds__(PA_THREADS) void prefill_attn_kv8_kernel(const f16* __restrict__ q, const uint8_t* __restrict__ kq,
                                                                      const uint8_t* __restrict__ vq, const float* __restrict__ ksc,
                                                                      const float* __restrict__ vsc, const f16* __restrict__ kn,
                                                                      const f16* __restrict__ vn, f16* __restrict__ out, Pa8Geom G8) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_k[PA_KT * PA_HD * 2];
    __shared__ __attribute__((aligned(16))) unsigned char lds_v[PA_KT * PA_HD * 2];
    PaStageKv8 stage{kq, vq, ksc, vsc, kn, vn, G8, pa_kv_head(G8.g, pa_block_head(G8.g, blockIdx.x)), (int)threadIdx.x,
                     G8.g.start + G8.g.t};
    pa_attend(q, out, G8.g, stage, lds_k, lds_v, blockIdx.x);
}

hipError_t prefill_attn_kv8_launch(const void* q, const void* kq, const void* vq, const void* ksc, const void* vsc, const void* kn,
                                   const void* vn, void* out, const Pa8Geom& G8, hipStream_t st) {
    g_last_variant = "attn_prefill_kv8";
    hipLaunchKernelGGL(prefill_attn_kv8_kernel, dim3(pa_q_tiles(G8.g) * G8.g.n_heads), dim3(PA_THREADS), 0, st, (const f16*)q,
                       (const uint8_t*)kq, (const uint8_t*)vq, (const float*)ksc, (const float*)vsc, (const f16*)kn, (const f16*)vn,
                       (f16*)out, G8);
    return hipGetLastError();
}

// Every global address the launch forms, on the CPU: the largest number of bytes by which one passes the end of its operand or
// runs in front of it, 0 when none does.  q and out as prefill_attn_count_out_of_range; K and V codes uint8 [n_kv][kv_rows][128];
// K and V scales fp32 [n_kv][kv_rows]; new K and V rows: t rows at new_stride, the last n_kv * 128 wide.
long long prefill_attn_kv8_count_out_of_range(const Pa8Geom& G8) {
    const PaGeom& G = G8.g;
    const long long code_bytes = (long long)G.n_kv * G.kv_rows * PA_HD, scale_bytes = 4 * (long long)G.n_kv * G.kv_rows;
    const long long new_bytes = 2 * ((long long)(G.t - 1) * G8.new_stride + (long long)G.n_kv * PA_HD);
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
            for (int c = 0; c < PA_CHUNKS; ++c) {                  // thread c % 256, piece c / 256; K and V share the offsets
                const int key = tile * PA_KT + (c >> 4), ch = c & 15;
                if (pa8_from_cache(G, key)) {
                    const int cr = pa8_cache_row(G, key);
                    touch(pa8_code_off(G, kvh, cr, pa8_code_pair(ch)), 16, code_bytes);
                    touch(4 * pa8_scale_off(G, kvh, cr), 4, scale_bytes);
                } else {
                    const long long noff = 2 * pa8_new_off(G8, pa8_new_row(G, key), kvh, ch);
                    touch(noff, 16, new_bytes);
                    touch(noff, 4, new_bytes);                     // the dword loaded in the scale's place
                }
            }
    }
    return worst;
}

}  // namespace qeft
