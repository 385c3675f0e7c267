// The body of the causal prompt attention, shared by prefill_attn.hip (K / V from an fp16 cache) and
// prefill_attn_kv8.hip (the past from an e4m3 cache, the chunk's own rows in fp16).  The two differ in the staging step alone: a
// `Stage` loads one 64-key tile of K and V into its registers (load) and writes the fp16 images to LDS (store); everything
// behind the LDS images -- both MFMA products and their k order, the online softmax, the masking, the output epilogue -- is
// this one function, so two stages that put the same fp16 bits into LDS give the same output bits.
//   S^T = K Q^T   (swapped, so a lane holds 32 scores of ONE query row, the other 32 sit in lane + 32): K rows read by
//                 ds_read_b128 from an XOR-swizzled image; scores * 128^-0.5 in fp32; keys past start + i are SELECTED to
//                 -inf before the running max, so a NaN key a row must not see never reaches m.
//   online softmax in fp32, rescaled at every tile (no deferred-rescale threshold: no decision is shared between rows);
//                 p = exp(s - m) rounded to fp16 for the second product, l sums the fp32 p.
//   O^T = V^T P^T the score registers are the B operand as they are (k order permuted the same way on the V side); V^T
//                 fragments by ds_read_b64_tr_b16 from row-major V; fp32 accumulation.  V rows at positions >= start + t
//                 are staged as zeros by the stage (0 x NaN is NaN in the MFMA).
// A tile that is fully masked for a row gives alpha = exp(0) = 1, p = 0: m, l and O keep their bits, so a row's result
// depends on that row, its position and the keys alone -- whichever chunk, Q tile or wave carried it.  A wave skips the
// tiles wholly beyond its last row's diagonal; the block's tile loop ends at the diagonal of its last row.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "prefill_attn.h"
#include "qeft_common.h"

namespace qeft {

typedef short pa_s4 __attribute__((ext_vector_type(4)));

// LDS images of one tile, [64 keys][128] fp16 each, 256-byte rows; `ch` = 16-byte chunk of the row
__device__ __forceinline__ uint32_t pa_k_lds(int row, int ch) { return (uint32_t)(row * 256 + ((ch ^ (row & 15)) << 4)); }
// one XOR for the transposed reads (4 rows x 2 chunks per 16-lane group): conflict-free for the 32x32x16 operand
__device__ __forceinline__ uint32_t pa_v_lds(int row, int ch) {
    return (uint32_t)(row * 256 + ((ch ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4));
}

// One block = one (head, 128-row Q tile), 4 waves of 32 query rows with Q in registers (the B operand of
// v_mfma_f32_32x32x16_f16).  Tiles sit at absolute multiples of 64 from position 0, register-staged: stage.load(j + 1) is issued
// before tile j's products and stage.store() runs after the next barrier.
// LSE (the training forward, attn_train.hip): the row's log-sum-exp m + log(l) also goes to lse[row][head], fp32 [t][n_heads];
// `block` is the block's index within its sequence (blockIdx.x for the two cache kernels, which pass no lse).
template <bool LSE = false, class Stage>
__device__ __forceinline__ void pa_attend(const f16* __restrict__ q, f16* __restrict__ out, const PaGeom& G, Stage& stage,
                                          unsigned char* lds_k, unsigned char* lds_v, int block, float* __restrict__ lse = nullptr) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int qtile = pa_block_qtile(G, block), head = pa_block_head(G, block);
    const int n_tiles = pa_key_tiles(G, qtile);

    // Q fragments: k-step s takes d = 16 s + 8 h .. + 7 of this lane's row
    const int qrow = pa_q_row(G, qtile, wave, r);
    const int qpos = G.start + qrow;                               // the last key this row sees
    h8 qf[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) qf[s] = *(const h8*)(q + pa_q_off(G, qrow, head, 2 * s + h));
    const int wave_row0 = qtile * PA_QT + wave * 32;
    const bool wave_on = wave_row0 < G.t;                          // wave-uniform
    const int wave_last_pos = G.start + pa_q_row(G, qtile, wave, 31);

    f32x16 o[4];
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[db][e] = 0.f;
    float m = -INFINITY, l = 0.f;
    const float scale = 0.08838834764831845f;                      // 128^-0.5

    // transposed V reads: lane 4 qq + p of a 16-lane group addresses row qq, columns 4 p .. 4 p + 3 of the group's 4 x 16 block
    const int tqq = (lane & 15) >> 2, tp = lane & 3, tcol = (lane >> 4) & 1;

    stage.load(0);
    for (int tile = 0; tile < n_tiles; ++tile) {
        __syncthreads();                                           // every wave is done with the previous tile's images
        stage.store(tile, lds_k, lds_v);
        __syncthreads();
        if (tile + 1 < n_tiles) stage.load(tile + 1);
        if (!wave_on || tile * PA_KT > wave_last_pos) continue;    // wholly beyond this wave's diagonal (wave-uniform)

        f32x16 st[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int e = 0; e < 16; ++e) st[kb][e] = 0.f;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const h8 kf = *(const h8*)(lds_k + pa_k_lds(kb * 32 + r, 2 * s + h));
                st[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s], st[kb], 0, 0, 0);
            }
        }
        // st[kb][e]: key tile * 64 + kb * 32 + pa_acc_row(e, h) against this lane's query row
        float mloc = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int kpos = tile * PA_KT + kb * 32 + pa_acc_row(e, h);
                const float sc = kpos <= qpos ? st[kb][e] * scale : -INFINITY;
                st[kb][e] = sc;
                mloc = fmaxf(mloc, sc);
            }
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32));
        const float m_new = fmaxf(m, mloc);                        // finite from tile 0 on: every row sees key 0
        const float alpha = __expf(m - m_new);
        m = m_new;
        float lsum = 0.f;
        h8 pf[2][2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float p = __expf(st[kb][e] - m_new);
                lsum += p;
                pf[kb][e >> 3][e & 7] = (f16)p;
            }
        lsum += __shfl_xor(lsum, 32);
        l = l * alpha + lsum;
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int e = 0; e < 16; ++e) o[db][e] *= alpha;
        // element j of pf[kb][s2] is key kb * 32 + 16 s2 + 8 (j >> 2) + 4 h + (j & 3): the V^T fragment takes the same keys
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int db = 0; db < 4; ++db) {
                    pa_s4 part[2];
#pragma unroll
                    for (int half = 0; half < 2; ++half) {
                        const int row = kb * 32 + 16 * s2 + 8 * half + 4 * h + tqq;
                        const uint32_t a = pa_v_lds(row, 4 * db + 2 * tcol + (tp >> 1)) + 8 * (tp & 1);
                        part[half] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) pa_s4*)(lds_v + a));
                    }
                    const u32x2 lo = __builtin_bit_cast(u32x2, part[0]), hi = __builtin_bit_cast(u32x2, part[1]);
                    const h8 vf = __builtin_bit_cast(h8, u32x4{lo[0], lo[1], hi[0], hi[1]});
                    o[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[kb][s2], o[db], 0, 0, 0);
                }
    }

    // o[db][e] = O[this lane's query row][32 db + pa_acc_row(e, h)]: four consecutive d per register group
    const int row = wave_row0 + r;
    if (wave_on && row < G.t) {
        const float inv = 1.f / l;
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                h4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (f16)(o[db][4 * g + j] * inv);
                *(h4*)(out + pa_out_off(G, row, head, 32 * db + pa_acc_row(4 * g, h))) = v;
            }
        if constexpr (LSE) {
            if (h == 0) lse[pa_lse_off(G, row, head)] = m + logf(l);   // both lane halves hold the row's m and l
        }
    }
}

// The enumeration of the operands both kernels share: every q load and out store of block `block`, through `touch(byte offset,
// bytes, operand bytes)`.
template <class Touch>
inline void pa_walk_q_out(const PaGeom& G, int block, Touch&& touch) {
    const long long q_bytes = 2 * ((long long)(G.t - 1) * G.q_stride + (long long)G.n_heads * PA_HD);
    const long long out_bytes = 2 * ((long long)(G.t - 1) * G.out_stride + (long long)G.n_heads * PA_HD);
    const int qtile = pa_block_qtile(G, block), head = pa_block_head(G, block);
    for (int wave = 0; wave < PA_WAVES; ++wave)
        for (int lane = 0; lane < 64; ++lane) {
            const int r = lane & 31, h = lane >> 5;
            for (int s = 0; s < 8; ++s) touch(2 * pa_q_off(G, pa_q_row(G, qtile, wave, r), head, 2 * s + h), 16, q_bytes);
            const int row = qtile * PA_QT + wave * 32 + r;
            if (row < G.t)
                for (int db = 0; db < 4; ++db)
                    for (int g = 0; g < 4; ++g) touch(2 * pa_out_off(G, row, head, 32 * db + pa_acc_row(4 * g, h)), 8, out_bytes);
        }
}

}  // namespace qeft
