// Causal attention for the training step (qeft_attn_train_fwd, qeft_attn_train_bwd).
//
// n_seq sequences of t rotated fp16 rows each, every one from position 0 and attending itself alone; q, k, v as the projections
// leave them, row-major [n_seq t][heads 128] at a row stride (views of one fused q|k|v buffer are fine), grouped-query layouts
// read in place.
//   forward   pa_attend (prefill_attn_body.h) behind a third staging step -- K and V tiles from the row-major operands -- with
//             the row's log-sum-exp stored next to the output: the output bits of qeft_attn_prefill at start = 0.
//   backward  three launches, no float atomics, nothing that waits on another workgroup:
//     delta   delta[row][head] = sum_d dout out, fp32, 16 lanes per (row, head).
//     dK / dV one block = 128 keys of one (sequence, kv head), a wave = 32 of them with K and V in registers as MFMA B
//             operands and dK^T, dV^T (fp32, 128 registers) on chip for the whole launch; it sweeps the group's query heads in
//             ascending order and, per head, the 64-row query tiles from its diagonal to the end: the grouped-query sum happens
//             in registers in that one order.  The key sits on the MFMA lane, so S and dP accumulators are the B operands of
//             the two products behind them; Q and dO tiles have ONE LDS image each, read by rows (S, dP) and through
//             ds_read_b64_tr_b16 (dV^T += dO^T P, dK^T += Q^T dS).
//     dQ      one block per (sequence, head, 128-row Q tile), the forward's shape with Q and dO in registers; per key tile it
//             recomputes S, p, dP, dS exactly as the dK / dV launch (at_p_ds) and accumulates dQ^T += K^T dS from the transposed
//             reads of the K image.  7 MFMA products per tile pair over both launches instead of 5.
//   p = exp(s 128^-0.5 - lse) in fp32 (no running max); P rounded to fp16 for dV; dS = p (dP - delta) in fp32, rounded once to
//   fp16; the 128^-0.5 of dK and dQ applied in fp32 in the epilogue.  Masked (key, row) pairs are SELECTED to p = dS = 0; rows
//   past t are staged as zeros where a transposed product reads them, computed where a lane owns them, never stored.
// Every global address comes from attn_train.h / prefill_attn.h, clamped into its sequence; the *_count_out_of_range below
// walk the same functions on the CPU.
//
// Packed sequences of unequal length (qeft_attn_train_varlen_fwd / _bwd): the three bodies are device
// functions of one block of one sequence (at_fwd_block, at_dkv_block, at_dq_block), each called by two kernels.  The
// fixed-length kernel finds its sequence in blockIdx.x; the variable-length kernel takes it from blockIdx.y, reads its first row
// and length out of the prefix in its own arguments (AtVarGeom, by value: no table on the device), builds that sequence's AtGeom,
// puts at_var_base on every pointer and runs the body at seq = 0 -- so a sequence's bits are those of the fixed-length launch on
// it alone.  A block past its sequence's count returns before it forms an address.  delta is row-wise and runs as it is.
#include "attn_train.h"
#include "prefill_attn_body.h"

namespace qeft {

// ---------------------------------------------------------------- forward
// K and V tiles from the row-major training operands: prefill_attn_kv8.hip's new-row access without the cache half
struct PaStageTrain {
    const f16* __restrict__ kn;
    const f16* __restrict__ vn;
    const Pa8Geom& G8;
    int kvh, tid;
    u32x4 kst[PA_STAGE], vst[PA_STAGE];

    __device__ __forceinline__ void load(int tile) {
#pragma unroll
        for (int i = 0; i < PA_STAGE; ++i) {
            const int c = tid + PA_THREADS * i, row = c >> 4, ch = c & 15, key = tile * PA_KT + row;
            const long long off = pa8_new_off(G8, pa8_new_row(G8.g, key), kvh, ch);
            kst[i] = *(const u32x4*)(kn + off);
            const u32x4 v = *(const u32x4*)(vn + off);
            vst[i] = key < G8.g.t ? v : u32x4{0u, 0u, 0u, 0u};
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

// block `block` of ONE sequence of A.f.g.t rows, every operand at the sequence's first row: what both forward kernels run
__device__ __forceinline__ void at_fwd_block(const f16* q, const f16* k, const f16* v, f16* out, float* lse, const AtGeom& A, int block,
                                             unsigned char* lds_k, unsigned char* lds_v) {
    const PaGeom& G = A.f.g;
    PaStageTrain stage{k, v, A.f, pa_kv_head(G, pa_block_head(G, block)), (int)threadIdx.x};
    pa_attend<true>(q, out, G, stage, lds_k, lds_v, block, lse);
}

__global__ __launch_bounds__(PA_THREADS) void attn_train_fwd_kernel(const f16* __restrict__ q, const f16* __restrict__ k,
                                                                    const f16* __restrict__ v, f16* __restrict__ out,
                                                                    float* __restrict__ lse, AtGeom A) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_k[PA_KT * PA_HD * 2];
    __shared__ __attribute__((aligned(16))) unsigned char lds_v[PA_KT * PA_HD * 2];
    const PaGeom& G = A.f.g;
    const int per_seq = at_q_blocks_per_seq(A), seq = blockIdx.x / per_seq, block = blockIdx.x % per_seq;
    q += at_seq_base(A, seq, G.q_stride);
    k += at_seq_base(A, seq, A.f.new_stride);
    v += at_seq_base(A, seq, A.f.new_stride);
    out += at_seq_base(A, seq, G.out_stride);
    lse += at_seq_base(A, seq, G.n_heads);
    at_fwd_block(q, k, v, out, lse, A, block, lds_k, lds_v);
}

// the variable-length forward: grid (blocks of the longest sequence, n_seq).  The block's sequence becomes a geometry of its own
// and a base on every pointer; a block past its sequence's count leaves before it forms an address.
__global__ __launch_bounds__(PA_THREADS) void attn_train_varlen_fwd_kernel(const f16* __restrict__ q, const f16* __restrict__ k,
                                                                           const f16* __restrict__ v, f16* __restrict__ out,
                                                                           float* __restrict__ lse, AtVarGeom V) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_k[PA_KT * PA_HD * 2];
    __shared__ __attribute__((aligned(16))) unsigned char lds_v[PA_KT * PA_HD * 2];
    const int seq = blockIdx.y, block = blockIdx.x;
    const AtGeom A = at_var_seq(V, seq);
    if (block >= at_q_blocks_per_seq(A)) return;
    const PaGeom& G = A.f.g;
    q += at_var_base(V, seq, G.q_stride);
    k += at_var_base(V, seq, A.f.new_stride);
    v += at_var_base(V, seq, A.f.new_stride);
    out += at_var_base(V, seq, G.out_stride);
    lse += at_var_base(V, seq, G.n_heads);
    at_fwd_block(q, k, v, out, lse, A, block, lds_k, lds_v);
}

hipError_t attn_train_fwd_launch(const void* q, const void* k, const void* v, void* out, float* lse, const AtGeom& A, hipStream_t st) {
    g_last_variant = "attn_train_fwd";
    hipLaunchKernelGGL(attn_train_fwd_kernel, dim3((unsigned)at_q_blocks(A)), dim3(PA_THREADS), 0, st, (const f16*)q, (const f16*)k,
                       (const f16*)v, (f16*)out, lse, A);
    return hipGetLastError();
}

hipError_t attn_train_varlen_fwd_launch(const void* q, const void* k, const void* v, void* out, float* lse, const AtVarGeom& V,
                                        hipStream_t st) {
    g_last_variant = "attn_train_varlen_fwd";
    hipLaunchKernelGGL(attn_train_varlen_fwd_kernel, dim3((unsigned)at_var_q_grid_x(V), (unsigned)V.a.n_seq), dim3(PA_THREADS), 0, st,
                       (const f16*)q, (const f16*)k, (const f16*)v, (f16*)out, lse, V);
    return hipGetLastError();
}

// ---------------------------------------------------------------- backward: shared pieces
// p and dS of one (query row, key) pair from its fp32 score and dP accumulators; the one place both launches compute them, so
// dS is the same fp16 value in both
__device__ __forceinline__ void at_p_ds(float s, float dp, float lse, float delta, bool seen, float& p, float& ds) {
    const float pe = __expf(s * 0.08838834764831845f - lse);        // 128^-0.5
    p = seen ? pe : 0.f;
    ds = seen ? pe * (dp - delta) : 0.f;
}

// A operand (32 x 16, transposed) of v_mfma_f32_32x32x16_f16 out of a row-major [64][128] image in pa_v_lds order: rows
// row0 + {4 h + tqq, 8 + 4 h + tqq}, the k order of an accumulator pair used as the B operand (prefill_attn_body.h)
__device__ __forceinline__ h8 at_tr_frag(const unsigned char* img, int row0, int db, int h, int tqq, int tp, int tcol) {
    pa_s4 part[2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int row = row0 + 8 * half + 4 * h + tqq;
        const uint32_t a = pa_v_lds(row, 4 * db + 2 * tcol + (tp >> 1)) + 8 * (tp & 1);
        part[half] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) pa_s4*)(img + a));
    }
    const u32x2 lo = __builtin_bit_cast(u32x2, part[0]), hi = __builtin_bit_cast(u32x2, part[1]);
    return __builtin_bit_cast(h8, u32x4{lo[0], lo[1], hi[0], hi[1]});
}

// ---------------------------------------------------------------- delta
__global__ __launch_bounds__(AT_THREADS) void attn_train_delta_kernel(const f16* __restrict__ out, const f16* __restrict__ dout,
                                                                      float* __restrict__ delta, AtGeom A) {
    const int slot = threadIdx.x >> 4, ch = threadIdx.x & 15, nh = A.f.g.n_heads;
    const long long pair = at_delta_pair(A, blockIdx.x, slot);
    const long long grow = pair / nh;                                // global row: sequence * t + row
    const int head = (int)(pair % nh), seq = (int)(grow / A.f.g.t), row = (int)(grow % A.f.g.t);
    const h8 o = *(const h8*)(out + at_out_off(A, seq, row, head, ch));
    const h8 d = *(const h8*)(dout + at_dout_off(A, seq, row, head, ch));
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s = fmaf((float)d[j], (float)o[j], s);
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 8);
    if (ch == 0 && (long long)blockIdx.x * AT_DELTA_PAIRS + slot < at_delta_pairs(A)) delta[at_lse_off(A, seq, row, head)] = s;
}

// ---------------------------------------------------------------- dK / dV
// VGPR / AGPR budget of a wave (one wave per SIMD, 512 registers): K and V fragments 32 + 32, dK^T and dV^T accumulators
// 64 + 64, S and dP of one 64-row tile 32 + 32, P and dS in fp16 16 + 16, the next tile's staging 33.  LDS: 16 KiB per image,
// two images, 512 bytes of lse | delta.
// The body: key block `kblock` of kv head `kvh` of sequence `seq` of A (the variable-length kernel: of its one sequence, seq = 0,
// behind the bases it put on the pointers).  lds_ld: lse of the tile's rows, then delta.
__device__ __forceinline__ void at_dkv_block(const f16* q, const f16* k, const f16* v, const f16* dout, const float* lse,
                                             const float* delta, f16* dk, f16* dv, const AtGeom& A, int seq, int kblock, int kvh,
                                             unsigned char* lds_q, unsigned char* lds_do, float* lds_ld) {
    const PaGeom& G = A.f.g;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int rep = G.n_heads / G.n_kv;
    const int wave_key0 = kblock * AT_KB + wave * 32, key = wave_key0 + r, krow = at_row(A, key);
    const bool wave_on = wave_key0 < G.t;                            // wave-uniform

    // K and V fragments, the B operands of S and dP: k-step s takes d = 16 s + 8 h .. + 7 of this lane's key
    h8 kf[8], vf[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        kf[s] = *(const h8*)(k + at_kv_off(A, seq, krow, kvh, 2 * s + h));
        vf[s] = *(const h8*)(v + at_kv_off(A, seq, krow, kvh, 2 * s + h));
    }
    f32x16 dka[4], dva[4];
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) dka[db][e] = dva[db][e] = 0.f;

    const int tile0 = at_dkv_first_tile(kblock), n_tiles = at_dkv_end_tile(A) - tile0, steps = rep * n_tiles;
    const int tqq = (lane & 15) >> 2, tp = lane & 3, tcol = (lane >> 4) & 1;
    const float* __restrict__ ldsrc = (wave & 1) ? delta : lse;      // waves 0 / 2 stage lse, 1 / 3 delta (the same values twice)

    u32x4 qst[PA_STAGE], dst[PA_STAGE];
    float ldst;
    auto load = [&](int step) {
        const int head = kvh * rep + step / n_tiles, tile = tile0 + step % n_tiles;
#pragma unroll
        for (int i = 0; i < PA_STAGE; ++i) {
            const int c = tid + AT_THREADS * i, row = tile * AT_QT + (c >> 4), ch = c & 15, rr = at_row(A, row);
            const u32x4 a = *(const u32x4*)(q + at_q_off(A, seq, rr, head, ch));
            const u32x4 b = *(const u32x4*)(dout + at_dout_off(A, seq, rr, head, ch));
            qst[i] = row < G.t ? a : u32x4{0u, 0u, 0u, 0u};         // rows past the sequence: zeros, not 0 x NaN
            dst[i] = row < G.t ? b : u32x4{0u, 0u, 0u, 0u};
        }
        ldst = ldsrc[at_lse_off(A, seq, at_row(A, tile * AT_QT + lane), head)];
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < PA_STAGE; ++i) {
            const int c = tid + AT_THREADS * i, row = c >> 4, ch = c & 15;
            *(u32x4*)(lds_q + pa_v_lds(row, ch)) = qst[i];
            *(u32x4*)(lds_do + pa_v_lds(row, ch)) = dst[i];
        }
        lds_ld[(wave & 1) * AT_QT + lane] = ldst;
    };

    load(0);
    for (int step = 0; step < steps; ++step) {
        __syncthreads();                                           // every wave is done with the previous tile's images
        store();
        __syncthreads();
        if (step + 1 < steps) load(step + 1);
        const int tile = tile0 + step % n_tiles;
        if (!wave_on || wave_key0 > tile * AT_QT + AT_QT - 1) continue;       // every key of the wave past the tile (wave-uniform)

        // S = Q K^T and dP = dO V^T with the key on the lane: acc[qb][e] is query row tile * 64 + qb * 32 + pa_acc_row(e, h)
        f32x16 sa[2], dpa[2];
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
#pragma unroll
            for (int e = 0; e < 16; ++e) sa[qb][e] = dpa[qb][e] = 0.f;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const h8 qa = *(const h8*)(lds_q + pa_v_lds(qb * 32 + r, 2 * s + h));
                sa[qb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(qa, kf[s], sa[qb], 0, 0, 0);
                const h8 da = *(const h8*)(lds_do + pa_v_lds(qb * 32 + r, 2 * s + h));
                dpa[qb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(da, vf[s], dpa[qb], 0, 0, 0);
            }
        }
        h8 pf[2][2], dsf[2][2];
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 l4 = *(const f32x4*)(lds_ld + qb * 32 + 8 * g + 4 * h);
                const f32x4 d4 = *(const f32x4*)(lds_ld + AT_QT + qb * 32 + 8 * g + 4 * h);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int e = 4 * g + j, qpos = tile * AT_QT + qb * 32 + pa_acc_row(e, h);
                    float p, ds;
                    at_p_ds(sa[qb][e], dpa[qb][e], l4[j], d4[j], key <= qpos && qpos < G.t, p, ds);
                    pf[qb][e >> 3][e & 7] = (f16)p;
                    dsf[qb][e >> 3][e & 7] = (f16)ds;
                }
            }
        // dV^T += dO^T P, dK^T += Q^T dS: the fp16 accumulator pairs are the B operands, rows of the images the k dimension
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int db = 0; db < 4; ++db) {
                    const h8 dot = at_tr_frag(lds_do, qb * 32 + 16 * s2, db, h, tqq, tp, tcol);
                    dva[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(dot, pf[qb][s2], dva[db], 0, 0, 0);
                    const h8 qt = at_tr_frag(lds_q, qb * 32 + 16 * s2, db, h, tqq, tp, tcol);
                    dka[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(qt, dsf[qb][s2], dka[db], 0, 0, 0);
                }
    }

    // acc[db][e] = dK^T / dV^T [32 db + pa_acc_row(e, h)][this lane's key]: four consecutive d per register group
    if (wave_on && key < G.t) {
        const float scale = 0.08838834764831845f;
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                h4 a, b;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    a[j] = (f16)(dka[db][4 * g + j] * scale);
                    b[j] = (f16)dva[db][4 * g + j];
                }
                const long long off = at_dkv_off(A, seq, key, kvh, 32 * db + pa_acc_row(4 * g, h));
                *(h4*)(dk + off) = a;
                *(h4*)(dv + off) = b;
            }
    }
}

__global__ __launch_bounds__(AT_THREADS) void attn_train_dkv_kernel(const f16* __restrict__ q, const f16* __restrict__ k,
                                                                    const f16* __restrict__ v, const f16* __restrict__ dout,
                                                                    const float* __restrict__ lse, const float* __restrict__ delta,
                                                                    f16* __restrict__ dk, f16* __restrict__ dv, AtGeom A) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_q[AT_QT * PA_HD * 2];
    __shared__ __attribute__((aligned(16))) unsigned char lds_do[AT_QT * PA_HD * 2];
    __shared__ __attribute__((aligned(16))) float lds_ld[2 * AT_QT];
    at_dkv_block(q, k, v, dout, lse, delta, dk, dv, A, at_dkv_seq(A, blockIdx.x), at_dkv_kblock(A, blockIdx.x),
                 at_dkv_kvh(A, blockIdx.x), lds_q, lds_do, lds_ld);
}

// variable-length: grid (key blocks x kv heads of the longest sequence, n_seq); see attn_train_varlen_fwd_kernel
__global__ __launch_bounds__(AT_THREADS) void attn_train_varlen_dkv_kernel(const f16* __restrict__ q, const f16* __restrict__ k,
                                                                           const f16* __restrict__ v, const f16* __restrict__ dout,
                                                                           const float* __restrict__ lse,
                                                                           const float* __restrict__ delta, f16* __restrict__ dk,
                                                                           f16* __restrict__ dv, AtVarGeom V) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_q[AT_QT * PA_HD * 2];
    __shared__ __attribute__((aligned(16))) unsigned char lds_do[AT_QT * PA_HD * 2];
    __shared__ __attribute__((aligned(16))) float lds_ld[2 * AT_QT];
    const int seq = blockIdx.y, block = blockIdx.x;
    const AtGeom A = at_var_seq(V, seq);
    if (block >= at_dkv_blocks_per_seq(A)) return;
    const PaGeom& G = A.f.g;
    q += at_var_base(V, seq, G.q_stride);
    k += at_var_base(V, seq, A.f.new_stride);
    v += at_var_base(V, seq, A.f.new_stride);
    dout += at_var_base(V, seq, A.dout_stride);
    lse += at_var_base(V, seq, G.n_heads);
    delta += at_var_base(V, seq, G.n_heads);
    dk += at_var_base(V, seq, A.dkv_stride);
    dv += at_var_base(V, seq, A.dkv_stride);
    at_dkv_block(q, k, v, dout, lse, delta, dk, dv, A, 0, at_dkv_kblock(A, block), at_dkv_kvh(A, block), lds_q, lds_do, lds_ld);
}

// ---------------------------------------------------------------- dQ
// Registers of a wave: Q and dO fragments 32 + 32, dQ^T accumulators 64, S^T and dP^T of one 64-key tile 32 + 32, dS in fp16 16,
// the next tile's staging 32.  LDS: a K and a V image of 16 KiB.
// The body: block `block` (head, Q tile) of sequence `seq` of A (the variable-length kernel: of its one sequence, seq = 0).
__device__ __forceinline__ void at_dq_block(const f16* q, const f16* k, const f16* v, const f16* dout, const float* lse,
                                            const float* delta, f16* dq, const AtGeom& A, int seq, int block, unsigned char* lds_k,
                                            unsigned char* lds_v) {
    const PaGeom& G = A.f.g;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int qtile = pa_block_qtile(G, block), head = pa_block_head(G, block), kvh = pa_kv_head(G, head);
    const int n_tiles = pa_key_tiles(G, qtile);

    const int qpos = pa_q_row(G, qtile, wave, r);                  // this lane's row = the last key it sees
    h8 qf[8], dof[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        qf[s] = *(const h8*)(q + at_q_off(A, seq, qpos, head, 2 * s + h));
        dof[s] = *(const h8*)(dout + at_dout_off(A, seq, qpos, head, 2 * s + h));
    }
    const float lse_q = lse[at_lse_off(A, seq, qpos, head)], delta_q = delta[at_lse_off(A, seq, qpos, head)];
    const int wave_row0 = qtile * PA_QT + wave * 32;
    const bool wave_on = wave_row0 < G.t;                          // wave-uniform
    const int wave_last_pos = pa_q_row(G, qtile, wave, 31);

    f32x16 dqa[4];
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) dqa[db][e] = 0.f;
    const int tqq = (lane & 15) >> 2, tp = lane & 3, tcol = (lane >> 4) & 1;

    u32x4 kst[PA_STAGE], vst[PA_STAGE];
    auto load = [&](int tile) {
#pragma unroll
        for (int i = 0; i < PA_STAGE; ++i) {
            const int c = tid + AT_THREADS * i, key = tile * PA_KT + (c >> 4), ch = c & 15;
            const long long off = at_kv_off(A, seq, at_row(A, key), kvh, ch);
            const u32x4 a = *(const u32x4*)(k + off);
            kst[i] = key < G.t ? a : u32x4{0u, 0u, 0u, 0u};         // K rows past the sequence: zeros under the transposed reads
            vst[i] = *(const u32x4*)(v + off);
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < PA_STAGE; ++i) {
            const int c = tid + AT_THREADS * i, row = c >> 4, ch = c & 15;
            *(u32x4*)(lds_k + pa_v_lds(row, ch)) = kst[i];
            *(u32x4*)(lds_v + pa_v_lds(row, ch)) = vst[i];
        }
    };

    load(0);
    for (int tile = 0; tile < n_tiles; ++tile) {
        __syncthreads();
        store();
        __syncthreads();
        if (tile + 1 < n_tiles) load(tile + 1);
        if (!wave_on || tile * PA_KT > wave_last_pos) continue;    // wholly beyond this wave's diagonal (wave-uniform)

        // S^T = K Q^T and dP^T = V dO^T: acc[kb][e] is key tile * 64 + kb * 32 + pa_acc_row(e, h) against this lane's row
        f32x16 sa[2], dpa[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int e = 0; e < 16; ++e) sa[kb][e] = dpa[kb][e] = 0.f;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const h8 ka = *(const h8*)(lds_k + pa_v_lds(kb * 32 + r, 2 * s + h));
                sa[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ka, qf[s], sa[kb], 0, 0, 0);
                const h8 va = *(const h8*)(lds_v + pa_v_lds(kb * 32 + r, 2 * s + h));
                dpa[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(va, dof[s], dpa[kb], 0, 0, 0);
            }
        }
        h8 dsf[2][2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int kpos = tile * PA_KT + kb * 32 + pa_acc_row(e, h);
                float p, ds;
                at_p_ds(sa[kb][e], dpa[kb][e], lse_q, delta_q, kpos <= qpos, p, ds);
                dsf[kb][e >> 3][e & 7] = (f16)ds;
            }
        // dQ^T += K^T dS^T
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int db = 0; db < 4; ++db) {
                    const h8 kt = at_tr_frag(lds_k, kb * 32 + 16 * s2, db, h, tqq, tp, tcol);
                    dqa[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kt, dsf[kb][s2], dqa[db], 0, 0, 0);
                }
    }

    const int row = wave_row0 + r;
    if (wave_on && row < G.t) {
        const float scale = 0.08838834764831845f;
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                h4 a;
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] = (f16)(dqa[db][4 * g + j] * scale);
                *(h4*)(dq + at_dq_off(A, seq, row, head, 32 * db + pa_acc_row(4 * g, h))) = a;
            }
    }
}

__global__ __launch_bounds__(AT_THREADS) void attn_train_dq_kernel(const f16* __restrict__ q, const f16* __restrict__ k,
                                                                   const f16* __restrict__ v, const f16* __restrict__ dout,
                                                                   const float* __restrict__ lse, const float* __restrict__ delta,
                                                                   f16* __restrict__ dq, AtGeom A) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_k[PA_KT * PA_HD * 2];
    __shared__ __attribute__((aligned(16))) unsigned char lds_v[PA_KT * PA_HD * 2];
    const int per_seq = at_q_blocks_per_seq(A);
    at_dq_block(q, k, v, dout, lse, delta, dq, A, blockIdx.x / per_seq, blockIdx.x % per_seq, lds_k, lds_v);
}

// variable-length: grid (heads x Q tiles of the longest sequence, n_seq); see attn_train_varlen_fwd_kernel
__global__ __launch_bounds__(AT_THREADS) void attn_train_varlen_dq_kernel(const f16* __restrict__ q, const f16* __restrict__ k,
                                                                          const f16* __restrict__ v, const f16* __restrict__ dout,
                                                                          const float* __restrict__ lse,
                                                                          const float* __restrict__ delta, f16* __restrict__ dq,
                                                                          AtVarGeom V) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_k[PA_KT * PA_HD * 2];
    __shared__ __attribute__((aligned(16))) unsigned char lds_v[PA_KT * PA_HD * 2];
    const int seq = blockIdx.y, block = blockIdx.x;
    const AtGeom A = at_var_seq(V, seq);
    if (block >= at_q_blocks_per_seq(A)) return;
    const PaGeom& G = A.f.g;
    q += at_var_base(V, seq, G.q_stride);
    k += at_var_base(V, seq, A.f.new_stride);
    v += at_var_base(V, seq, A.f.new_stride);
    dout += at_var_base(V, seq, A.dout_stride);
    lse += at_var_base(V, seq, G.n_heads);
    delta += at_var_base(V, seq, G.n_heads);
    dq += at_var_base(V, seq, A.dq_stride);
    at_dq_block(q, k, v, dout, lse, delta, dq, A, 0, block, lds_k, lds_v);
}

// parts: bit 0 the delta launch, bit 1 dK / dV, bit 2 dQ, in this order (qeft_attn_train_bwd: all three; qeft_attn_train_bwd_part:
// one alone, for the timing tool and the variant tests)
hipError_t attn_train_bwd_launch(const void* q, const void* k, const void* v, const void* out, const void* dout, const float* lse,
                                 void* dq, void* dk, void* dv, float* delta, const AtGeom& A, int parts, hipStream_t st) {
    if (parts & 1) {
        g_last_variant = "attn_train_delta";
        hipLaunchKernelGGL(attn_train_delta_kernel, dim3((unsigned)at_delta_blocks(A)), dim3(AT_THREADS), 0, st, (const f16*)out,
                           (const f16*)dout, delta, A);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (parts & 2) {
        g_last_variant = "attn_train_dkv";
        hipLaunchKernelGGL(attn_train_dkv_kernel, dim3((unsigned)at_dkv_blocks(A)), dim3(AT_THREADS), 0, st, (const f16*)q,
                           (const f16*)k, (const f16*)v, (const f16*)dout, lse, (const float*)delta, (f16*)dk, (f16*)dv, A);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (parts & 4) {
        g_last_variant = "attn_train_dq";
        hipLaunchKernelGGL(attn_train_dq_kernel, dim3((unsigned)at_q_blocks(A)), dim3(AT_THREADS), 0, st, (const f16*)q, (const f16*)k,
                           (const f16*)v, (const f16*)dout, lse, (const float*)delta, (f16*)dq, A);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

// the same three launches over a prefix of sequence lengths; delta is row-wise over global rows and runs as it is, with all R
// rows as one sequence
hipError_t attn_train_varlen_bwd_launch(const void* q, const void* k, const void* v, const void* out, const void* dout,
                                        const float* lse, void* dq, void* dk, void* dv, float* delta, const AtVarGeom& V, int parts,
                                        hipStream_t st) {
    const dim3 seqs_q((unsigned)at_var_q_grid_x(V), (unsigned)V.a.n_seq), seqs_k((unsigned)at_var_dkv_grid_x(V), (unsigned)V.a.n_seq);
    if (parts & 1) {
        const AtGeom D = at_var_all(V);
        g_last_variant = "attn_train_delta";
        hipLaunchKernelGGL(attn_train_delta_kernel, dim3((unsigned)at_delta_blocks(D)), dim3(AT_THREADS), 0, st, (const f16*)out,
                           (const f16*)dout, delta, D);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (parts & 2) {
        g_last_variant = "attn_train_varlen_dkv";
        hipLaunchKernelGGL(attn_train_varlen_dkv_kernel, seqs_k, dim3(AT_THREADS), 0, st, (const f16*)q, (const f16*)k, (const f16*)v,
                           (const f16*)dout, lse, (const float*)delta, (f16*)dk, (f16*)dv, V);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (parts & 4) {
        g_last_variant = "attn_train_varlen_dq";
        hipLaunchKernelGGL(attn_train_varlen_dq_kernel, seqs_q, dim3(AT_THREADS), 0, st, (const f16*)q, (const f16*)k, (const f16*)v,
                           (const f16*)dout, lse, (const float*)delta, (f16*)dq, V);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

// ---------------------------------------------------------------- the address enumerations (CPU)
// One walker per launch and sequence, shared by the fixed-length enumerations (sequence `seq` of A, no further base) and the
// variable-length ones (A = at_var_seq, seq = 0, behind the at_var_base of every operand): the functions the kernels call, in
// the kernels' order of composition.
namespace {
struct AtWorst {
    long long worst = 0;
    void operator()(long long b, long long bytes, long long operand_bytes) {
        if (b < 0 && -b > worst) worst = -b;
        if (b + bytes - operand_bytes > worst) worst = b + bytes - operand_bytes;
    }
};
// bytes of an operand of `rows` rows at `stride`, the last one `width` elements wide
inline long long at_bytes(long long rows, int stride, int width) { return 2 * ((rows - 1) * stride + width); }
struct AtSizes {                             // bytes of every operand of a launch over `rows` rows
    long long q, out, dout, dq, kv, dkv, lse;
    AtSizes(const AtGeom& A, long long rows) {
        const PaGeom& G = A.f.g;
        const int hw = G.n_heads * PA_HD, kw = G.n_kv * PA_HD;
        q = at_bytes(rows, G.q_stride, hw), out = at_bytes(rows, G.out_stride, hw), dout = at_bytes(rows, A.dout_stride, hw);
        dq = at_bytes(rows, A.dq_stride, hw), kv = at_bytes(rows, A.f.new_stride, kw), dkv = at_bytes(rows, A.dkv_stride, kw);
        lse = 4ll * rows * G.n_heads;
    }
};
struct AtBase {                              // element offsets a kernel put on its pointers before the body: at_var_base, or none
    long long q = 0, out = 0, dout = 0, dq = 0, kv = 0, dkv = 0, lse = 0;
    AtBase() {}
    AtBase(const AtVarGeom& V, int seq) {
        const PaGeom& G = V.a.f.g;
        q = at_var_base(V, seq, G.q_stride), out = at_var_base(V, seq, G.out_stride), dout = at_var_base(V, seq, V.a.dout_stride);
        dq = at_var_base(V, seq, V.a.dq_stride), kv = at_var_base(V, seq, V.a.f.new_stride);
        dkv = at_var_base(V, seq, V.a.dkv_stride), lse = at_var_base(V, seq, G.n_heads);
    }
};

// the forward blocks of one sequence.  q and out as prefill_attn_count_out_of_range; K, V rows at kv_stride; lse fp32 [rows][n_heads]
void at_walk_fwd(const AtGeom& A, int seq, const AtBase& B, const AtSizes& S, AtWorst& w) {
    const PaGeom& G = A.f.g;
    const long long qb = 2 * (B.q + at_seq_base(A, seq, G.q_stride)), ob = 2 * (B.out + at_seq_base(A, seq, G.out_stride));
    const long long kb = 2 * (B.kv + at_seq_base(A, seq, A.f.new_stride)), lb = 4 * (B.lse + at_seq_base(A, seq, G.n_heads));
    const int per_seq = at_q_blocks_per_seq(A);
    for (int block = 0; block < per_seq; ++block) {
        const int qtile = pa_block_qtile(G, block), head = pa_block_head(G, block), kvh = pa_kv_head(G, head);
        // pa_walk_q_out names the operand by its size within one sequence: q loads are 16 bytes, out stores 8
        pa_walk_q_out(G, block, [&](long long b, int bytes, long long) {
            if (bytes == 16) w(qb + b, bytes, S.q); else w(ob + b, bytes, S.out);
        });
        for (int row = qtile * PA_QT; row < qtile * PA_QT + PA_QT && row < G.t; ++row)
            w(lb + 4 * pa_lse_off(G, row, head), 4, S.lse);
        const int n_tiles = pa_key_tiles(G, qtile);
        for (int tile = 0; tile < n_tiles; ++tile)
            for (int c = 0; c < PA_CHUNKS; ++c)                // K and V share the offset
                w(kb + 2 * pa8_new_off(A.f, pa8_new_row(G, tile * PA_KT + (c >> 4)), kvh, c & 15), 16, S.kv);
    }
}

// the delta launch over all of A's rows
void at_walk_delta(const AtGeom& A, const AtSizes& S, AtWorst& w) {
    const PaGeom& G = A.f.g;
    for (long long block = 0; block < at_delta_blocks(A); ++block)
        for (int slot = 0; slot < AT_DELTA_PAIRS; ++slot) {
            const long long pair = at_delta_pair(A, block, slot), grow = pair / G.n_heads;
            const int head = (int)(pair % G.n_heads), seq = (int)(grow / G.t), row = (int)(grow % G.t);
            for (int ch = 0; ch < 16; ++ch) {
                w(2 * at_out_off(A, seq, row, head, ch), 16, S.out);
                w(2 * at_dout_off(A, seq, row, head, ch), 16, S.dout);
            }
            w(4 * at_lse_off(A, seq, row, head), 4, S.lse);
        }
}

// the dK / dV blocks of one sequence
void at_walk_dkv(const AtGeom& A, int seq, const AtBase& B, const AtSizes& S, AtWorst& w) {
    const PaGeom& G = A.f.g;
    const int rep = G.n_heads / G.n_kv;
    for (int block = 0; block < at_dkv_blocks_per_seq(A); ++block) {
        const int kblock = at_dkv_kblock(A, block), kvh = at_dkv_kvh(A, block);
        for (int kr = 0; kr < AT_KB; ++kr) {
            const int key = kblock * AT_KB + kr;
            for (int ch = 0; ch < 16; ++ch) w(2 * (B.kv + at_kv_off(A, seq, at_row(A, key), kvh, ch)), 16, S.kv);
            if (key < G.t)
                for (int d = 0; d < PA_HD; d += 4) w(2 * (B.dkv + at_dkv_off(A, seq, key, kvh, d)), 8, S.dkv);
        }
        const int tile0 = at_dkv_first_tile(kblock), n_tiles = at_dkv_end_tile(A) - tile0;
        for (int step = 0; step < rep * n_tiles; ++step) {
            const int head = kvh * rep + step / n_tiles, tile = tile0 + step % n_tiles;
            for (int c = 0; c < PA_CHUNKS; ++c) {
                const int rr = at_row(A, tile * AT_QT + (c >> 4));
                w(2 * (B.q + at_q_off(A, seq, rr, head, c & 15)), 16, S.q);
                w(2 * (B.dout + at_dout_off(A, seq, rr, head, c & 15)), 16, S.dout);
            }
            for (int lane = 0; lane < 64; ++lane)
                w(4 * (B.lse + at_lse_off(A, seq, at_row(A, tile * AT_QT + lane), head)), 4, S.lse);
        }
    }
}

// the dQ blocks of one sequence
void at_walk_dq(const AtGeom& A, int seq, const AtBase& B, const AtSizes& S, AtWorst& w) {
    const PaGeom& G = A.f.g;
    const int per_seq = at_q_blocks_per_seq(A);
    for (int block = 0; block < per_seq; ++block) {
        const int qtile = pa_block_qtile(G, block), head = pa_block_head(G, block), kvh = pa_kv_head(G, head);
        for (int wave = 0; wave < PA_WAVES; ++wave)
            for (int r = 0; r < 32; ++r) {
                const int qpos = pa_q_row(G, qtile, wave, r), row = qtile * PA_QT + wave * 32 + r;
                for (int ch = 0; ch < 16; ++ch) {
                    w(2 * (B.q + at_q_off(A, seq, qpos, head, ch)), 16, S.q);
                    w(2 * (B.dout + at_dout_off(A, seq, qpos, head, ch)), 16, S.dout);
                }
                w(4 * (B.lse + at_lse_off(A, seq, qpos, head)), 4, S.lse);
                if (row < G.t)
                    for (int d = 0; d < PA_HD; d += 4) w(2 * (B.dq + at_dq_off(A, seq, row, head, d)), 8, S.dq);
            }
        const int n_tiles = pa_key_tiles(G, qtile);
        for (int tile = 0; tile < n_tiles; ++tile)
            for (int c = 0; c < PA_CHUNKS; ++c)
                w(2 * (B.kv + at_kv_off(A, seq, at_row(A, tile * PA_KT + (c >> 4)), kvh, c & 15)), 16, S.kv);
    }
}
}  // namespace

// The forward: the largest number of bytes by which an address passes the end of its operand or runs in front of it, 0 when
// none does.
long long attn_train_fwd_count_out_of_range(const AtGeom& A) {
    const AtSizes S(A, (long long)A.n_seq * A.f.g.t);
    AtWorst w;
    for (int seq = 0; seq < A.n_seq; ++seq) at_walk_fwd(A, seq, AtBase(), S, w);
    return w.worst;
}

// The three backward launches, the same way, over q, k, v, out, dout, lse, delta, dq, dk, dv.
long long attn_train_bwd_count_out_of_range(const AtGeom& A) {
    const AtSizes S(A, (long long)A.n_seq * A.f.g.t);
    AtWorst w;
    at_walk_delta(A, S, w);
    for (int seq = 0; seq < A.n_seq; ++seq) {
        at_walk_dkv(A, seq, AtBase(), S, w);
        at_walk_dq(A, seq, AtBase(), S, w);
    }
    return w.worst;
}

// The variable-length launches: every block of the grid that does not return at once, as its kernel composes it -- the
// sequence's own geometry, the prefix's base on every pointer, the walkers above at seq = 0 -- against operands of cu[n_seq] rows.
long long attn_train_varlen_fwd_count_out_of_range(const AtVarGeom& V) {
    const AtSizes S(V.a, at_var_rows(V));
    AtWorst w;
    for (int seq = 0; seq < V.a.n_seq; ++seq) at_walk_fwd(at_var_seq(V, seq), 0, AtBase(V, seq), S, w);
    return w.worst;
}

long long attn_train_varlen_bwd_count_out_of_range(const AtVarGeom& V) {
    const AtSizes S(V.a, at_var_rows(V));
    AtWorst w;
    at_walk_delta(at_var_all(V), S, w);
    for (int seq = 0; seq < V.a.n_seq; ++seq) {
        at_walk_dkv(at_var_seq(V, seq), 0, AtBase(V, seq), S, w);
        at_walk_dq(at_var_seq(V, seq), 0, AtBase(V, seq), S, w);
    }
    return w.worst;
}

}  // namespace qeft
