// The NT logit tile of the fused lm_head kernels: geometry, global offsets and the k loop shared by lm_head_nll.hip (forward:
// lse, target logit, argmax) and lm_head_nll_grad.hip (backward: g = softmax - onehot).  Both kernels run THIS loop, so a logit
// is the same fp32 value in both, bit for bit (DESIGN.md sections 4.13, 4.14).
#pragma once
#include "qeft_common.h"

namespace qeft {

constexpr int LN_BN = 128;     // vocabulary columns of a tile
constexpr int LN_BK = 64;      // k of a staged tile: rows of 128 bytes, 8 chunks of 16
constexpr int LN_RED_THREADS = 64;

struct LnGeom {
    int x_stride, t, hidden, vocab;
};

#define LN_HD __host__ __device__ __forceinline__

LN_HD int ln_col_tiles(const LnGeom& G) { return (G.vocab + LN_BN - 1) / LN_BN; }
LN_HD int ln_waves(const LnGeom& G) { return G.t <= 64 ? 2 : 4; }                   // 64- or 128-row block tile
LN_HD int ln_row_tiles(const LnGeom& G, int nw) { return (G.t + 32 * nw - 1) / (32 * nw); }
// Block ids go round the 8 XCDs (each with an L2 of its own).  XCD c takes a contiguous run of the tile order -- ids c, c + 8, ...
// become consecutive -- and in that order the row tiles that share a weight tile are adjacent: a weight tile is fetched into ONE
// L2, and the weight streams from HBM once.  (Dealt round the XCDs as they come, every weight tile crosses the fabric into as many
// L2s as it has row tiles: 402 -> 288 us at t = 512, hidden 4096, vocab 32000.)  A bijection for any grid size.
LN_HD int ln_tile_order(int nblocks, int block) {
    const int q = nblocks / 8, rem = nblocks % 8, xcd = block % 8;
    return xcd * q + min(xcd, rem) + block / 8;
}
LN_HD int ln_block_row_tile(const LnGeom& G, int nw, int block) {
    return ln_tile_order(ln_row_tiles(G, nw) * ln_col_tiles(G), block) % ln_row_tiles(G, nw);
}
LN_HD int ln_block_col_tile(const LnGeom& G, int nw, int block) {
    return ln_tile_order(ln_row_tiles(G, nw) * ln_col_tiles(G), block) / ln_row_tiles(G, nw);
}
// LDS slot `slot` of tile row `trow` holds k-chunk slot ^ ((trow >> 1) & 7): two 128-byte rows share a period of the 64 banks, so
// the 8 rows of one parity that a 16-lane ds_read_b128 group touches need 8 different slots
LN_HD int ln_chunk(int trow, int slot) { return slot ^ ((trow >> 1) & 7); }
// element offsets of the 16-byte piece (tile row, slot) of k-tile kt; rows / columns past the end read the last one
LN_HD long long ln_x_off(const LnGeom& G, int row_tile, int nw, int trow, int slot, int kt) {
    const int row = min(row_tile * 32 * nw + trow, G.t - 1);
    return (long long)row * G.x_stride + kt * LN_BK + ln_chunk(trow, slot) * 8;
}
LN_HD long long ln_w_off(const LnGeom& G, int col_tile, int trow, int slot, int kt) {
    const int col = min(col_tile * LN_BN + trow, G.vocab - 1);
    return (long long)col * G.hidden + kt * LN_BK + ln_chunk(trow, slot) * 8;
}
LN_HD bool ln_target_ok(const LnGeom& G, int tg) { return tg >= 0 && tg < G.vocab; }

// LDS reads of DMA-written tiles go through inline asm (as in gemm_w4.hip): hipcc otherwise drains the DMA in flight with
// s_waitcnt vmcnt(0) before any ds_read that might alias it.  The values are usable only after ln_lds_wait().
__device__ __forceinline__ u32x4 ln_lds_read16(uint32_t addr) {
    u32x4 v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr) : "memory");
    return v;
}
__device__ __forceinline__ void ln_lds_wait() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

template <int NW>
struct LnTile {
    static constexpr int BM = 32 * NW;
    static constexpr int XI = 4, WI = 16 / NW;                 // DMA instructions per wave and k-tile (8 tile rows = 1 KB each)
    static constexpr int X_BYTES = BM * LN_BK * 2, BUF_BYTES = X_BYTES + LN_BN * LN_BK * 2;
    static constexpr int LDS_BYTES = 2 * BUF_BYTES;            // [2][x tile | w tile]
};

// The logits of tile (row_tile, col_tile) of a block of NW waves: on return register e of acc[vt] is the logit of column
// col_tile * 128 + 32 vt + (e & 3) + 8 (e >> 2) + 4 (lane >> 5), token row_tile * 32 NW + 32 wave + (lane & 31).
// lds: LnTile<NW>::LDS_BYTES bytes, 16-byte aligned.  Every thread of the block calls it: there is one s_barrier per k-tile inside.
template <int NW>
__device__ __forceinline__ void ln_logit_tile(const f16* __restrict__ x, const f16* __restrict__ w, const LnGeom& G, int row_tile,
                                              int col_tile, unsigned char* lds, f32x16 (&acc)[4]) {
    typedef LnTile<NW> T;
    constexpr int XI = T::XI, WI = T::WI, X_BYTES = T::X_BYTES, BUF_BYTES = T::BUF_BYTES;
    const uint32_t lds0 = (uint32_t)(uintptr_t)lds;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int ktiles = G.hidden / LN_BK;

    // DMA sources of k-tile 0: piece p of a tile = its rows 8 p .. 8 p + 7, lane -> (row lane / 8, slot lane % 8); the offsets are
    // linear in kt (ln_x_off(.., kt) = ln_x_off(.., 0) + kt * LN_BK), so a k-tile is one add away
    const f16* xsrc[XI];
    const f16* wsrc[WI];
#pragma unroll
    for (int i = 0; i < XI; ++i) xsrc[i] = x + ln_x_off(G, row_tile, NW, (wave * XI + i) * 8 + (lane >> 3), lane & 7, 0);
#pragma unroll
    for (int i = 0; i < WI; ++i) wsrc[i] = w + ln_w_off(G, col_tile, (wave * WI + i) * 8 + (lane >> 3), lane & 7, 0);

    auto stage = [&](int kt) {
        unsigned char* base = lds + (kt & 1) * BUF_BYTES;
#pragma unroll
        for (int i = 0; i < XI; ++i)
            __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(xsrc[i] + (size_t)kt * LN_BK),
                                             (void __attribute__((address_space(3)))*)(base + (wave * XI + i) * 1024), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < WI; ++i)
            __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(wsrc[i] + (size_t)kt * LN_BK),
                                             (void __attribute__((address_space(3)))*)(base + X_BYTES + (wave * WI + i) * 1024), 16, 0, 0);
    };

#pragma unroll
    for (int vt = 0; vt < 4; ++vt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[vt][e] = 0.f;

    // fragment of k-step ks: tile row * 128 + slot of chunk 2 ks + h (every 32-row block keeps (row >> 1) & 7 of r)
    uint32_t foff[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) foff[ks] = (uint32_t)(r * 128 + (ln_chunk(r, 2 * ks + h) << 4));
    const uint32_t xrow = (uint32_t)(wave * 32 * 128);

    stage(0);
    for (int kt = 0; kt < ktiles; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's pieces of tile kt landed
        __builtin_amdgcn_s_barrier();                          // ... and everyone's; everyone has read tile kt - 1
        if (kt + 1 < ktiles) stage(kt + 1);                    // into the buffer of tile kt - 1
        const uint32_t tb = lds0 + (uint32_t)(kt & 1) * BUF_BYTES;
        u32x4 fx[2], fw[2][4];
        fx[0] = ln_lds_read16(tb + xrow + foff[0]);
#pragma unroll
        for (int vt = 0; vt < 4; ++vt) fw[0][vt] = ln_lds_read16(tb + X_BYTES + vt * 32 * 128 + foff[0]);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            ln_lds_wait();
            if (ks + 1 < 4) {                                  // the next k-step's fragments, in flight behind these MFMAs
                fx[(ks + 1) & 1] = ln_lds_read16(tb + xrow + foff[ks + 1]);
#pragma unroll
                for (int vt = 0; vt < 4; ++vt) fw[(ks + 1) & 1][vt] = ln_lds_read16(tb + X_BYTES + vt * 32 * 128 + foff[ks + 1]);
            }
#pragma unroll
            for (int vt = 0; vt < 4; ++vt)
                acc[vt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, fw[ks & 1][vt]),
                                                                __builtin_bit_cast(h8, fx[ks & 1]), acc[vt], 0, 0, 0);
        }
    }
}

}  // namespace qeft
