// Geometry and index arithmetic of the calibration kernels (calib.hip).  Every global address a launch of
// qeft_hessian_accum forms comes out of the ha_* functions below, which the host-side enumeration behind
// qeft_hessian_accum_check_extents walks too.  qeft_gptq_block has its grid here (gb_blocks); its addresses are row * ld + column
// under the guards row < n, column < count, written out in the kernel.
//
// qeft_hessian_accum    H <- beta * H + alpha * X^T X.   X fp16 [T][K] row-major, H fp32 [K][K], K % 64 == 0, T >= 1.
//   One block of 4 waves per 128 x 128 tile (ti, tj), ti <= tj, of H: the upper triangle of tiles only.  The block walks ALL T rows
//   in ascending tiles of 64, so an element's sum has one order whatever the grid is: MFMA 32x32x16 steps over rows 16 s .. 16 s +
//   15 for s = 0, 1, 2, ..., fp32 accumulation, no split, no atomics.  Rows >= T and columns >= K are staged as zeros (never read
//   from memory), so a ragged T adds exact zeros.  Both operands are columns of X: the staged image is [64 rows][128 columns] fp16
//   with 256-byte rows under the chunk XOR of ha_chunk, read through the transposing LDS read.
//   Epilogue, pinned: S the fp32 sum; out = fl(fl(beta * H[i][j]) + fl(alpha * S)), nothing contracted; with beta == 0 H is not
//   read (the term is +0).  H[i][j] is read for i <= j ONLY and `out` is stored to H[i][j] and to H[j][i]: both triangles carry
//   the same bits by construction, and what the lower triangle held before does not matter.
//
// qeft_gptq_block       one block (count <= 128 columns) of the GPTQ error-feedback loop, one thread per row of W.
//   The count x count upper triangle of the inverse factor sits in LDS (64 KiB), the thread's row in registers.  The arithmetic is
//   fp32, one rounding per operation, nothing contracted, IEEE division, rint = round half to even:
//     x = w_i / scale;  c = min(max(rint(x) + zero, 0), maxq);  q = scale * (c - zero);  e = (w_i - q) / Hinv1[i][i]
//     w_j = w_j - fl(e * Hinv1[i][j])   for j = i .. count - 1
//   A row's results depend on that row, its scale and zero and the triangle alone -- not on N, the row's index or the grid.
#pragma once
#include <hip/hip_runtime.h>

namespace qeft {

#define CAL_HD __host__ __device__ inline

constexpr int HA_TILE = 128;                            // edge of an H tile
constexpr int HA_BT = 64;                               // rows of X in a staged tile
constexpr int HA_THREADS = 256;
constexpr int HA_IMG_BYTES = HA_BT * HA_TILE * 2;       // one staged image: 16 KiB
constexpr int HA_MAX_K = 1 << 15;
constexpr int HA_MAX_T = 1 << 24;
constexpr int HA_MAX_K_ENUM = 4096;                      // the address enumeration keeps one byte per element of H: 16 MiB here

struct HaGeom {
    int t, k;
};

CAL_HD int ha_tiles(const HaGeom& G) { return (G.k + HA_TILE - 1) / HA_TILE; }
CAL_HD int ha_blocks(const HaGeom& G) { return ha_tiles(G) * (ha_tiles(G) + 1) / 2; }
CAL_HD int ha_row_tiles(const HaGeom& G) { return (G.t + HA_BT - 1) / HA_BT; }
// block -> tile (ti, tj) of the upper triangle, row by row: ti = 0 has tiles(G) blocks, ti = 1 one fewer, ...
CAL_HD void ha_block_tile(const HaGeom& G, int block, int& ti, int& tj) {
    int i = 0, rem = block;
    const int nt = ha_tiles(G);
    while (rem >= nt - i) {
        rem -= nt - i;
        ++i;
    }
    ti = i;
    tj = i + rem;
}
// the image: LDS slot `slot` (16 bytes) of image row `trow` holds column chunk ha_chunk(trow, slot) (an involution)
CAL_HD int ha_chunk(int trow, int slot) { return slot ^ (((trow & 3) << 2) | ((trow >> 2) & 3)); }
// staging piece p (0..3) of thread tid: image row and slot
CAL_HD int ha_stage_row(int p, int tid) { return (p * HA_THREADS + tid) >> 4; }
CAL_HD int ha_stage_slot(int p, int tid) { return (p * HA_THREADS + tid) & 15; }
// element offset in X of the 8 columns staged at (trow, slot) of column tile `tile`, row tile kt; -1: past T or K, staged as zeros
CAL_HD long long ha_x_off(const HaGeom& G, int tile, int trow, int slot, int kt) {
    const int row = kt * HA_BT + trow, col = tile * HA_TILE + ha_chunk(trow, slot) * 8;
    return row < G.t && col < G.k ? (long long)row * G.k + col : -1;
}
CAL_HD long long ha_h_off(const HaGeom& G, int row, int col) { return (long long)row * G.k + col; }
// byte offset in an image of the transposing read of lane `lane`: the 32 columns 64 half64 + 32 sub + (lane & 31), rows
// 8 (lane >> 5) + 4 quad .. + 3 of the k-step's 16.  Lane 4 q + p of a 16-lane group addresses row q, columns 4 p .. 4 p + 3.
CAL_HD int ha_frag_off(int lane, int half64, int sub, int quad) {
    const int q = (lane & 15) >> 2, p = lane & 3, h = lane >> 5;
    const int trow = 8 * h + 4 * quad + q;
    const int ch = half64 * 8 + sub * 4 + ((lane >> 4) & 1) * 2 + (p >> 1);
    return trow * 256 + (ha_chunk(trow, ch) << 4) + (p & 1) * 8;
}
// register e of the accumulator (a-tile sub nt, b-tile sub tt) of wave (wm, wn), lane (r = lane & 31, h = lane >> 5)
CAL_HD int ha_acc_row(int ti, int wm, int nt, int h, int e) { return ti * HA_TILE + wm * 64 + nt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h; }
CAL_HD int ha_acc_col(int tj, int wn, int tt, int r) { return tj * HA_TILE + wn * 64 + tt * 32 + r; }

constexpr int GB_MAX_COUNT = 128;
constexpr int GB_THREADS = 64;

struct GbGeom {
    int n, count, ld_w, ld_h;
};
CAL_HD int gb_blocks(const GbGeom& G) { return (G.n + GB_THREADS - 1) / GB_THREADS; }

// ---- host side: calib.hip
hipError_t hessian_accum_launch(const void* x, void* h, const HaGeom& G, float alpha, float beta, hipStream_t st);
long long hessian_accum_count_out_of_range(const HaGeom& G);
hipError_t gptq_block_launch(void* w1, const void* hinv1, const void* scale, const void* zero, void* q1, void* err1, const GbGeom& G,
                             float maxq, hipStream_t st);

}  // namespace qeft
