// Geometry and contract of the row-owned GPTQ loop (calib_rows.hip; calibrate.gptq_reorder(loop="rows")).
//
// qeft_gptq_rows    the WHOLE error-feedback loop of one weight matrix in ONE launch.  GPTQ's rows are independent: given the
//   factor U (Hd^-1 = U^T U), a row's codes, errors and feedback depend on that row alone.  So a workgroup of 256 threads owns 16
//   rows and sweeps every column of them, forming the trailing update lazily, left-looking:
//       w[rows, tile] = W0[rows, tile] - Err[rows, 0:depth] . U[0:depth, tile]
//   No workspace, no atomics, no flags, no communication between workgroups, nothing on the host between blocks.
//
//   Operands.  w0 fp32 [n][k] (row stride ld_w; columns in `ids` order, dead columns zeroed; read only), hinv fp32 [k][k] (stride
//   ld_h; the upper factor, entries [j][i] with j <= i are used, what lies below the diagonal is loaded with the 128 x 128
//   diagonal blocks and masked), n_nonout live columns (k - n_nonout even, may be 0), maxq 7 or 15.
//   q fp32 [n][k]: dequantised values in the live columns, W0 - Err . U[:n_nonout, n_nonout:] in the others.  err fp32
//   [n][n_nonout]: a result AND the kernel's own left-looking operand.  scale, zero fp32 [n][k / 128]: one pair per started live
//   group, the last repeated up to k / 128.
//
//   The columns are walked in k / 128 aligned tiles of 128 (k % 128 == 0, so every tile is whole and 16-byte aligned).  A tile
//   that starts below n_nonout is a live block of count = min(128, n_nonout - start) columns; one that starts at or above it
//   holds outlier columns only.  Three phases per tile:
//     1. the left-looking product  acc[16 x 128] = Err[rows, 0:depth] . U[0:depth, tile]  on v_mfma_f32_16x16x4f32; depth = the
//        tile's start for a live block, n_nonout for an outlier tile.  Wave w owns columns 32 w .. 32 w + 31 (two accumulators).
//        U comes through LDS in chunks of 32 rows x 128 columns ([32][144] floats: the 4 rows x 16 columns of an operand read hit
//        64 different banks), Err in chunks of 16 x 32 ([16][36]); both double-buffered, 16-byte / 8-byte global loads of the next
//        chunk in flight behind the current chunk's MFMAs, one barrier per chunk.  Rows of the chunk at or past depth are staged
//        as zeros and never read from memory (an outlier tile's depth need not be a multiple of 4).  One fixed order, k ascending.
//     2. the block start  w = W0[rows, tile] - acc: the accumulators go through LDS ([16][132]) into the sweep's layout -- thread
//        t holds row t / 16, columns c, c + 16, .., c + 112 with c = t % 16 -- and the row's min / max over the live columns is
//        reduced over its 16 lanes (lane ^ 1, 2, 4, 8).  The pair is qp_minmax_pair<true> (quant_pack.h): the lines of
//        quant.minmax_params as torch runs them on the device between the block launches (the scale is the product with
//        fl(1 / maxq) there, not the quotient that qeft_quant_pack's find mode and the CPU give).  The 128 x 128 diagonal block
//        of U was brought into LDS (64 KiB, zeros below the diagonal) in four pieces riding on the first four chunks of phase 1.
//     3. the serial sweep, no barrier in it: at step i every lane of the row's 16 reads w_i from its owner by a cross-lane read
//        and runs the pinned lines of calib.h --  x = w_i / s;  c = min(max(rint(x) + z, 0), maxq);  q = s (c - z);
//        e = (w_i - q) / U[i][i];  w_j = w_j - fl(e U[i][j]) for the lane's columns j >= i -- the 16 lanes compute the same q and
//        e bits, the owner keeps them.  The row-i read of the triangle is 16 consecutive words, the same for the wave's 4 rows.
//        A short last block (count < 128) shares its tile with the first outlier columns, which receive that block's feedback
//        here, in the sweep's order; an outlier start that is only 8-byte aligned therefore needs no unaligned access at all.
//        Then q, err and the pair are stored; a barrier (with its wait for the stores) ends the tile, which makes the tile's
//        err visible to the workgroup's own next phase 1.
//   Given the same block-start columns, q, err, scale and zero carry the bits of qeft_gptq_block + quant.minmax_params on the
//   device.  The left-looking sum has its own order (no bit parity with a rocBLAS GEMM is claimed); a rerun gives the same bits.
//   A row's outputs depend on that row and hinv alone -- not on n, the row's index or the grid.
//
//   Every global address: row < n (a thread past n repeats row n - 1 and stores nothing); w0 and q at row * ld + tile start +
//   column with column < 128 and tile start + 128 <= k; hinv at (r < depth <= k) * ld_h + tile start + 4-column piece, or the
//   diagonal block (tile start + i) * ld_h + tile start + piece; err at row * n_nonout + (column < depth <= n_nonout) for loads and
//   (column < count) for stores; scale / zero at row * (k / 128) + tile.
//
// qeft_gptq_rows_mse    the same launch -- phases 1 and 2, the sweep, LDS, workgroup, grid and every address above -- with the
//   block-start pair found by the reference's MSE search (Quantizer.find_params(mse=True): num ranges x 2^bits zero points) over
//   the tile's live block-start columns, between phase 2 and the sweep (gptq_reorder(tuning="mse_fused",
//   loop="rows")).  After phase 2 the 16 lanes of a row hold its 128 block-start columns in registers and nothing outside those
//   lanes enters a row's result, so the search needs no LDS, no barrier and no global address.
//   Pinned, as calib_mse.h (fp32, nothing contracted, IEEE divisions, rint half to even), over the count live columns of the tile:
//     xmin = min(min_j w_j, 0);  xmax = max(max_j w_j, 0);  step = (xmax - xmin) / num
//     per range i = 1 .. num:  tmp_max = fl(step i);  delta = max(tmp_max / maxq, 1e-8f);  x_round = rint(w_j / delta)
//     per zero point zp:  new_min = 0 - fl(zp delta);  zero = clamp(0 - rint(new_min / delta), 0, maxq)
//       x_q = delta (clamp(x_round + zero, 0, maxq) - zero);  d = w_j - x_q;  term = d d exp2(0.4 log2 |d|)  (0 for d == 0)
//     the winner's closing lines: new_max = tmp_max - fl(zp delta);  lo = min(new_min, 0);  hi = max(new_max, 0)
//       scale = max((hi - lo) / maxq, 1e-8f);  zero = clamp(0 - rint(lo / scale), 0, maxq)
//   so a candidate's residuals are the bits calibrate.mse_params gives on the CPU.  A candidate's score has the kernel's OWN
//   order: lane c sums the terms of its columns c, c + 16, .., c + 112 (ascending; a column >= count adds an exact +0), and the
//   row's 16 partials are combined by the fixed tree ((p_c + p_c^8) + (p_c^4 + p_c^12)) + .. over lane ^ 8, 4, 2, 1 -- a
//   reduce-scatter that leaves lane c with the score of zero point c % 2^bits.  The order does not depend on the row's index, n,
//   the grid or the lane that asks; it is NOT qeft_mse_search's ascending-j order, so no bit parity with tuning="mse" is claimed.
//   The winner is the first minimum in the reference's order (i ascending, then zp ascending, strict <): each lane keeps the
//   first minimum over i of its zero point, one 16-lane arg-min on (score, i 2^bits + zp) follows, and all 16 lanes form the pair
//   from the same key -- the sweep needs the same s and z bits in every lane of the row.  Without a candidate below infinity the
//   pair is that of (xmin, xmax).  A tile without a live column repeats the last pair; a short last block searches its count
//   columns.  num is 1 .. 40 (MS_MAX_NUM).
//
// qeft_gptq_rows_pc, qeft_gptq_rows_pc_mse    the same launch with ONE pair per row, the reference's --groupsize -1 (DESIGN.md
//   section 4.26; gptq_reorder(group_size=-1, loop="rows")): scale and zero are fp32 [n], every other operand, the grid, the
//   workgroup, phases 1 and 3, LDS and every address above are unchanged; phase 2 searches nothing.  The pair is found in
//   phase 0, per workgroup before tile 0, from W0 itself (dead columns zeroed, no feedback yet -- the reference's find_params
//   before its loop): thread (row, c) walks its row's live columns c + 16 m of every live tile, W0 at row * ld_w + column with
//   column < n_nonout.
//     min-max   the row's extremes over the live columns and 0 (16-lane reduce), then qp_minmax_pair<true>: the bits of
//               quant.minmax_params(W0[:, :n_nonout], n_nonout, bits) as torch runs it on the device.
//     MSE       a second pass (it needs xmin / xmax): the search above, num ranges x 2^bits zero points, over the row's n_nonout
//               columns.  Tiles outer, ranges inner: per (tile, range) the per-lane partials and the reduce-scatter of the tile
//               search, then lane c adds its zero point's tile sum into its own slot of a score table [num][256] floats in LDS
//               (40 KiB at num = 40).  The table lies over the Us and Es regions, idle until phase 1 of tile 1, so GR_LDS does not
//               grow; a lane touches only its own slots (a wave's 64 lanes hit 64 consecutive words), so the pass has no barrier;
//               one barrier follows it.  No score lives in a dynamically indexed register array (that would be scratch).
//               A score is: the tile sum in the order stated above, then tiles ascending -- independent of n, the row's index
//               and the grid; not qeft_mse_search's order (no bit parity with tuning="mse").  The lane then takes the first
//               minimum over i of its slots (strict <), and the 16-lane arg-min and the closing lines are the tile search's.
//   The sweep of every tile runs with the row's pair; scale[row] and zero[row] are stored once.  Rows are independent, a rerun
//   gives the same bits, no workspace, no atomics.
#pragma once
#include <hip/hip_runtime.h>

namespace qeft {

constexpr int GR_ROWS = 16;                            // rows of a workgroup
constexpr int GR_THREADS = 256;
constexpr int GR_B = 128;                               // tile == block == group
constexpr int GR_BK = 32;                               // depth of a staged chunk
constexpr int GR_LDU = GR_B + 16;                       // row stride of a staged U chunk
constexpr int GR_LDE = GR_BK + 4;                       // row stride of a staged Err chunk
constexpr int GR_LDC = GR_B + 4;                        // row stride of the accumulators' turn
constexpr int GR_MAX_K = 1 << 15;
constexpr int GR_LDS_FLOATS = 2 * GR_BK * GR_LDU + 2 * GR_ROWS * GR_LDE + GR_ROWS * GR_LDC + GR_B * GR_B;
constexpr int GR_LDS = GR_LDS_FLOATS * 4;               // 115 456 bytes: one workgroup per CU
constexpr int GR_PC_TABLE_FLOATS = 40 * GR_THREADS;     // the per-channel search's scores [MS_MAX_NUM][256], over Us and Es
static_assert(GR_PC_TABLE_FLOATS <= 2 * GR_BK * GR_LDU + 2 * GR_ROWS * GR_LDE, "the score table must end before Cs");

struct GrGeom {
    int n, k, ld_w, ld_h, n_nonout;
};
__host__ __device__ inline int gr_blocks(const GrGeom& G) { return (G.n + GR_ROWS - 1) / GR_ROWS; }

// ---- host side: calib_rows.hip
hipError_t gptq_rows_launch(const void* w0, const void* hinv, void* q, void* err, void* scale, void* zero, const GrGeom& G,
                            float maxq, hipStream_t st);
hipError_t gptq_rows_mse_launch(const void* w0, const void* hinv, void* q, void* err, void* scale, void* zero, const GrGeom& G,
                                int bits, int num, hipStream_t st);
// per-channel: scale and zero are fp32 [n]
hipError_t gptq_rows_pc_launch(const void* w0, const void* hinv, void* q, void* err, void* scale, void* zero, const GrGeom& G,
                               float maxq, hipStream_t st);
hipError_t gptq_rows_pc_mse_launch(const void* w0, const void* hinv, void* q, void* err, void* scale, void* zero, const GrGeom& G,
                                   int bits, int num, hipStream_t st);

}  // namespace qeft
