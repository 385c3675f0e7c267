// Geometry, contract and index arithmetic of the device quantise-and-pack kernel (quant_pack.hip; DESIGN.md section 4.22;
// qeft_cuda.quant_pack, QuantLinear.pack_device, calibrate.rtn_linear).
//
// qeft_quant_pack    ONE pass over an fp16 weight matrix W [n][k] (row stride ld_w; column j of the operand is W[.][j], or
//   W[.][col_ids[j]] where col_ids is given) into the buffers of a QuantLinear: the codes in their kernel layout, the group
//   parameters as the fp16 pair the GEMV / GEMM read, and (find mode) the fp32 parameters themselves.  Group size 128.  The last
//   n_out columns of the operand stay fp16 elsewhere (oweight): they are "dead" here, the k - n_out before them are "live".
//
//   Expression-level spec: QuantLinear.pack, pack_intweight and pack_w3 in qeft_amd/qlinear.py.
//     qweight       4 bits: int16 [n / 4][k], nibble b of [r / 4][(c / 64) * 64 + (r % 4) * 16 + ((c % 64) / 32) * 8 + j] holds the
//                   code of (r, c), c % 32 == 8 b + j.  A dead column's nibble holds its group's zero point.
//                   3 bits: int32 [n / 16][(k - n_out) / 128 * 192], words (step * 64 + chunk * 16 + r % 16) * 3 + 0..2 hold the 32
//                   codes of row r, columns step * 128 + chunk * 32 .. + 31 (pack_w3); dead columns have no words.
//     scales        fp16 [k / 128][n]: the fp32 scale, rounded once
//     scaled_zeros  fp16 [k / 128][n]: -(z * s), the fp32 product rounded once
//     scale_out, zero_out   fp32 [n][k / 128], optional: the parameters used (what find mode found)
//
//   Two modes, by whether scale_in / zero_in (fp32 [n][k / 128]) are given.  Everything is fp32, one rounding per operation,
//   nothing contracted into an FMA, IEEE division, rint = half to even.
//     given   the parameters of every group come from the caller (a GPTQ reconstruction's).  x = float(w16) (exact);
//             zs = fl(z * s);  code = min(max(rint((x + zs) / s), 0), maxq).  QuantLinear.pack runs the same sequence on the host
//             WITHOUT the clamp: there a value outside 0..maxq spills into the neighbouring nibbles of the word.  The device clamps;
//             the two differ only where the host's word is already corrupt.
//     find    round to nearest with the parameters found on the spot, quant.minmax_params over the group's LIVE columns:
//             xmin = min(min_j x_j, 0);  xmax = max(max_j x_j, 0);  xmin == xmax == 0: (xmin, xmax) = (-1, 1);
//             s = (xmax - xmin) / maxq;  z = rint(-xmin / s)  (so an all-positive group gets z = -0, as torch gives);
//             code = min(max(rint(x / s) + z, 0), maxq).
//             A group with no live column (4 bits, n_out >= 128; 3 bits past the stream) repeats the parameters of the last group
//             that has one, as the reconstruction's scale_group does: its wave finds them again from that group's columns.
//   Both: the nibble of a dead column holds min(max(z, 0), maxq) as an integer.  A short last live group (n_out % 128 != 0) is
//   4 bits only.  NaN weights give code 0 in given mode and are outside the contract in find mode.
//
//   Split of the work: one wave owns 16 rows x one 128-column group, lane = chunk * 16 + row (chunk = the 32-column quarter).
//   A lane holds its 32 values in registers (four 16-byte loads; element loads through col_ids), the row's min / max is
//   reduced over its 4 lanes (lane ^ 16, lane ^ 32), the codes are packed in registers.  4 bits: a lane stores 8 int16 = 16
//   bytes at [r / 4][t * 64 + (r % 4) * 16 + (chunk % 2) * 8], t = group * 2 + chunk / 2: 256-byte runs per qweight row and wave.
//   3 bits: a lane stores its 3 words, the wave 768 contiguous bytes.  Lanes of chunk 0 write the wave's 16 fp16 pairs
//   (32-byte runs of scales / scaled_zeros) and the fp32 outputs.  No LDS, no barrier, no atomics; a block is 4 waves on 4
//   neighbouring groups of one row set, the grid (n / 16) x ceil(k / 128 / 4).  Nothing depends on launch order: a rerun
//   gives the same bits.
//
//   Every global address: W at (row < n) * ld_w + (col < k), col a multiple of 8 on the 16-byte route (ld_w % 8 == 0, base
//   aligned) or clamp(col_ids[col], 0, k - 1); qweight at qp_q4_off / qp_q3_off, proven inside by qp_*_elems below; the
//   parameter arrays at row * G + group or group * n + row with row < n, group < G.
//
// qeft_quant_pack_pc    the same operand, modes, pinned lines, code layouts and clamp with ONE pair per row (per-channel, the
//   reference's --groupsize -1): scale_in / zero_in and scale_out / zero_out are fp32 [n], scales /
//   scaled_zeros fp16 [n] (a QuantLinear's [1][n]).  Find mode: quant.minmax_params over ALL the row's live columns and 0
//   (qp_minmax_pair, the quotient: the CPU's bits); every dead nibble holds the row's min(max(z, 0), maxq).
//   Split of the work -- a wave that owns "16 rows x one group" cannot know the row's extremes: a workgroup of QPC_WAVES waves
//   owns 16 rows, wave v takes their groups v, v + QPC_WAVES, ..; lane = chunk * 16 + row as above.  Find mode is two passes:
//   pass 1 takes each wave's extremes over the live columns of its groups (4-lane reduce), one exchange through LDS
//   ([2][QPC_WAVES][16] floats) and ONE barrier give every lane the row's; pass 2 quantises and packs with the per-group body
//   above, reading w again.  Given mode is pass 2 alone (the barrier is not compiled in).  Wave 0 writes the 16 pairs.  Grid n / 16.
//   Addresses: W and qweight as above (group < k / 128, row < n), the parameter arrays at row < n.  A rerun gives the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace qeft {

#define QP_HD __host__ __device__ inline

constexpr int QP_GROUP = 128;                           // the only group size
constexpr int QP_ROWS = 16;                             // rows of a wave
constexpr int QP_WAVES = 4;                             // groups of a block
constexpr int QP_THREADS = 64 * QP_WAVES;
constexpr int QPC_WAVES = 16;                           // per-channel: waves of a workgroup, sharing one row set's groups
constexpr int QPC_THREADS = 64 * QPC_WAVES;
constexpr int QP_MAX_N = 1 << 20;                       // grid x = n / 16
constexpr int QP_MAX_K = 1 << 20;                       // grid y = k / 512

struct QpGeom {
    int n, k, ld_w, n_out, bits;
};

QP_HD int qp_groups(const QpGeom& G) { return G.k / QP_GROUP; }
QP_HD int qp_live(const QpGeom& G) { return G.k - G.n_out; }
QP_HD int qp_last_live_group(const QpGeom& G) { return (qp_live(G) - 1) / QP_GROUP; }
QP_HD int qp_grid_x(const QpGeom& G) { return G.n / QP_ROWS; }
QP_HD int qp_grid_y(const QpGeom& G) { return (qp_groups(G) + QP_WAVES - 1) / QP_WAVES; }
// elements of qweight: int16 at 4 bits, int32 at 3 bits
QP_HD long long qp_q4_elems(const QpGeom& G) { return (long long)(G.n / 4) * G.k; }
QP_HD long long qp_q3_elems(const QpGeom& G) { return (long long)(G.n / 16) * (qp_live(G) / QP_GROUP * 192); }
// first of the 8 int16 a lane stores: row < n, group < G, chunk < 4  ->  offset + 8 <= qp_q4_elems
QP_HD long long qp_q4_off(const QpGeom& G, int row, int group, int chunk) {
    return (long long)(row >> 2) * G.k + (group * 2 + (chunk >> 1)) * 64 + (row & 3) * 16 + (chunk & 1) * 8;
}
// first of the 3 int32 a lane stores: row < n, group < live / 128, lane < 64 with lane % 16 == row % 16  ->  offset + 3 <= qp_q3_elems
QP_HD long long qp_q3_off(const QpGeom& G, int row, int group, int lane) {
    return (long long)(row >> 4) * (qp_live(G) / QP_GROUP * 192) + (long long)(group * 64 + lane) * 3;
}

// The pair of find mode from a row's min and max over the group's live columns with 0 among them (lo <= 0 <= hi): the lines of
// quant.minmax_params, one rounding per operation, IEEE division, rint = half to even (nothing here can contract).  Shared with
// the row-owned GPTQ loop (calib_rows.hip), whose block-start parameters are these as torch runs them ON THE DEVICE: there a
// division by a host scalar is the product with the scalar's fp32 reciprocal, s = fl((xmax - xmin) * fl(1 / maxq)), which is not
// the quotient's bits for most rows (RECIP).  The division of two tensors behind z is IEEE on both.
template <bool RECIP = false>
__device__ __forceinline__ void qp_minmax_pair(float lo, float hi, float maxq, float& s, float& z) {
    if (lo == 0.f && hi == 0.f) {
        lo = -1.f;
        hi = 1.f;
    }
    s = RECIP ? (hi - lo) * (1.f / maxq) : (hi - lo) / maxq;
    z = rintf(-lo / s);
}

// ---- host side: quant_pack.hip.  col_ids, scale_in / zero_in (both or neither), scale_out, zero_out may be null.
hipError_t quant_pack_launch(const void* w, const void* col_ids, const void* scale_in, const void* zero_in, void* qweight, void* scales,
                             void* scaled_zeros, void* scale_out, void* zero_out, const QpGeom& G, hipStream_t st);
// per-channel: the parameter arrays hold one entry per row
hipError_t quant_pack_pc_launch(const void* w, const void* col_ids, const void* scale_in, const void* zero_in, void* qweight,
                                void* scales, void* scaled_zeros, void* scale_out, void* zero_out, const QpGeom& G, hipStream_t st);

}  // namespace qeft
