// Geometry and index arithmetic of the MSE parameter search (calib_mse.hip; calibrate.mse_search).
//
// qeft_mse_search    per row of x fp32 [n][g] (row stride ld >= g, read in place): the (scale, zero) that the reference's
//   Quantizer.find_params(mse=True) finds on the asymmetric grid -- num ranges i = 1 .. num, 2^bits zero points zp per range,
//   scored by sum_j |x_j - q_j|^2.4, the first minimum in the order (i ascending, zp ascending) winning.
//
//   One lane per (row, zero point): a wave64 holds ms_rows(bits) = 4 rows at 4 bits, 8 rows at 3 bits, and a block is ONE wave --
//   nothing is shared between rows, so a wider block would buy only a dearer barrier.  The wave walks its rows in tiles of
//   MS_TILE = 128 columns (any g fits; a lane's sum has one order, ascending j).  Per tile and range i the row's lanes first stage,
//   one column each in turn, what does not depend on the zero point: x_round = rint(x_j / scale_i) (ONE IEEE division per
//   (row, i, j), not one per zero point) and the score term of the element where it does not clamp.  Then every lane walks the
//   tile, reads both as a broadcast and recomputes the term only where ITS zero point clamps the element (the clamped x_q is one
//   of two values per lane and range).  The num running sums of a lane live in LDS at [i][lane], touched once per (tile, i).
//
//   Pinned (fp32, one rounding per operation, nothing contracted, IEEE division, rint = half to even, eps = 1e-8f):
//     xmin = min(min_j x_j, 0);  xmax = max(max_j x_j, 0);  tmp_max = fl(fl((xmax - xmin) / num) * i);  delta = max(tmp_max / maxq, eps)
//     x_round = rint(x_j / delta);  new_min = 0 - fl(zp * delta);  zero = min(max(0 - rint(new_min / delta), 0), maxq)
//     x_q = delta * (min(max(x_round + zero, 0), maxq) - zero);  d = x_j - x_q
//     at the end, for the winner: new_max = tmp_max - fl(zp * delta);  lo = min(new_min, 0);  hi = max(new_max, 0)
//     scale = max((hi - lo) / maxq, eps);  zero = min(max(0 - rint(lo / scale), 0), maxq)
//   Where the element does not clamp, (x_round + zero) - zero == x_round exactly (integers far below 2^24), so x_q = delta * x_round
//   whatever zp is: that is what the staging shares.  (x_round = -0 gives x_q = -0 there and +0 in the long form; d = x_j either way.)
//   The kernel's own: the score term |d|^2.4 = d * d * exp2(0.4 * log2 |d|) on the hardware transcendentals (exactly 0 for d == 0).
#pragma once
#include <hip/hip_runtime.h>

namespace qeft {

#define MSE_HD __host__ __device__ inline

constexpr int MS_THREADS = 64;                          // one wave
constexpr int MS_TILE = 128;                            // columns per tile
constexpr int MS_MAX_NUM = 40;                          // ranges: the LDS sums are [MS_MAX_NUM][MS_THREADS]
constexpr int MS_MAX_G = 1 << 15;

struct MsGeom {
    int n, g, ld, bits, num;
};

MSE_HD int ms_lanes(int bits) { return 1 << bits; }                            // lanes (zero points) of a row
MSE_HD int ms_rows(int bits) { return MS_THREADS >> bits; }                    // rows of a wave
MSE_HD int ms_blocks(const MsGeom& G) { return (G.n + ms_rows(G.bits) - 1) / ms_rows(G.bits); }
MSE_HD int ms_tiles(const MsGeom& G) { return (G.g + MS_TILE - 1) / MS_TILE; }
// the row a lane works for; a lane past n repeats the last row and stores nothing
MSE_HD int ms_row(const MsGeom& G, int block, int lane) {
    const int row = block * ms_rows(G.bits) + (lane >> G.bits);
    return row < G.n ? row : G.n - 1;
}
// element offset in x of column `col` (< g) of row `row` (< n)
MSE_HD long long ms_x_off(const MsGeom& G, int row, int col) { return (long long)row * G.ld + col; }

// ---- device side: the lines that calib_mse.hip and the in-launch search of calib_rows.hip share (products, min and max only:
// nothing here could be contracted, whichever side of a unit's contract pragma the include stands on)
constexpr float MS_EPS = 1e-8f;

// |d|^2.4 as d * d * 2^(0.4 log2 |d|) on v_log_f32 / v_exp_f32: log2(0) = -inf and 2^-inf = 0, so d == 0 gives exactly 0.
__device__ __forceinline__ float ms_term(float d) {
    const float e = __builtin_amdgcn_exp2f(0.4f * __builtin_amdgcn_logf(fabsf(d)));
    return d * d * e;
}

__device__ __forceinline__ float ms_clamp(float v, float maxq) { return fminf(fmaxf(v, 0.f), maxq); }

// ---- host side: calib_mse.hip
hipError_t mse_search_launch(const void* x, void* scale, void* zero, const MsGeom& G, hipStream_t st);

}  // namespace qeft
