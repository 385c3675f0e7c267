// The MSE parameter search of the calibrator (qeft_amd/calibrate.py: mse_search, tuning="mse").  The
// contract, the split of the work and the pinned arithmetic: calib_mse.h.  Nothing below may be contracted into an FMA, hence the
// pragma over the whole file; the divisions are IEEE (the compiler's default for fp32).
//
// Every global address is ms_x_off(row, col) with row = ms_row(..) < n and col < g <= ld, or scale / zero at a row < n.
#include <math.h>

#include "qeft_common.h"
#include "calib_mse.h"

#pragma clang fp contract(off)

namespace qeft {

template <int BITS>
__global__ __launch_bounds__(MS_THREADS) void mse_search_kernel(const float* __restrict__ x, float* __restrict__ scale_out,
                                                                float* __restrict__ zero_out, MsGeom G) {
    constexpr int LPR = 1 << BITS, ROWS = MS_THREADS / LPR;
    constexpr float MAXQ = (float)(LPR - 1);
    // one pad element per row: the rows of a wave read the same column at once, from different banks
    __shared__ float xs[ROWS][MS_TILE + 1];                 // the tile of x
    __shared__ float2 st[ROWS][MS_TILE + 1];                // range i of the tile: {x_round, the unclamped element's score term}
    __shared__ float sums[MS_MAX_NUM][MS_THREADS];          // [i - 1][lane]: the lane's running score of range i
    const int lane = threadIdx.x, r = lane >> BITS, zp = lane & (LPR - 1);
    const int row = ms_row(G, blockIdx.x, lane);
    const bool live = blockIdx.x * ROWS + r < G.n;
    const float* xrow = x + ms_x_off(G, row, 0);
    const int g = G.g, num = G.num;
    const float zpf = (float)zp;

    // ---- xmin, xmax: min and max do not round, so any order gives the row's
    float lo = 0.f, hi = 0.f;
    for (int j = zp; j < g; j += LPR) {
        const float v = xrow[j];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
#pragma unroll
    for (int off = 1; off < LPR; off <<= 1) {
        lo = fminf(lo, __shfl_xor(lo, off));
        hi = fmaxf(hi, __shfl_xor(hi, off));
    }
    const float xmin = lo, xmax = hi;
    const float step = (xmax - xmin) / (float)num;          // xrange / num; tmp_max = step * i
    for (int i = 0; i < num; ++i) sums[i][lane] = 0.f;

    for (int t0 = 0; t0 < g; t0 += MS_TILE) {
        const int jn = min(MS_TILE, g - t0);                // uniform
        __syncthreads();                                    // the last tile's readers have left xs and st
        for (int jj = zp; jj < jn; jj += LPR) xs[r][jj] = xrow[t0 + jj];
        for (int i = 1; i <= num; ++i) {
            const float tmp_max = step * (float)i;
            const float delta = fmaxf(tmp_max / MAXQ, MS_EPS);
            const float new_min = 0.f - zpf * delta;
            const float zero = ms_clamp(0.f - rintf(new_min / delta), MAXQ);
            const float q_lo = delta * (0.f - zero), q_hi = delta * (MAXQ - zero);     // x_q of an element clamped to 0 / to maxq
            __syncthreads();                                // xs is written (i == 1); range i - 1's readers have left st
            for (int jj = zp; jj < jn; jj += LPR) {
                const float xv = xs[r][jj];
                const float xr = rintf(xv / delta);
                const float q = delta * xr;
                st[r][jj] = float2{xr, ms_term(xv - q)};
            }
            __syncthreads();
            float acc = sums[i - 1][lane];
#pragma unroll 4
            for (int jj = 0; jj < jn; ++jj) {
                const float2 e = st[r][jj];
                const float c = e.x + zero;
                float term = e.y;
                if (c < 0.f || c > MAXQ) term = ms_term(xs[r][jj] - (c < 0.f ? q_lo : q_hi));
                acc = acc + term;
            }
            sums[i - 1][lane] = acc;
        }
    }

    // ---- the lane's best range (the first among equal scores), then the row's best (i, zp) in the reference's order
    float best = INFINITY;
    int key = 0;                                            // i * LPR + zp; 0: no candidate scored below infinity
    for (int i = 1; i <= num; ++i) {
        const float s = sums[i - 1][lane];
        if (s < best) {
            best = s;
            key = i * LPR + zp;
        }
    }
#pragma unroll
    for (int off = 1; off < LPR; off <<= 1) {
        const float ob = __shfl_xor(best, off);
        const int ok = __shfl_xor(key, off);
        if (ob < best || (ob == best && ok < key)) {
            best = ob;
            key = ok;
        }
    }
    float best_min = xmin, best_max = xmax;                 // the reference's initial pair
    if (key != 0) {
        const float tmp_max = step * (float)(key >> BITS);
        const float delta = fmaxf(tmp_max / MAXQ, MS_EPS);
        const float zd = (float)(key & (LPR - 1)) * delta;
        best_min = 0.f - zd;
        best_max = tmp_max - zd;
    }
    const float mn = fminf(best_min, 0.f), mx = fmaxf(best_max, 0.f);
    const float sc = fmaxf((mx - mn) / MAXQ, MS_EPS);
    const float ze = ms_clamp(0.f - rintf(mn / sc), MAXQ);
    if (live && zp == 0) {
        scale_out[row] = sc;
        zero_out[row] = ze;
    }
}

hipError_t mse_search_launch(const void* x, void* scale, void* zero, const MsGeom& G, hipStream_t st) {
    g_last_variant = G.bits == 4 ? "mse_search_w4" : "mse_search_w3";
    const dim3 grid((unsigned)ms_blocks(G)), block(MS_THREADS);
    if (G.bits == 4)
        hipLaunchKernelGGL(mse_search_kernel<4>, grid, block, 0, st, (const float*)x, (float*)scale, (float*)zero, G);
    else
        hipLaunchKernelGGL(mse_search_kernel<3>, grid, block, 0, st, (const float*)x, (float*)scale, (float*)zero, G);
    return hipGetLastError();
}

}  // namespace qeft
