// The v3 decode GEMV on m = 2..8 batch rows WITH the decode engine's fused epilogues (gemv_v3.h, MB = 2, FL = false): the
// linears of the verify pass (DecodeEngine.verify), which scores m tokens of one sequence per weight pass.  The batch rows are
// the A rows of the same MFMAs, so the weights stream once for all m rows.  Modes: PLAIN with ssq_in (q|k|v), PLAIN with the
// fp32 residual and gamma_out / ssq_out (o_proj, down_proj), PAIR (gate|up, silu(gate) * up).  x rows sit in LDS where m K
// fits, and come from global memory (the XG form) where it does not: K = 11008 at m >= 5.
// Row layouts: x [m][K], y [m][N] (PAIR: [m][N/2]), residual / y32 [m][N], ssq_in [m][n_ssq_in], ynorm [m][N],
// ssq_out [m][blocks of the launch] (qeft_decode_linear_blocks(N): the same count as the one-row launch).
#include "gemv_v3.h"

namespace qeft {

static int cdiv(int a, int b) { return (a + b - 1) / b; }

// Geometry of an m-row engine launch: the one-row launch's blocks and row sets, 8 waves, x in LDS unless it does not fit.
bool gemv_v3_multi_plan(V3Args& a, size_t& smem) {
    const int nblk = gemv_v3_blocks(a.g.nsets);
    a.nblk = nblk;
    a.rs_cap = cdiv(a.g.nsets, nblk);
    a.sets_q = a.g.nsets / nblk;
    a.sets_r = a.g.nsets % nblk;
    a.nw = V3_NW;
    a.xg = false;
    smem = v3_lds(a.g.K, a.g.ngroups, a.g.n_out, a.rs_cap, a.m, V3_NW, false, false, false, false).total;
    if (smem > 160 * 1024) {
        a.xg = true;
        smem = v3_lds(a.g.K, a.g.ngroups, a.g.n_out, a.rs_cap, a.m, V3_NW, false, false, false, true).total;
    }
    return smem <= 160 * 1024 && nblk < 65536;
}

template <int D, bool OUTL, int MODE, int RSC, bool XG>
static hipError_t go_multi(const V3Args& a, size_t smem, hipStream_t st) {
    auto kern = gemv_v3_kernel<8, D, OUTL, MODE, 4, 2, RSC, false, XG>;
    if (smem > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(a.nblk), dim3(8 * 64), smem, st, V3_KERNEL_ARGS(a));
    return hipGetLastError();
}

template <bool OUTL, int MODE, int RSC>
static hipError_t launch_multi_r(const V3Args& a, size_t smem, int depth, hipStream_t st) {
    constexpr int DD = RSC >= 3 ? 6 : 4;        // the deep ring of gemv_v3_dispatch.h
    if (a.xg) return go_multi<DD, OUTL, MODE, RSC, true>(a, smem, st);
    return depth >= 4 ? go_multi<DD, OUTL, MODE, RSC, false>(a, smem, st) : go_multi<2, OUTL, MODE, RSC, false>(a, smem, st);
}

template <bool OUTL, int MODE>
static hipError_t launch_multi_m(const V3Args& a, size_t smem, int depth, hipStream_t st) {
    switch (a.rs_cap) {
        case 1: return launch_multi_r<OUTL, MODE, 1>(a, smem, depth, st);
        case 2: return launch_multi_r<OUTL, MODE, 2>(a, smem, depth, st);
        case 3: return launch_multi_r<OUTL, MODE, 3>(a, smem, depth, st);
        case 4: return launch_multi_r<OUTL, MODE, 4>(a, smem, depth, st);
    }
    return hipErrorInvalidValue;
}

// a: packed operands (szp, plain oweight), m = 2..8, no per-channel scales / xn / gather (the launch carries no run-time flag)
hipError_t gemv_v3_multi_launch(V3Args a, int mode, hipStream_t st) {
    if (a.m < 2 || a.m > 8 || !a.szp || a.xn_gamma || a.ids || a.bits == 3) return hipErrorInvalidValue;
    if (a.g.ngroups == 1 && a.g.K > 128) return hipErrorInvalidValue;        // per-channel scales: a flag path
    if (a.g.n_out > 0 && !a.ow) return hipErrorInvalidValue;
    size_t smem;
    if (!gemv_v3_multi_plan(a, smem)) return hipErrorInvalidValue;
    // ring depth as the batch-row launches of gemv_v3_launch: 4 / 6 loads per wave where a CU holds one block with >= 8 loads
    const int loads_per_wave = cdiv(a.g.nfull, V3_NW) * a.rs_cap;
    const int depth = a.xg ? 4 : (a.nblk <= 256 && loads_per_wave >= 8 ? 4 : 2);
    g_last_variant = a.xg ? "gemv_v3_multi_xg" : mode == V3_MODE_PAIR ? "gemv_v3_multi_pair" : "gemv_v3_multi";
    if (mode == V3_MODE_PAIR)
        return a.g.n_out > 0 ? launch_multi_m<true, V3_MODE_PAIR>(a, smem, depth, st) : launch_multi_m<false, V3_MODE_PAIR>(a, smem, depth, st);
    return a.g.n_out > 0 ? launch_multi_m<true, V3_MODE_PLAIN>(a, smem, depth, st) : launch_multi_m<false, V3_MODE_PLAIN>(a, smem, depth, st);
}

// Host-side enumeration of every address an m-row engine launch forms beyond those of the one-row launch (which
// gemv_v3_count_out_of_range walks): the m x rows (LDS pieces, or the XG lanes' global fragments) and their LDS destinations,
// and the per-row epilogue operands: residual / y32 / ynorm [m][N], gamma_out [N], ssq_in [m][n_ssq_in], ssq_out [m][nblk],
// y [m][N] or [m][N/2].  n_rows_have: rows the operands really hold (< N: the negative control).
long long gemv_v3_count_out_of_range_multi(const V3Geom& G, int n_rows_have, int m, int mode, int n_ssq_in) {
    long long bad = 0;
    V3Args a{};
    a.g = G;
    a.m = m;
    size_t smem;
    if (!gemv_v3_multi_plan(a, smem)) return 1;
    const int N = G.nsets * 16, nblk = a.nblk;
    const size_t x_bytes = (size_t)m * G.K * 2, rows_f32 = (size_t)m * n_rows_have * 4, rows_f16 = (size_t)m * n_rows_have * 2;
    const V3Lds L = v3_lds(G.K, G.ngroups, G.n_out, a.rs_cap, m, V3_NW, false, false, false, a.xg);
    const int XB = v3_x_bytes(G.K), XS = v3_x_stride(G.K, m);
    for (int lane = 0; lane < 64; ++lane) {
        const int nl = lane & 15, kc = lane >> 4, row = nl < m - 1 ? nl : m - 1;
        if (a.xg) {
            for (int step = 0; step < G.nsteps; ++step) bad += (size_t)row * G.K * 2 + (size_t)step * 256 + kc * 64 + 64 > x_bytes;
        } else {
            for (int i = 0; i < m; ++i)
                for (int p = 0; p < (XB >> 10); ++p) {
                    bad += (size_t)i * G.K * 2 + v3_x_off(G, p, lane) + 16 > x_bytes;
                    bad += L.xs + (uint32_t)i * XS + ((uint32_t)p << 10) + lane * 16 + 16 > L.szl;
                }
            // the lanes' A-fragment reads: row (clamped), 64 bytes of every step
            bad += (size_t)row * XS + (size_t)(G.nsteps - 1) * 256 + kc * 64 + 64 > L.szl;
        }
    }
    // the partial sums of every (row set, wave, batch row) inside the red region
    bad += (size_t)((a.rs_cap - 1) * V3_NW + V3_NW - 1) * 8 * 16 * 4 + (size_t)7 * 16 * 4 + 16 * 4 > v3_red_bytes(a.rs_cap, m, V3_NW);
    for (int b = 0; b < nblk; ++b) {
        int set0, RS;
        v3_block_sets(v3_xcd_block(b, nblk), G.nsets / nblk, G.nsets % nblk, set0, RS);
        if (RS < 1 || RS > V3_MAX_RS || set0 < 0 || set0 + RS > G.nsets) { ++bad; continue; }
        for (int i = 0; i < m; ++i)
            for (int lane = 0; lane < 64; ++lane) {
                if (mode == V3_MODE_PAIR) {
                    if (lane < RS * 8) bad += (size_t)i * (N / 2) + (set0 + (lane >> 3)) * 8 + (lane & 7) >= (size_t)m * (n_rows_have / 2);
                    continue;
                }
                if (lane < RS * 16) {
                    const size_t row = (size_t)set0 * 16 + lane;
                    bad += ((size_t)i * N + row) * 4 + 4 > rows_f32;         // residual / y32
                    bad += ((size_t)i * N + row) * 2 + 2 > rows_f16;         // y or ynorm
                    bad += row >= (size_t)n_rows_have;                        // gamma_out
                }
                if (n_ssq_in > 0)
                    for (int e = 0; e < 4; ++e) {
                        const int b0 = 4 * lane + e, b1 = 256 + 4 * lane + e;
                        if (b0 < n_ssq_in) bad += (size_t)i * n_ssq_in + b0 >= (size_t)m * n_ssq_in;
                        if (b1 < n_ssq_in) bad += (size_t)i * n_ssq_in + b1 >= (size_t)m * n_ssq_in;
                    }
            }
        for (int i = 0; i < m; ++i) bad += (size_t)i * nblk + b >= (size_t)m * gemv_v3_blocks(n_rows_have / 16);      // ssq_out, sized by the caller's N
    }
    return bad;
}

}  // namespace qeft
