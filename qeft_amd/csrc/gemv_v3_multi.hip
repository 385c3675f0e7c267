// The v3 decode GEMV on m = 2..8 batch rows WITH the decode engine's fused epilogues (gemv_v3.h, MB = 2, FL = false): the
// linears of the verify pass (DecodeEngine.verify), which scores m tokens of one sequence per weight pass.  The batch rows are
// the A rows of the same MFMAs, so the weights stream once for all m rows.  Modes: PLAIN with ssq_in (q|k|v), PLAIN with the
// fp32 residual and gamma_out / ssq_out (o_proj, down_proj), PAIR (gate|up, silu(gate) * up).  x rows sit in LDS where m K
// fits, and come from global memory (the XG form) where it does not: K = 11008 at m >= 5.
// Row layouts: x [m][K], y [m][N] (PAIR: [m][N/2]), residual / y32 [m][N], ssq_in [m][n_ssq_in], ynorm [m][N],
// ssq_out [m][blocks of the launch] (qeft_decode_linear_blocks(N): the same count as the one-row launch).
// What a launch runs is gemv_v3_plan's answer under V3_PLAN_ENGINE_M (gemv_v3.hip), and gemv_v3_dispatch.h launches it: this file
// holds the family's 48 instances gemv_v3_kernel<8, D, OUTL, MODE, 4, 2, RSC, false, XG> and nothing that decides.
#include "gemv_v3_dispatch.h"

namespace qeft {

// The plan of an m-row engine launch: x in LDS unless it does not fit
static V3Plan engine_m_plan(const V3Geom& g, int m, int mode, int bits, uint32_t flags) {
    const V3Plan p = gemv_v3_plan(g, m, mode, bits, flags | V3_PLAN_ENGINE_M);
    return p.ok ? p : gemv_v3_plan(g, m, mode, bits, flags | V3_PLAN_ENGINE_M | V3_PLAN_XG);
}

// a: packed operands (szp, plain oweight), m = 2..8, no per-channel scales / xn / gather (the launch carries no run-time flag)
hipError_t gemv_v3_multi_launch(V3Args a, int mode, hipStream_t st) {
    const V3Plan p = engine_m_plan(a.g, a.m, mode, a.bits, v3_plan_flags(a) & ~V3_PLAN_XG);
    if (!p.ok) return hipErrorInvalidValue;
    a.nblk = p.nblk, a.rs_cap = p.rs_cap, a.sets_q = p.sets_q, a.sets_r = p.sets_r, a.nw = p.nw, a.xg = p.xg;
    g_last_variant = p.xg ? "gemv_v3_multi_xg" : mode == V3_MODE_PAIR ? "gemv_v3_multi_pair" : "gemv_v3_multi";
    g_last_plan = p;
    return launch_b<4, V3_FAM_ENGINE_M>(a, p, st);
}

// Host-side enumeration of every address an m-row engine launch forms beyond those of the one-row launch (which
// gemv_v3_count_out_of_range walks): the m x rows (LDS pieces, or the XG lanes' global fragments) and their LDS destinations,
// and the per-row epilogue operands: residual / y32 / ynorm [m][N], gamma_out [N], ssq_in [m][n_ssq_in], ssq_out [m][nblk],
// y [m][N] or [m][N/2].  n_rows_have: rows the operands really hold (< N: the negative control).
long long gemv_v3_count_out_of_range_multi(const V3Geom& G, int n_rows_have, int m, int mode, int n_ssq_in) {
    long long bad = 0;
    const V3Plan pl = engine_m_plan(G, m, mode, 4, 0);
    if (!pl.ok) return 1;
    const int N = G.nsets * 16, nblk = pl.nblk;
    const size_t x_bytes = (size_t)m * G.K * 2, rows_f32 = (size_t)m * n_rows_have * 4, rows_f16 = (size_t)m * n_rows_have * 2;
    const V3Lds L = v3_lds(G.K, G.ngroups, G.n_out, pl.rs_cap, m, V3_NW, false, false, false, pl.xg);
    const int XB = v3_x_bytes(G.K), XS = v3_x_stride(G.K, m);
    for (int lane = 0; lane < 64; ++lane) {
        const int nl = lane & 15, kc = lane >> 4, row = nl < m - 1 ? nl : m - 1;
        if (pl.xg) {
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
    bad += (size_t)((pl.rs_cap - 1) * V3_NW + V3_NW - 1) * 8 * 16 * 4 + (size_t)7 * 16 * 4 + 16 * 4 > v3_red_bytes(pl.rs_cap, m, V3_NW);
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
