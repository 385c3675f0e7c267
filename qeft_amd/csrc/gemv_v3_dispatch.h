// Kernel instantiation and dispatch of the v3 decode GEMV, shared by its three translation units, one per family of instances:
// gemv_v3.hip (V3_FAM_FLAGGED, FL = true: launches that carry run-time flags -- the reference's entry points, the consumer-side
// norm, per-channel scales, several batch rows), gemv_v3_plain.hip (V3_FAM_PLAIN, FL = false: the decode engine's one-row launches)
// and gemv_v3_multi.hip (V3_FAM_ENGINE_M: the engine's m-row launches, MB = 2 without the flag paths).  Three files so that hipcc
// builds the families in parallel; each instantiates launch_b with its own family only.
#pragma once
#include "gemv_v3.h"

namespace qeft {

// the FL = false half (gemv_v3_plain.hip), called by gemv_v3_launch
hipError_t gemv_v3_dispatch_plain(const V3Args& a, const V3Plan& p, hipStream_t st);

enum V3Family { V3_FAM_PLAIN, V3_FAM_FLAGGED, V3_FAM_ENGINE_M };

// Instantiations.  8 waves per block (the 16-wave form of round 2 lost to it on every launch kind once the step loop had its row
// sets at compile time, profiles/r03_gemv_lab.txt): ring depth 2 for every RSC, 4 for RSC <= 2, 6 for RSC >= 3.  4 waves per
// block with ring depth 4 for launches of more than 256 blocks (several blocks per CU: gate|up 10.47 vs 10.76 us).  12 waves, ring
// depth 2, for one-set launches with a long K (round 4: down_proj 7.44 -> 7.31 us, profiles/r04_gemv_lab.txt).  The engine's m-row
// family holds the 8-wave forms only: ring 2 and the deep ring x outliers x PLAIN / PAIR x RSC 1..4, xg on the deep ring (48).
// Nothing is decided here: each function maps fields of the plan (gemv_v3_plan) to template arguments, and a plan that names an
// instance the build does not hold is an error.

// Compile-time K (gemv_v3.h: KCT).  The decode engine launches each kind of linear with one K for the life of the model, so the
// instances its Llama-2-7B and -13B launches run are built a second time with that K as a template argument: flag-free half, one
// batch row, 4 bits, with the outlier step.  The table is the whole choice: v3_ctk_pick (called by gemv_v3_plan, and by nobody
// else) looks a plan up in it, and launch_dmr instantiates exactly its rows.  Any other shape -- another K, another grid and so
// another (waves, ring, row sets) -- runs the run-time instance; QEFT_GEMV_CTK=0 sends every launch there (A/B).
struct V3CtkRow {
    int nw, D, rs_cap, mode, K;
};
constexpr V3CtkRow V3_CTK[] = {
    {8, 6, 3, V3_MODE_PLAIN, 4096},     // 7B  q|k|v     12288 x 4096: 256 blocks of three sets
    {4, 4, 3, V3_MODE_PAIR, 4096},      //     gate|up   22016 x 4096: 459 blocks of three
    {8, 2, 1, V3_MODE_PLAIN, 4096},     //     o_proj     4096 x 4096: 256 blocks of one
    {12, 2, 1, V3_MODE_PLAIN, 11008},   //     down       4096 x 11008
    {8, 6, 4, V3_MODE_PLAIN, 5120},     // 13B q|k|v     15360 x 5120: 240 blocks of four
    {4, 4, 4, V3_MODE_PAIR, 5120},      //     gate|up   27648 x 5120: 432 blocks of four
    {8, 4, 2, V3_MODE_PLAIN, 5120},     //     o_proj     5120 x 5120: 160 blocks of two
    {8, 4, 2, V3_MODE_PLAIN, 13824},    //     down       5120 x 13824
};
constexpr int V3_CTK_ROWS = (int)(sizeof(V3_CTK) / sizeof(V3_CTK[0]));
// the K to compile in for this plan and this K, or 0 (the run-time instance)
inline int v3_ctk_pick(const V3Plan& p, int K, bool enabled) {
    if (!enabled || p.fl || p.mb != 1 || p.bits != 4 || !p.outl || p.xg) return 0;
    for (const V3CtkRow& r : V3_CTK)
        if (r.nw == p.nw && r.D == p.D && r.rs_cap == p.rs_cap && r.mode == p.mode && r.K == K) return K;
    return 0;
}

// launch_dmr's search of the table: row I and the rest
template <int NW, int D, int RSC, int I, typename GO>
static hipError_t launch_ctk(const V3Plan& p, GO&& go) {
    if constexpr (I < V3_CTK_ROWS) {
        constexpr V3CtkRow R = V3_CTK[I];
        if constexpr (R.nw == NW && R.D == D && R.rs_cap == RSC) {
            if (p.kct == R.K && p.mode == R.mode) return go(gemv_v3_kernel<NW, D, true, R.mode, 4, 1, RSC, false, false, R.K>);
        }
        return launch_ctk<NW, D, RSC, I + 1>(p, go);
    } else {
        return hipErrorInvalidValue;        // a plan that names an instance the build does not hold
    }
}

// launch_dmr's engine-m family: m = 2..8 rows with the engine's epilogues, PLAIN or PAIR; no flag path, no compile-time K
template <int NW, int D, bool OUTL, int BITS, int RSC, typename GO>
static hipError_t launch_em(const V3Plan& p, GO&& go) {
    if constexpr (NW == 8 && BITS == 4) {
        if (p.mb != 2 || p.fl || p.kct != 0) return hipErrorInvalidValue;
        if constexpr (D >= 4) {
            if (p.xg)       // x read from global memory
                return p.mode == V3_MODE_PAIR ? go(gemv_v3_kernel<8, D, OUTL, V3_MODE_PAIR, 4, 2, RSC, false, true>) : go(gemv_v3_kernel<8, D, OUTL, V3_MODE_PLAIN, 4, 2, RSC, false, true>);
        }
        if (p.xg) return hipErrorInvalidValue;
        return p.mode == V3_MODE_PAIR ? go(gemv_v3_kernel<8, D, OUTL, V3_MODE_PAIR, 4, 2, RSC, false>) : go(gemv_v3_kernel<8, D, OUTL, V3_MODE_PLAIN, 4, 2, RSC, false>);
    }
    return hipErrorInvalidValue;
}

template <int NW, int D, bool OUTL, int BITS, int RSC, V3Family FAM>
static hipError_t launch_dmr(const V3Args& a, const V3Plan& p, hipStream_t st) {
    constexpr bool FL = FAM == V3_FAM_FLAGGED;
    auto go = [&](auto kern) -> hipError_t {
        if (p.smem > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.smem);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, dim3(p.nblk), dim3(NW * 64), p.smem, st, V3_KERNEL_ARGS(a));
        return hipGetLastError();
    };
    if constexpr (FAM == V3_FAM_ENGINE_M) {
        return launch_em<NW, D, OUTL, BITS, RSC>(p, go);
    } else {
        if (p.kct != 0) {
            if constexpr (!FL && BITS == 4 && OUTL) return launch_ctk<NW, D, RSC, 0>(p, go);
            return hipErrorInvalidValue;
        }
        if constexpr (NW == 8 && BITS == 4 && FL) {       // several batch rows (the reference's gemv entries, m = 2..7; 8..16 from the GEMM entries): plain launches
            if constexpr (D >= 4) {
                if (p.mb > 1 && p.xg) return go(gemv_v3_kernel<8, D, OUTL, V3_MODE_PLAIN, 4, 2, RSC, true, true>);     // x read from global memory
            }
            if (p.mb > 1 && p.xg) return hipErrorInvalidValue;
            if (p.mb > 1) return go(gemv_v3_kernel<8, D, OUTL, V3_MODE_PLAIN, 4, 2, RSC, true>);
        }
        if (p.mb > 1) return hipErrorInvalidValue;
        return p.mode == V3_MODE_PAIR ? go(gemv_v3_kernel<NW, D, OUTL, V3_MODE_PAIR, BITS, 1, RSC, FL>) : go(gemv_v3_kernel<NW, D, OUTL, V3_MODE_PLAIN, BITS, 1, RSC, FL>);
    }
}

template <bool OUTL, int BITS, V3Family FAM>
static hipError_t launch_d(const V3Args& a, const V3Plan& p, hipStream_t st) {
    if (p.nw == 4) {
        if (p.D != 4) return hipErrorInvalidValue;
        switch (p.rs_cap) {
            case 1: return launch_dmr<4, 4, OUTL, BITS, 1, FAM>(a, p, st);
            case 2: return launch_dmr<4, 4, OUTL, BITS, 2, FAM>(a, p, st);
            case 3: return launch_dmr<4, 4, OUTL, BITS, 3, FAM>(a, p, st);
            case 4: return launch_dmr<4, 4, OUTL, BITS, 4, FAM>(a, p, st);
        }
        return hipErrorInvalidValue;
    }
    if (p.nw == 12) {             // long one-set launches (down_proj: 85 full steps = 8 / 7 per wave instead of 11 / 10)
        if (p.rs_cap == 1 && p.D == 2) return launch_dmr<12, 2, OUTL, BITS, 1, FAM>(a, p, st);
        return hipErrorInvalidValue;
    }
    const bool deep = p.D != 2;       // the deep ring of the block's RSC: 4 loads, 6 with three or four row sets
    if (p.nw != 8 || (deep && p.D != (p.rs_cap >= 3 ? 6 : 4))) return hipErrorInvalidValue;
    switch (p.rs_cap) {           // row sets per block: a compile-time constant of the kernel
        case 1: return deep ? launch_dmr<8, 4, OUTL, BITS, 1, FAM>(a, p, st) : launch_dmr<8, 2, OUTL, BITS, 1, FAM>(a, p, st);
        case 2: return deep ? launch_dmr<8, 4, OUTL, BITS, 2, FAM>(a, p, st) : launch_dmr<8, 2, OUTL, BITS, 2, FAM>(a, p, st);
        case 3: return deep ? launch_dmr<8, 6, OUTL, BITS, 3, FAM>(a, p, st) : launch_dmr<8, 2, OUTL, BITS, 3, FAM>(a, p, st);
        case 4: return deep ? launch_dmr<8, 6, OUTL, BITS, 4, FAM>(a, p, st) : launch_dmr<8, 2, OUTL, BITS, 4, FAM>(a, p, st);
    }
    return hipErrorInvalidValue;
}

template <int BITS, V3Family FAM>
static hipError_t launch_b(const V3Args& a, const V3Plan& p, hipStream_t st) {
    return p.outl ? launch_d<true, BITS, FAM>(a, p, st) : launch_d<false, BITS, FAM>(a, p, st);
}

}  // namespace qeft
