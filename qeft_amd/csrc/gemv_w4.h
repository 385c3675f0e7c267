// Host side of the round-1 decode GEMV at 4 and 3 bits (gemv_w4.hip): a PLAN -- a pure function of the
// kind of call, the bit width, the shape and the overrides that says which kernel instance runs, with what grid, LDS and row
// slices, or with which error the call is refused -- and two launchers that compute the plan and execute it.
#pragma once

#include <hip/hip_runtime.h>

#include "qeft_common.h"      // GemvArgs, GemvGroupArgs

namespace qeft {

// rows: the fused / plain / qeft entries (m rows of x); small-M: the GEMM entry's route (16 rows per weight pass);
// group: up to three linears on one x, batch 1, optional RMSNorm staging; silu: x := silu(gate) * up staged, batch 1
enum GemvKind { kGemvRows = 0, kGemvSmallM, kGemvGroup, kGemvSilu };

// one id per name qeft_last_variant can report from gemv_w4.hip (gemv_w4_variant); kGemvNone: nothing is launched
enum GemvVariant {
    kGemvNone = 0,
    kGemvValu, kGemvValuGroup, kGemvValuSilu, kGemvMfma, kGemvMfmaGroup, kGemvMfmaSilu, kGemvMfmaSmallM,      // (family, then + kind)
    kGemvW3, kGemvW3Rows, kGemvW3Group, kGemvW3Silu,
    kGemvVariantCount
};
const char* gemv_w4_variant(int variant);

// The lab switches.  gemv_w4_overrides() is the one place that reads them, once per process; both bit widths obey them.
struct GemvOverrides {
    int blocks = 0;     // QEFT_GEMV_BLOCKS  > 0: at most that many blocks for a batch-1 MFMA launch
    int depth = 0;      // QEFT_GEMV_DEPTH   set: MFMA ring depth 6 if it says 6, else 4
};
GemvOverrides gemv_w4_overrides();

// One kernel launch of `rows` batch rows, made `count` times on consecutive row slices.
struct GemvLaunch {
    int count = 0, rows = 0;
    int M = 0;                          // template selector M: 1..7 fixed rows, 16 the run-time-M instance (m_rt = rows)
    int grid = 0, lds = 0, rs_cap = 0;  // blocks, dynamic LDS bytes, row sets a block's LDS is carved for (MFMA)
};
struct GemvPlan {
    hipError_t rc = hipSuccess;         // hipErrorNotSupported / hipErrorInvalidValue: refused, nothing else is set
    int variant = kGemvNone;
    bool mfma = false;                  // family: gemv_w4_mfma.h or the VALU kernels of gemv_w4_kernel.h
    int bits = 4, D = 0, rgi = 0;       // template selectors BITS, D, RGI (VALU),
    bool outl = false, xg = false;      //   OUTL, XG
    int xt = 0;                         //   XT: 0 plain, 1 RMSNorm staging (group), 2 SiLU * up staging (silu)
    int threads = 0;
    int blk_end[3] = {0, 0, 0};         // group: the parts' cumulative block counts
    GemvLaunch body, tail;              // the m rows: body.count launches of body.rows, then tail.count (0 or 1) of tail.rows
};
// N[nparts]: the rows of the layer (nparts == 1) or of the group's parts; gather: x through reorder_ids (rows); xt_aux: the
// group's RMSNorm gamma.  m is 1 for group and silu.
GemvPlan gemv_w4_plan(int kind, int bits, int m, int nparts, const int* N, int K, int G, int n_out, bool gather, bool xt_aux,
                      const GemvOverrides& ov);

// y[m, N] = x[m, K] . W^T (+ bias, + residual) for kind rows, small-M or silu (m == 1: a.x is the gate, a.xt_aux is up)
hipError_t gemv_w4_launch(int kind, int bits, const GemvArgs& a, int m, hipStream_t st);
hipError_t gemv_w4_group_launch(int bits, GemvGroupArgs g, int nparts, hipStream_t st);
// 3-bit stream -> 4-bit checkpoint layout, for the GEMM kernels
hipError_t expand_w3_launch(const void* q3, void* q4, int N, int K, int n_out, hipStream_t st);

}  // namespace qeft
