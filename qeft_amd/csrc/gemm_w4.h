// Host side of the GEMM forward, dX and d(oweight) (gemm_w4.hip): for each of the three a PLAN -- a pure
// function of the shape, the bit width, the gate kind, the workspace size and the overrides that says which tier takes the launch
// and with what grid, block and LDS -- and a launcher that computes the plan and executes it.  The support queries of the C ABI
// ask the same predicates, so what an entry calls supported is what its launcher takes.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

namespace qeft {

// one id per name qeft_last_variant can report from gemm_w4.hip (gemm_tier_variant); kTierNone: the shape is not supported
enum GemmTier {
    kTierNone = 0,
    kFwdV1, kFwdV2, kFwdV2SplitK, kFwdV2x256,
    kFwdV3x128, kFwdV3x128SplitK, kFwdV3x256, kFwdV3x256Silu, kFwdV3x256SiluPair, kFwdV3x128W3, kFwdV3x256W3,
    kDx64, kDx64Split, kDx128, kDx128V3, kDx256, kDx128V3W3, kDx256W3,
    kDowFma, kDowMfma, kDowMfmaN64,
    kTierCount
};
const char* gemm_tier_variant(int tier);

// silu(gate) * y in the epilogue: no gate, a gate tensor [M, N], or the gate|up halves of one paired launch (kSiluPair64)
enum GemmGate { kGateNone = 0, kGateTensor = 1, kGatePair = 2 };
// silu_gate == kSiluPair64: the paired-halves epilogue (EPI 2) instead of an external gate tensor
extern const void* const kSiluPair64;

// The environment overrides (A/B switches of the tiers).  gemm_overrides() reads QEFT_GEMM_V3, _V3M, _V3S, _NWV, QEFT_DX_V3,
// QEFT_DOW_BN and (lab builds) QEFT_GEMM_ABL once per process and QEFT_GEMM_V1 on every call.
struct GemmOverrides {
    int v3 = -1;        // QEFT_GEMM_V3   0 / 1: never / always the 256-row loader-wave tier where ok3 admits it
    int v3m = -1;       // QEFT_GEMM_V3M  0 / 1: never / always the 128-row loader-wave tier
    int v3s = -1;       // QEFT_GEMM_V3S  0: no split-K on the 128-row loader-wave tier
    int nwv = 0;        // QEFT_GEMM_NWV  4 / 8: the v2 kernel's waves per block
    int dx_v3 = -1;     // QEFT_DX_V3     0 / 1: never the loader-wave dX tiles / always the 256-row one
    int dow_bn = 0;     // QEFT_DOW_BN    32 / 64: columns of dy per d(oweight) block
    int abl = 0;        // QEFT_GEMM_ABL  1 .. 6: ablation of the 256-row kernel (honoured by QEFT_LAB builds only)
    bool v1 = false;    // QEFT_GEMM_V1   set: gemm_v1 instead of the v2 kernels
};
GemmOverrides gemm_overrides();

// Everything a launch needs.  n_out is the outlier width in effect throughout (0 without an oweight tensor).
struct GemmPlan {
    int tier = kTierNone;
    bool outl = false;                  // template selectors: OUTL,
    int abl = 0, epi = 0, tile = 0;     //   ABL, EPI, and MT (forward / dX loader-wave kernels), NWV (v2) or BN (d(oweight) MFMA kernel),
    int bits = 4;                       //   BITS
    unsigned gx = 1, gy = 1, gz = 1;    // grid
    int threads = 0, lds = 0;           // block, dynamic LDS bytes
    int S = 1;                          // split factor; S > 1: fp32 partials in the workspace, gemm_splitk_reduce_kernel follows
    bool fused = false;                 // silu(gate) * y formed in the kernel's own epilogue
    bool supported() const { return tier != kTierNone; }
    bool reduce() const { return S > 1; }
};
// workspace_bytes == 0: no workspace
GemmPlan gemm_w4_plan(int M, int N, int K, int G, int n_out, int bits, int gate, size_t workspace_bytes, const GemmOverrides& ov);
GemmPlan gemm_w4_dx_plan(int M, int N, int K, int G, int n_out, int bits, size_t workspace_bytes, const GemmOverrides& ov);
GemmPlan grad_oweight_plan(int N, int K, int n_out, const GemmOverrides& ov);

hipError_t gemm_w4_launch(const void* x, const void* qw, const void* scales, const void* zeros, const void* ow,
                          const void* bias, void* y, int M, int N, int K, int G, int n_out, hipStream_t st,
                          void* workspace = nullptr, size_t workspace_bytes = 0, const void* silu_gate = nullptr,
                          bool* fused_epilogue = nullptr, int bits = 4);
hipError_t gemm_w4_dx_launch(const void* dy, const void* qw, const void* scales, const void* zeros, const void* ow,
                             void* dx, int M, int N, int K, int G, int n_out, hipStream_t st, void* workspace = nullptr,
                             size_t workspace_bytes = 0, int bits = 4);
hipError_t grad_oweight_launch(const void* dy, const void* x, void* dow, int M, int N, int K, int n_out,
                               hipStream_t st);

// queries the C ABI answers with (the plans call the same functions)
bool gemm_w4_pair64_ok(int M, int n2, int K, int G, int n_out);
int gemm_w3_native_tile(int M, int N, int K, int G, int n_out);
bool gemm_w3_dx_native(int M, int N, int K, int G, int n_out);
int gemm_w4_split(int M, int N, int K, int n_out);
int gemm_v3_split(int M, int N, int K, int n_out);
int gemm_w4_dx_split(int M, int N, int K);
bool gemm_dx128_takes(int M, int K);

}  // namespace qeft
