// What the attention kernels over an e4m3 KV cache share (decode_attn_kv8.hip: one row per slot; decode_verify_kv8.hip: m rows of
// one sequence): the cache recipe of include/qeft_hip.h for one row, the registers of one 16-position run in flight, and the host
// side of both launches (chunk rule, R, LDS bytes, dispatch).  The two kernels are one algorithm (the one-row kernel is the m-row
// kernel at m = 1 in a slot of its own) but stay written out, so a fix to one (masking constants, the merge factor of an empty
// split, the counter re-arm) belongs in both, and in the fp16 pair.  Shared device code was built in four cuts and taken back: the
// whole core cost the one-row kernel 17 % (m a compile-time 1) or 0.3 - 3.7 % (m a runtime value); the merges alone left the run
// loop the same instruction for instruction but moved it within its 64-byte fetch lines, which by itself costs up to 2 %
// (profiles/kv8_attn_core_refactor.log, sections A - D).
#pragma once
#include <type_traits>
#include "qeft_common.h"
#include "decode_attn.h"      // wave_max
#include "decode_rows.h"      // AttnRowsArgs

namespace qeft {

typedef float fx2 __attribute__((ext_vector_type(2)));

// ---- one row of 128 fp16 values by one wave (all 64 lanes active): the lane holds elements `lane` (a) and `lane + 64` (b) as
// fp32; returns their codes and the row's scale.  amax == 0: scale 0, codes 0.
__device__ __forceinline__ void kv8_quant_row(float a, float b, uint8_t& ca, uint8_t& cb, float& scale) {
    const float amax = wave_max(fmaxf(fabsf(a), fabsf(b)));
    scale = 0.f;
    ca = cb = 0;
    if (amax > 0.f) {
        const float inv = 448.0f / amax;              // correctly rounded divides (no fast-math in this build)
        scale = amax / 448.0f;
        const float x = fminf(fmaxf(a * inv, -448.0f), 448.0f), y = fminf(fmaxf(b * inv, -448.0f), 448.0f);
        const int pk = __builtin_amdgcn_cvt_pk_fp8_f32(x, y, 0, false);      // v_cvt_pk_fp8_f32: OCP e4m3fn, round to nearest even
        ca = (uint8_t)(pk & 0xff);
        cb = (uint8_t)((pk >> 8) & 0xff);
    }
}

// ---- one run of 16 cache rows as a wave holds it: score role (lane = position lane / 4, quarter lane % 4) two 16-byte K loads
// and the position's two scales; P.V role (lane = position class lane / 16, dim group lane % 16) four 8-byte V loads.
struct Kv8Run {
    u32x4 k[2];
    u32x2 v[4];
    float ks, vs;
};

// ---- host side of both launches
// Query rows per block (heads of a chunk x m; m = 1 for the one-row kernel).  Measured on the 64/8 layout against a 16-row block
// of the same role (302 VGPRs, one block per CU): 8 rows are 1.7 - 2.4 x faster at m = 4 and 8 at every context and split
// (DESIGN.md §4.11 has the lines), although the chunks of a kv head each re-read its runs.
constexpr int kAttnKv8Rows = 8;
// heads of a chunk: the largest divisor of the group with hc * m <= kAttnKv8Rows
inline int kv8_attn_chunk(int grp, int m) {
    int hc = 1;
    for (int d = 1; d <= grp; ++d)
        if (grp % d == 0 && d * m <= kAttnKv8Rows) hc = d;
    return hc;
}

// dynamic LDS of a block compiled for R query rows with MN new-row slots (1: one-row kernel, 8: m-row kernel); at most 24896 bytes.
// The scale area keeps the exp weights behind it 16-byte aligned (4 floats for MN = 1).
template <int MN>
constexpr size_t kv8_attn_smem_bytes(int R) {
    return (size_t)R * 128 * 2 + 2 * MN * 128 + (MN == 1 ? 4 : 2 * MN) * 4 + 2 * 4 * R * 16 * 4 + 4 * R * 128 * 4 + 2 * 4 * R * 4;
}

// go(std::integral_constant<int, R>) with the smallest R of 1, 2, 4, 8 that holds `rows`; more than kAttnKv8Rows rows are refused
template <class Go>
hipError_t kv8_attn_dispatch(int rows, Go go) {
    if (rows < 1 || rows > kAttnKv8Rows) return hipErrorInvalidValue;
    if (rows <= 1) return go(std::integral_constant<int, 1>());
    if (rows <= 2) return go(std::integral_constant<int, 2>());
    if (rows <= 4) return go(std::integral_constant<int, 4>());
    return go(std::integral_constant<int, 8>());
}

// decode_attn_kv8.hip (one row per slot), decode_verify_kv8.hip (m rows of one sequence; its workspace is attn_m_workspace_bytes)
size_t attn_kv8_workspace_bytes(int n_heads, int S, int m);
hipError_t rope_attn_kv8_launch(const AttnRowsArgs& a, hipStream_t st);
hipError_t rope_attn_m_kv8_launch(const AttnRowsArgs& a, hipStream_t st);
hipError_t kv8_store_rows_launch(const void* k, const void* v, int row_stride, void* kc, void* vc, void* ks, void* vs, int n_kv,
                                 int max_seq, int p0, int T, hipStream_t st);

}  // namespace qeft
