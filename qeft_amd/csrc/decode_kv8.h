// What the attention kernels over an e4m3 KV cache share (decode_attn_kv8.hip: one row per slot; decode_verify_kv8.hip: m rows of
// one sequence): the cache recipe of include/qeft_hip.h for one row, and the registers of one 16-position run in flight.
#pragma once
#include "qeft_common.h"
#include "decode_attn.h"      // wave_max

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

}  // namespace qeft
