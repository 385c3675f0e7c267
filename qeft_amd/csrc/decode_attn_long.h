// One-token attention for long caches (decode_attn_long.hip): host-side geometry and launcher.
#pragma once
#include "qeft_common.h"

namespace qeft {

constexpr int kAttnLongMaxSeq = 1 << 20;    // cache rows: every offset of a kv head's cache stays far below 2^31 elements
constexpr int kAttnLongMaxSplit = 64;
constexpr int kAttnLongStep = 128;          // keys of a block step (4 waves x 32): a split's range is a multiple of it

// S in {1, 2, 4, .., 64}, max_seq % 16 == 0 in [16, 2^20], n_heads a multiple of n_kv
inline bool attn_long_shape_ok(int n_heads, int n_kv, int S, int max_seq) {
    return n_heads >= 1 && n_heads <= 4096 && n_kv >= 1 && n_heads % n_kv == 0 && S >= 1 && S <= kAttnLongMaxSplit && (S & (S - 1)) == 0 &&
           max_seq >= 16 && max_seq % 16 == 0 && max_seq <= kAttnLongMaxSeq;
}

// bytes of the workspace for S > 1: the arrival counters (attn_ctr_floats, decode_attn.h), then one kAttnRec record per (head, split)
size_t attn_long_workspace_bytes(int n_heads, int S);
hipError_t rope_attn_decode_long_launch(const void* q, const void* k, const void* v, const void* cs, const void* sn, void* kc, void* vc,
                                        const int* pos, const int* out_pos, void* out, void* ws, int n_heads, int n_kv, int max_seq, int S,
                                        int tab_rows, hipStream_t st);

}  // namespace qeft
