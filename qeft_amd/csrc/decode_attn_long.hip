// One-token attention for long caches (qeft_rope_attn_decode_long).
//
// qeft_rope_attn_decode keeps one raw score per cache row in LDS and launches a block per QUERY head; past 32768 rows that table no
// longer fits, and under grouped queries every query head of a group pulls the group's K and V again.  This kernel streams:
//
//   grid    n_kv x S blocks of 256 threads.  A block owns ONE kv head and one contiguous range of its pos + 1 live positions (the
//           ranges are multiples of kAttnLongStep = 128 keys; a range may be empty) and serves all grp = n_heads / n_kv query heads
//           of the group from one pass over K and V.  grp > 16 walks column tiles of 16 heads (one pass per tile).
//   wave    walks its share of the range in tiles of 32 keys (wave w takes tiles w, w + 4, ..) with a running (max, sum, acc[128])
//           per query head -- online softmax, fp32 -- so LDS use does not depend on max_seq and nothing per position is kept.
//   scores  v_mfma_f32_16x16x32_f16, A = 16 K rows (a lane's 8 contiguous halves of a row are ONE 16-byte global load: no LDS hop),
//           B = the rotated, scaled fp16 queries of the tile's 16 heads (zero columns past grp), in registers for the whole pass.
//           The result hands lane (head = lane % 16, g = lane / 16) the keys 4 g .. 4 g + 3 of each 16-key sub-tile.
//   P.V     out^T[d][head] = sum_key V^T[d][key] P^T[key][head] on the same MFMA: B = the lane's 8 probabilities rounded to fp16,
//           straight from the score registers (the k index of an MFMA may be any permutation, as long as A agrees); A = 8 keys of
//           ONE dim, which is a transposed V: the wave stages its 32 V rows in LDS (rows 288 bytes apart: the 4 rows x 32 bytes of
//           each 16-lane group then fall on distinct banks) and reads them back with ds_read_b64_tr_b16.  The accumulator lane
//           (head, g) holds dims 16 dt + 4 g .. + 3: the softmax rescale is one per-lane factor.
//   masks   rows past pos and the tail of the last tile: scores by select to -3e38, P by select to 0, V by select to the token's
//           own v (finite: a stale cache row may hold NaN, and 0 x NaN is NaN on the matrix unit).  Row pos itself comes from the
//           call's operands (k rotated here, v as given), never from the cache.  Every row index is clamped to pos before it
//           becomes an address, whatever the range or the prefetch distance.
//   merge   the block's 4 waves through LDS (the V staging area, reused); S > 1: one kAttnRec record per (query head, split) by
//           write-through stores, one ticket per kv head, the last arriver merges the records in split order and re-arms the
//           counter (decode_attn.h's scheme; no float atomics, deterministic for a given S).
#include "decode_attn.h"
#include "decode_attn_long.h"

namespace qeft {

constexpr int AL_KT = 32;                       // keys of a wave tile
constexpr int AL_VROW = 288;                    // bytes between staged V rows
constexpr int AL_VBYTES = AL_KT * AL_VROW;      // one wave's V tile
constexpr int AL_PROW = 132;                    // floats between the rows of a wave's partial (16-byte aligned rows)
static_assert(4 * 16 * AL_PROW * 4 <= 4 * AL_VBYTES, "the merge reuses the V staging area");
static_assert(kAttnLongStep == 4 * AL_KT, "a block step is one tile of each wave");

struct AttnLongArgs {
    const f16 *q, *k, *v;
    const float *cs, *sn;
    const int* out_pos;
    f16 *kc, *vc;
    const int* pos;
    f16* out;
    float* ws;
    int n_heads, grp, lgS, max_seq, whole_table;
};

// two transposing reads and their wait in one statement: the values are valid when it ends, wherever the compiler puts it
__device__ __forceinline__ h8 al_read_vt(uint32_t a0, uint32_t a1) {
    u32x2 lo, hi;
    asm volatile("ds_read_b64_tr_b16 %0, %2\n\tds_read_b64_tr_b16 %1, %3\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(lo), "=&v"(hi)
                 : "v"(a0), "v"(a1)
                 : "memory");
    return __builtin_bit_cast(h8, u32x4{lo[0], lo[1], hi[0], hi[1]});
}

__global__ __launch_bounds__(256) void rope_attn_decode_long_kernel(const AttnLongArgs a) {
    constexpr int HD = 128;
    __shared__ __attribute__((aligned(16))) uint8_t lds[4 * AL_VBYTES];   // the waves' V tiles; at the merge their partials
    __shared__ __attribute__((aligned(16))) f16 qs[16 * HD];              // rotated, scaled queries of the column tile
    __shared__ __attribute__((aligned(16))) f16 knew[HD];
    __shared__ __attribute__((aligned(16))) f16 vnew[HD];
    __shared__ float wmax[4][16], wsum[4][4][16];
    __shared__ int last_ticket;

    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int S = 1 << a.lgS, hk = (int)(blockIdx.x >> a.lgS), sp = (int)(blockIdx.x & (S - 1));
    const int grp = a.grp, max_seq = a.max_seq;
    const int pos = *a.pos;
    if (pos < 0 || pos >= max_seq) return;      // grid-uniform: nothing is written, no ticket is taken
    const int L = pos + 1;
    // the S ranges: multiples of the block step; [r0, r1) is empty for the splits past the context
    const int per = ((L + kAttnLongStep - 1) / kAttnLongStep + S - 1) / S * kAttnLongStep;
    const int r0 = sp * per, r1 = min(r0 + per, L);
    f16* const kch = a.kc + (size_t)hk * max_seq * HD;
    f16* const vch = a.vc + (size_t)hk * max_seq * HD;

    // ---- rotary of the new key, staging of the new value, append (the block whose range holds pos)
    const int ri = t & 63;
    const size_t trow = a.whole_table ? (size_t)pos * 64 : 0;
    const float rc = a.cs[trow + ri], rs = a.sn[trow + ri];
    const float scale = 0.08838834764831845f;   // 1/sqrt(128)
    const bool appender = sp == pos / per;
    if (t < 64) {
        const float ka = (float)a.k[hk * HD + ri], kb = (float)a.k[hk * HD + ri + 64];
        float x0 = ka * rc - kb * rs, x1 = kb * rc + ka * rs;
        asm("" : "+v"(x0), "+v"(x1));           // the rotated pair in fp32 once, then one rounding
        const f16 k0 = (f16)x0, k1 = (f16)x1;
        knew[ri] = k0;
        knew[ri + 64] = k1;
        if (appender) {
            kch[(size_t)pos * HD + ri] = k0;
            kch[(size_t)pos * HD + ri + 64] = k1;
        }
    } else if (t >= 128) {
        const f16 vv = a.v[hk * HD + (t - 128)];
        vnew[t - 128] = vv;
        if (appender) vch[(size_t)pos * HD + (t - 128)] = vv;
    }

    const int kr = lane & 15, g = lane >> 4;    // MFMA roles: row / column lane % 16, k group lane / 16
    uint8_t* const vl = lds + w * AL_VBYTES;
    // transposing read: lane 4 q + p of a 16-lane group addresses row q, dims 4 p .. 4 p + 3 of the group's 16; the group g reads
    // rows 4 g + q (keys 4 g .. 4 g + 3 of sub-tile 0) and 16 + 4 g + q (sub-tile 1); lane i of the group receives dim i
    const uint32_t vt0 = (uint32_t)(uintptr_t)vl + (uint32_t)((g * 4 + (kr >> 2)) * AL_VROW + (kr & 3) * 8);
    const uint32_t vt1 = vt0 + 16 * AL_VROW;

    // rows are clamped to pos: inside the cache and inside the context whatever the tile
    auto load_tile = [&](int t0, h8 (&kk)[2][4], h8 (&vv)[8]) {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const f16* row = kch + (size_t)min(t0 + sub * 16 + kr, pos) * HD + g * 8;
#pragma unroll
            for (int c = 0; c < 4; ++c) kk[sub][c] = *(const h8*)(row + c * 32);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) vv[i] = *(const h8*)(vch + (size_t)min(t0 + i * 4 + g, pos) * HD + kr * 8);
    };

    float* const part = (float*)lds;
    float* const rec0 = a.ws + attn_ctr_floats(a.n_heads);
    for (int ct = 0; ct * 16 < grp; ++ct) {
        __syncthreads();                        // knew / vnew staged; the previous tile's merge has read `lds` and qs
        // ---- rotary of the tile's 16 query heads (zero columns past grp; their address is clamped)
        for (int idx = t; idx < 16 * 64; idx += 256) {
            const int hh = idx >> 6, hg = ct * 16 + hh;
            const f16* src = a.q + (size_t)(hk * grp + min(hg, grp - 1)) * HD;
            const float qa = (float)src[ri], qb = (float)src[ri + 64];
            float x0 = qa * rc - qb * rs, x1 = qb * rc + qa * rs;
            asm("" : "+v"(x0), "+v"(x1));
            const f16 q0 = (f16)(x0 * scale), q1 = (f16)(x1 * scale);
            qs[hh * HD + ri] = hg < grp ? q0 : (f16)0.f;
            qs[hh * HD + ri + 64] = hg < grp ? q1 : (f16)0.f;
        }
        __syncthreads();
        h8 bq[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) bq[c] = *(const h8*)(qs + kr * HD + c * 32 + g * 8);
        const h8 vn = *(const h8*)(vnew + kr * 8);

        float m = -3.0e38f, lsum = 0.f;
        f32x4 acc[8];
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

        h8 kcur[2][4], vcur[8];
        load_tile(r0 + w * AL_KT, kcur, vcur);
        for (int t0 = r0 + w * AL_KT; t0 < r1; t0 += kAttnLongStep) {      // wave-uniform trip count
            h8 knext[2][4], vnext[8];
            load_tile(t0 + kAttnLongStep, knext, vnext);                   // this wave's next tile, in flight behind this one
            if (pos >= t0 && pos < t0 + AL_KT) {                           // wave-uniform: the tile of the token's own key
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const h8 kw = *(const h8*)(knew + c * 32 + g * 8);
#pragma unroll
                    for (int sub = 0; sub < 2; ++sub) kcur[sub][c] = (t0 + sub * 16 + kr == pos) ? kw : kcur[sub][c];
                }
            }
            // V rows to LDS: a cached row below pos, else the token's own v
#pragma unroll
            for (int i = 0; i < 8; ++i)
                *(h8*)(vl + (i * 4 + g) * AL_VROW + kr * 16) = (t0 + i * 4 + g < pos) ? vcur[i] : vn;
            // scores: lane (head kr, g) gets keys t0 + 16 sub + 4 g + i
            f32x4 sc[2];
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                sc[sub] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < 4; ++c) sc[sub] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kcur[sub][c], bq[c], sc[sub], 0, 0, 0);
            }
            float tm = -3.0e38f;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    sc[sub][i] = (t0 + sub * 16 + g * 4 + i > pos) ? -3.0e38f : sc[sub][i];
                    tm = fmaxf(tm, sc[sub][i]);
                }
            tm = fmaxf(tm, __shfl_xor(tm, 16));
            tm = fmaxf(tm, __shfl_xor(tm, 32));
            const float mn = fmaxf(m, tm);                                 // finite: a visited tile holds a live key
            const float alpha = __expf(m - mn);
            m = mn;
            h8 pb;
            float ps = 0.f;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float e = (t0 + sub * 16 + g * 4 + i > pos) ? 0.f : __expf(sc[sub][i] - mn);
                    const f16 eh = (f16)e;
                    pb[sub * 4 + i] = eh;
                    ps += (float)eh;                                       // the sum of what P.V multiplies
                }
            lsum = lsum * alpha + ps;
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) acc[dt] *= alpha;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             // the V rows are in LDS (this wave's own, in order)
#pragma unroll
            for (int dt = 0; dt < 8; ++dt)
                acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al_read_vt(vt0 + dt * 32, vt1 + dt * 32), pb, acc[dt], 0, 0, 0);
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int c = 0; c < 4; ++c) kcur[sub][c] = knext[sub][c];
#pragma unroll
            for (int i = 0; i < 8; ++i) vcur[i] = vnext[i];
        }

        // ---- merge the block's 4 waves (a wave without tiles has max -3e38 and sum 0)
        __syncthreads();                        // every wave is done with its V tile
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) *(f32x4*)(part + (w * 16 + kr) * AL_PROW + dt * 16 + g * 4) = acc[dt];
        if (g == 0) wmax[w][kr] = m;
        wsum[w][g][kr] = lsum;
        __syncthreads();
        for (int idx = t; idx < 16 * HD; idx += 256) {
            const int hh = idx >> 7, d = idx & (HD - 1), hg = ct * 16 + hh;
            if (hg >= grp) continue;
            const float M = fmaxf(fmaxf(wmax[0][hh], wmax[1][hh]), fmaxf(wmax[2][hh], wmax[3][hh]));
            float o = 0.f, den = 0.f;
#pragma unroll
            for (int ww = 0; ww < 4; ++ww) {
                const float f = __expf(wmax[ww][hh] - M);
                o += f * part[(ww * 16 + hh) * AL_PROW + d];
                den += f * ((wsum[ww][0][hh] + wsum[ww][1][hh]) + (wsum[ww][2][hh] + wsum[ww][3][hh]));
            }
            const int h = hk * grp + hg;
            if (S == 1) {
                const int oi = h * HD + d;
                a.out[a.out_pos ? a.out_pos[oi] : oi] = (f16)(o / den);
            } else {
                float* rec = rec0 + (size_t)(h * S + sp) * kAttnRec;
                st_agent(rec + d, o);
                if (d == 0) {
                    st_agent(rec + HD, M);
                    st_agent(rec + HD + 1, den);
                }
            }
        }
    }
    if (S == 1) return;

    // ---- the records are out: take the kv head's ticket; the last arriver merges its grp heads in split order
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned* ctr = (unsigned*)a.ws + hk;
    if (t == 0) {
        const unsigned ticket = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_ticket = (ticket == (unsigned)(S - 1));
        if (ticket == (unsigned)(S - 1)) __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!last_ticket) return;
    for (int idx = t; idx < grp * HD; idx += 256) {
        const int h = hk * grp + (idx >> 7), d = idx & (HD - 1);
        const float* r = rec0 + (size_t)h * S * kAttnRec;
        float Mh = -3.0e38f;
#pragma unroll 8                                // independent loads: several in flight (the sums keep the split order)
        for (int j = 0; j < S; ++j) Mh = fmaxf(Mh, ld_agent(r + j * kAttnRec + HD));
        float o = 0.f, den = 0.f;
#pragma unroll 8
        for (int j = 0; j < S; ++j) {
            const float f = __expf(ld_agent(r + j * kAttnRec + HD) - Mh);   // an empty split: factor 0
            o += f * ld_agent(r + j * kAttnRec + d);
            den += f * ld_agent(r + j * kAttnRec + HD + 1);
        }
        const int oi = h * HD + d;
        a.out[a.out_pos ? a.out_pos[oi] : oi] = (f16)(o / den);
    }
}

size_t attn_long_workspace_bytes(int n_heads, int S) { return S > 1 ? (attn_ctr_floats(n_heads) + (size_t)n_heads * S * kAttnRec) * 4 : 0; }

hipError_t rope_attn_decode_long_launch(const void* q, const void* k, const void* v, const void* cs, const void* sn, void* kc, void* vc,
                                        const int* pos, const int* out_pos, void* out, void* ws, int n_heads, int n_kv, int max_seq, int S,
                                        int tab_rows, hipStream_t st) {
    if (!attn_long_shape_ok(n_heads, n_kv, S, max_seq)) return hipErrorInvalidValue;
    int lgS = 0;
    while ((1 << lgS) != S) ++lgS;
    const AttnLongArgs a{(const f16*)q, (const f16*)k, (const f16*)v, (const float*)cs, (const float*)sn, out_pos, (f16*)kc, (f16*)vc, pos,
                         (f16*)out, (float*)ws, n_heads, n_heads / n_kv, lgS, max_seq, tab_rows != 1};
    g_last_variant = "attn_decode_long";
    hipLaunchKernelGGL(rope_attn_decode_long_kernel, dim3((unsigned)(n_kv * S)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace qeft
