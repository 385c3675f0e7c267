// The launches of batched decoding (BatchDecodeEngine, qeft_amd/batch.py): m <= 8 rows of m DIFFERENT sequences in one launch
// sequence, so that every weight byte streams once for all of them (the linears and the head are the verify pass's m-row
// launches, gemv_v3_multi.hip / decode_verify.hip; their rows are independent).  Row r serves cache slot slot[r]; the position
// and the stop state are per slot, all on the device, so a captured graph stays valid when the host rewrites the slot table.
//   token_begin_norm_b   embedding of tok[r] -> h32 [m][H], the first norm's producer form, rotary row of pos[slot[r]]
//   rope_attn_b          rotary + KV append + attention of row r over keys [0, pos[slot[r]]] of its own slot's cache
//   token_end_b          per-row argmax -> tok[r], out[r][k]; pos[slot] += 1; EOS / length stop on the device
// KV caches: [n_slots][n_kv][max_seq][128] fp16 per layer (one slot = the layout of DecodeEngine.kc[li]).
// The token-begin body and the block argmax are shared with the verify pass (decode_verify.hip): decode_rows.h.
#include "qeft_common.h"
#include "decode_attn.h"      // wave_max, st_agent / ld_agent, kAttnRec
#include "decode_rows.h"      // token_begin_norm_row, block_argmax_1024, row_slot, attn_b_ctr_floats
#include "host_launch.h"      // token_begin_norm_blocks

namespace qeft {

typedef float fx2 __attribute__((ext_vector_type(2)));

// ---- token begin, one row per sequence.  grid = (blocks of the one-row launch, m), block 256; row = blockIdx.y.  The rotary row is
// that of pos[slot[row]].
__global__ __launch_bounds__(256) void token_begin_norm_b_kernel(const f16* __restrict__ embed, const long long* __restrict__ toks,
                                                                 const float* __restrict__ rope_tab, const int* __restrict__ slot_tab,
                                                                 const int* __restrict__ pos_tab, float* __restrict__ h,
                                                                 float* __restrict__ rope_rows, const f16* __restrict__ gamma,
                                                                 f16* __restrict__ hnorm, float* __restrict__ ssq_out, int hidden,
                                                                 int vocab, int max_seq, int n_slots) {
    token_begin_norm_row(embed, toks, rope_tab, h, rope_rows, gamma, hnorm, ssq_out, hidden, vocab, max_seq, [&](int row) {
        const int s = row_slot(slot_tab, row, n_slots);
        return s >= 0 ? pos_tab[s] : 0;
    });
}

hipError_t token_begin_norm_b_launch(const void* embed, const void* toks, const void* rope_tab, const int* slot_tab, const int* pos_tab,
                                     void* h, void* rope_rows, const void* gamma, void* hnorm, float* ssq_out, int hidden, int vocab,
                                     int max_seq, int n_slots, int m, hipStream_t st) {
    hipLaunchKernelGGL(token_begin_norm_b_kernel, dim3(token_begin_norm_blocks(hidden), m), dim3(256), 0, st, (const f16*)embed,
                       (const long long*)toks, (const float*)rope_tab, slot_tab, pos_tab, (float*)h, (float*)rope_rows,
                       (const f16*)gamma, (f16*)hnorm, ssq_out, hidden, vocab, max_seq, n_slots);
    return hipGetLastError();
}

// ---- rotary + KV append + attention, one query token per row, each row in its own slot.
// grid = (n_kv * n_chunk * S, m) blocks of 256 threads (4 waves).  Block (x, row) serves row `row`, ONE kv head hk, hc of its
// group's query heads (a chunk; n_chunk = grp / hc), and split sp of that row's context: keys [0, p], p = pos[slot[row]], are
// dealt in runs of 16 positions to the 4 S waves of (row, kv head) (run j -> wave j % 4S), so a short row leaves some splits
// without keys (their records carry max -3e38: merge factor 0).  A wave loads a run's K and V once and scores it against the
// hc query heads (GQA: the run is read once per group).  Key p (this launch's own) comes from LDS, rotated here, so no block
// depends on another block's cache stores.  Online softmax per run, the block's 4 waves merged through LDS, and with S > 1 the
// last block of (row, kv head, chunk) to arrive merges the S records in split order (ticket counter; the counters sit in front
// of the records, at an offset that does not depend on (m, S)).
// A row whose slot is outside [0, n_slots), is done (done[slot] != 0), or whose p is outside [0, max_seq) writes nothing to the
// cache and zeros to its output.
template <int R>
__global__ __launch_bounds__(256) void rope_attn_b_kernel(const int* __restrict__ slot_tab, const int* __restrict__ pos_tab,
                                                          const int* __restrict__ done, const int* __restrict__ out_pos,
                                                          const f16* __restrict__ q, const f16* __restrict__ k,
                                                          const f16* __restrict__ v, const float* __restrict__ cs,
                                                          const float* __restrict__ sn, f16* __restrict__ kc, f16* __restrict__ vc,
                                                          f16* __restrict__ out, float* __restrict__ ws, int qkv_stride,
                                                          int out_stride, int tab_stride, int tab_rows, int max_seq, int n_slots,
                                                          int n_heads, int n_kv, int S, int hc) {
    constexpr int HD = 128;
    constexpr int NE = (R * HD + 255) / 256;         // (row, dim) pairs per thread
    extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
    f16* qs = (f16*)smem_raw;                        // [R][128] rotated, pre-scaled q
    f16* knew = qs + R * HD;                         // [128] this row's rotated k
    f16* vnew = knew + HD;                           // [128]
    float* pw = (float*)(vnew + HD);                 // [4 waves][R][16] exp weights of the current run
    float* wacc = pw + 4 * R * 16;                   // [4][R][128] the waves' P.V partials
    float* wM = wacc + 4 * R * HD;                   // [4][R]
    float* wl = wM + 4 * R;                          // [4][R]
    __shared__ int last_ticket;

    const int grp = n_heads / n_kv, n_chunk = grp / hc;
    const int row = blockIdx.y;
    const int bid = blockIdx.x, sp = bid % S, hkc = bid / S, chunk = hkc % n_chunk, hk = hkc / n_chunk;
    const int h0 = hk * grp + chunk * hc;            // first query head of this block
    const int rows = hc;
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int gw = sp * 4 + w, NWH = 4 * S;
    f16* const orow = out + (size_t)row * out_stride;
    auto store_out = [&](int e, float val) {
        const int r = e >> 7, d = e & 127, h = h0 + r;
        orow[out_pos ? out_pos[h * HD + d] : h * HD + d] = (f16)val;
    };
    const int slot = row_slot(slot_tab, row, n_slots);
    const int pos = slot >= 0 ? pos_tab[slot] : -1;
    if (slot < 0 || (done && done[slot] != 0) || pos < 0 || pos >= max_seq) {     // uniform over the row's blocks
        if (sp == 0)
            for (int e = t; e < rows * HD; e += 256) store_out(e, 0.f);
        return;
    }
    const size_t cbase = ((size_t)slot * n_kv + hk) * max_seq * HD;
    f16* const kch = kc + cbase;
    f16* const vch = vc + cbase;
    const bool appender = sp == 0 && chunk == 0;
    const int Lk = pos + 1;
    const f16* const qr0 = q + (size_t)row * qkv_stride;
    const f16* const kr0 = k + (size_t)row * qkv_stride + (size_t)hk * HD;
    const f16* const vr0 = v + (size_t)row * qkv_stride + (size_t)hk * HD;

    // ---- rotary of the block's q rows and of the kv head's new k row; the new v row; the appender writes the caches
    const size_t ro = tab_rows >= max_seq ? (size_t)pos * tab_stride : (size_t)row * tab_stride;
    auto rot = [&](int ii, float a, float b, float& r0, float& r1) {
        const float c = cs[ro + ii], s = sn[ro + ii];
        r0 = a * c - b * s;
        r1 = b * c + a * s;
    };
    for (int e = t; e < R * 64; e += 256) {
        const int r = e >> 6, ii = e & 63;
        if (r < rows) {
            const f16* src = qr0 + (size_t)(h0 + r) * HD;
            float r0, r1;
            rot(ii, (float)src[ii], (float)src[ii + 64], r0, r1);
            const float scale = 0.08838834764831845f;   // 1/sqrt(128)
            qs[r * HD + ii] = (f16)(r0 * scale);
            qs[r * HD + ii + 64] = (f16)(r1 * scale);
        } else {                                     // padding rows: zero (their scores are masked anyway)
            qs[r * HD + ii] = (f16)0.f;
            qs[r * HD + ii + 64] = (f16)0.f;
        }
    }
    if (t < 64) {
        float r0, r1;
        rot(t, (float)kr0[t], (float)kr0[t + 64], r0, r1);
        const f16 k0 = (f16)r0, k1 = (f16)r1;
        knew[t] = k0;
        knew[t + 64] = k1;
        if (appender) {
            kch[(size_t)pos * HD + t] = k0;
            kch[(size_t)pos * HD + t + 64] = k1;
        }
    } else if (t < 64 + HD) {
        const int d = t - 64;
        const f16 vv = vr0[d];
        vnew[d] = vv;
        if (appender) vch[(size_t)pos * HD + d] = vv;
    }
    __syncthreads();

    // ---- this wave's runs.  Score role: lane = (position pj of the run, dim quarter qd); P.V role: lane = dims 2 lane, 2 lane + 1
    const int qd = lane & 3, pj = lane >> 2, d0 = 2 * lane;
    float Mx[R], ls[R];
    fx2 acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        Mx[r] = -3.0e38f;
        ls[r] = 0.f;
        acc[r] = fx2{0.f, 0.f};
    }
    float* const pwv = pw + w * R * 16;
    const int nrun = (Lk + 15) >> 4;
    h8 kr[4];
    h2 vr[16];
    auto load_run = [&](int j) {        // rows < max_seq always (pos < max_seq, max_seq % 16 == 0); rows >= pos replaced below
        const int r0 = j * 16;
#pragma unroll
        for (int c = 0; c < 4; ++c) kr[c] = *(const h8*)(kch + (size_t)(r0 + pj) * HD + qd * 8 + 32 * c);
#pragma unroll
        for (int p = 0; p < 16; ++p) vr[p] = *(const h2*)(vch + (size_t)(r0 + p) * HD + d0);
    };
    int j = gw;
    if (j < nrun) load_run(j);
    for (; j < nrun; j += NWH) {
        const int r0 = j * 16, p = r0 + pj;
        h8 kk[4];
        h2 vv[16];
#pragma unroll
        for (int c = 0; c < 4; ++c) kk[c] = p >= pos ? *(const h8*)(knew + qd * 8 + 32 * c) : kr[c];
#pragma unroll
        for (int e = 0; e < 16; ++e) vv[e] = r0 + e >= pos ? *(const h2*)(vnew + d0) : vr[e];
        if (j + NWH < nrun) load_run(j + NWH);       // the next run's K / V in flight during this one
        float scl[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const h8* qr = (const h8*)(qs + r * HD + qd * 8);
            float sdot = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const h8 qv = qr[4 * c];
                const u32x4 kw = __builtin_bit_cast(u32x4, kk[c]), qw = __builtin_bit_cast(u32x4, qv);
#pragma unroll
                for (int e = 0; e < 4; ++e) sdot = dot2(as_h2(qw[e]), as_h2(kw[e]), sdot);
            }
            sdot += dpp_mov<0xB1>(sdot);
            sdot += dpp_mov<0x4E>(sdot);
            const bool ok = p <= pos && r < rows;
            const float s = ok ? sdot : -3.0e38f;
            const float mn = fmaxf(Mx[r], wave_max(s));
            const float ev = ok ? __expf(s - mn) : 0.f;
            if (qd == 0) pwv[r * 16 + pj] = ev;
            scl[r] = __expf(Mx[r] - mn);
            Mx[r] = mn;
        }
        __builtin_amdgcn_wave_barrier();              // pw of this wave: written and read by this wave only
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const f32x4* pr = (const f32x4*)(pwv + r * 16);
            float a0 = acc[r][0] * scl[r], a1 = acc[r][1] * scl[r], l = ls[r] * scl[r];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const f32x4 e4 = pr[c];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const h2 vx = vv[4 * c + e];
                    a0 += e4[e] * (float)vx[0];
                    a1 += e4[e] * (float)vx[1];
                    l += e4[e];
                }
            }
            acc[r] = fx2{a0, a1};
            ls[r] = l;
        }
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        *(fx2*)(wacc + ((size_t)w * R + r) * HD + d0) = acc[r];
        if (lane == 0) {
            wM[w * R + r] = Mx[r];
            wl[w * R + r] = ls[r];
        }
    }
    __syncthreads();
    // ---- merge the block's 4 waves (a wave without positions has max -3e38: factor 0); thread -> (row, dim) pairs
    const int nel = rows * HD;
    float mrg[NE], mM[NE], mD[NE];
#pragma unroll
    for (int u = 0; u < NE; ++u) {
        const int e = t + 256 * u, r = e >> 7, d = e & 127;
        mrg[u] = 0.f;
        mM[u] = -3.0e38f;
        mD[u] = 0.f;
        if (e < nel) {
            const float M = fmaxf(fmaxf(wM[r], wM[R + r]), fmaxf(wM[2 * R + r], wM[3 * R + r]));
            float a = 0.f, den = 0.f;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float f = __expf(wM[g * R + r] - M);
                a += f * wacc[((size_t)g * R + r) * HD + d];
                den += f * wl[g * R + r];
            }
            mrg[u] = a;
            mM[u] = M;
            mD[u] = den;
        }
    }
    if (S == 1) {
#pragma unroll
        for (int u = 0; u < NE; ++u)
            if (t + 256 * u < nel) store_out(t + 256 * u, mrg[u] / mD[u]);
        return;
    }
    // ---- publish this split's records (one per query head: acc[128], max, sum), take a ticket; the last arriver merges
    float* const recs = ws + attn_b_ctr_floats(n_heads) + (size_t)row * n_heads * S * kAttnRec;
#pragma unroll
    for (int u = 0; u < NE; ++u) {
        const int e = t + 256 * u, r = e >> 7, d = e & 127;
        if (e < nel) {
            float* rec = recs + ((size_t)(h0 + r) * S + sp) * kAttnRec;
            st_agent(rec + d, mrg[u]);
            if (d == 0) {
                st_agent(rec + HD, mM[u]);
                st_agent(rec + HD + 1, mD[u]);
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned* ctr = (unsigned*)ws + (size_t)row * (n_kv * n_chunk) + hkc;
    if (t == 0) {
        const unsigned ticket = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_ticket = (ticket == (unsigned)(S - 1));
        if (ticket == (unsigned)(S - 1)) __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!last_ticket) return;
#pragma unroll
    for (int u = 0; u < NE; ++u) {
        const int e = t + 256 * u, r = e >> 7, d = e & 127;
        if (e < nel) {
            const float* r0 = recs + (size_t)(h0 + r) * S * kAttnRec;
            float Mh = -3.0e38f;
            for (int s = 0; s < S; ++s) Mh = fmaxf(Mh, ld_agent(r0 + s * kAttnRec + HD));
            float a2 = 0.f, d2 = 0.f;
            for (int s = 0; s < S; ++s) {
                const float f = __expf(ld_agent(r0 + s * kAttnRec + HD) - Mh);      // a split without positions: factor 0
                a2 += f * ld_agent(r0 + s * kAttnRec + d);
                d2 += f * ld_agent(r0 + s * kAttnRec + HD + 1);
            }
            store_out(e, a2 / d2);
        }
    }
}

// heads of a chunk: the largest divisor of the group that is <= 8 (one block scores hc heads against each K/V run it loads)
static int attn_b_chunk(int grp) {
    int hc = 1;
    for (int d = 1; d <= grp && d <= 8; ++d)
        if (grp % d == 0) hc = d;
    return hc;
}

size_t attn_b_smem_bytes(int R) { return (size_t)R * 128 * 2 + 2 * 128 * 2 + 4 * R * 16 * 4 + 4 * R * 128 * 4 + 2 * 4 * R * 4; }

size_t attn_b_workspace_bytes(int n_heads, int S, int m) {
    return S > 1 ? (attn_b_ctr_floats(n_heads) + (size_t)m * n_heads * S * kAttnRec) * 4 : 0;
}

hipError_t rope_attn_b_launch(const AttnRowsArgs& a, hipStream_t st) {
    const int grp = a.n_heads / a.n_kv, hc = attn_b_chunk(grp);
    const int R = hc <= 1 ? 1 : hc <= 2 ? 2 : hc <= 4 ? 4 : 8;
    const size_t smem = attn_b_smem_bytes(R);
    auto go = [&](auto kern) -> hipError_t {
        hipLaunchKernelGGL(kern, dim3(a.n_kv * (grp / hc) * a.S, a.m), dim3(256), smem, st, a.slot_tab, a.pos, a.done, a.out_pos,
                           (const f16*)a.q, (const f16*)a.k, (const f16*)a.v, (const float*)a.cs, (const float*)a.sn, (f16*)a.kc, (f16*)a.vc,
                           (f16*)a.out, (float*)a.ws, a.qkv_stride, a.out_stride, a.tab_stride, a.tab_rows, a.max_seq, a.n_slots, a.n_heads,
                           a.n_kv, a.S, hc);
        return hipGetLastError();
    };
    if (R == 1) return go(rope_attn_b_kernel<1>);
    if (R == 2) return go(rope_attn_b_kernel<2>);
    if (R == 4) return go(rope_attn_b_kernel<4>);
    return go(rope_attn_b_kernel<8>);
}

// ---- token end, one block of 1024 per row.  Row r, slot s = slot[r], k = ctr[0] (the step counter):
//   s done (or outside the table): out[r][k] = -1, nothing else changes;
//   otherwise a = argmax(logits[r]) (lowest index among equal maxima, as token_end), tok[r] = a, out[r][k] = a, pos[s] += 1, and
//   done[s] = 1 if a == eos[s] (eos[s] >= 0), else 2 if the new position reaches limit[s].
// The last row to arrive (ticket ctr[1]) advances ctr[0] and re-arms ctr[1].  out[r][k] is written only for k < out_cap.
__global__ __launch_bounds__(1024) void token_end_b_kernel(const f16* __restrict__ logits, const int* __restrict__ slot_tab,
                                                           long long* __restrict__ tok, int* __restrict__ pos_tab,
                                                           const int* __restrict__ limit, const int* __restrict__ eos,
                                                           int* __restrict__ done, long long* __restrict__ out, int* __restrict__ ctr,
                                                           int vocab, int out_cap, int n_slots) {
    __shared__ float bv[16];
    __shared__ int bi[16];
    const int t = threadIdx.x, row = blockIdx.x;
    const int s = row_slot(slot_tab, row, n_slots);
    const bool active = s >= 0 && done[s] == 0;       // uniform over the block
    const int a = active ? block_argmax_1024(logits + (size_t)row * vocab, vocab, bv, bi) : 0;
    if (t != 0) return;
    const int k = ctr[0];
    if (active) {
        tok[row] = a;
        if (k >= 0 && k < out_cap) out[(size_t)row * out_cap + k] = a;
        const int np = pos_tab[s] + 1;
        pos_tab[s] = np;
        if (eos[s] >= 0 && a == eos[s]) done[s] = 1;
        else if (np >= limit[s]) done[s] = 2;
    } else if (k >= 0 && k < out_cap) {
        out[(size_t)row * out_cap + k] = -1;
    }
    // (k has been used above, so its load completed before this arrival; the last arriver alone advances it)
    const int ticket = __hip_atomic_fetch_add(ctr + 1, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket == (int)gridDim.x - 1) {
        __hip_atomic_store(ctr + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(ctr, k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

hipError_t token_end_b_launch(const void* logits, const int* slot_tab, void* tok, int* pos_tab, const int* limit, const int* eos,
                              int* done, void* out, int* ctr, int vocab, int out_cap, int n_slots, int m, hipStream_t st) {
    hipLaunchKernelGGL(token_end_b_kernel, dim3(m), dim3(1024), 0, st, (const f16*)logits, slot_tab, (long long*)tok, pos_tab, limit,
                       eos, done, (long long*)out, ctr, vocab, out_cap, n_slots);
    return hipGetLastError();
}

}  // namespace qeft
