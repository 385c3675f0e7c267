// Decode attention over an e4m3 KV cache (kv_dtype="fp8" of DecodeEngine / BatchDecodeEngine).
//   kv8_quant_row        the cache recipe of include/qeft_hip.h for one row of 128, by one wave (decode_kv8.h)
//   kv8_store_rows       T already rotated K rows and V rows -> codes + scales at positions p0 .. p0 + T - 1 (the prefill hand-over)
//   rope_attn_kv8        rotary + quantise + append + attention, one query token per row, each row in its own slot
// Cache of one slot and layer: K codes, V codes uint8 [n_kv][max_seq][128]; K scales, V scales fp32 [n_kv][max_seq]; a batch
// engine's arrays carry [n_slots] in front.  A value is float(code) * scale.
#include "qeft_common.h"
#include "decode_attn.h"      // wave_max, dpp_mov, st_agent / ld_agent, kAttnRec
#include "decode_rows.h"      // row_slot, attn_b_ctr_floats
#include "decode_kv8.h"       // kv8_quant_row, Kv8Run, fx2, the host side of the launch

namespace qeft {

// ---- prefill hand-over.  grid = (n_kv, T), block 128: wave 0 the K row of (kv head, t), wave 1 the V row.
__global__ __launch_bounds__(128) void kv8_store_rows_kernel(const f16* __restrict__ k, const f16* __restrict__ v, int row_stride,
                                                             uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                                             float* __restrict__ ks, float* __restrict__ vs, int max_seq, int p0) {
    const int hk = blockIdx.x, tt = blockIdx.y, lane = threadIdx.x & 63;
    const bool is_v = threadIdx.x >= 64;              // wave-uniform
    const f16* src = (is_v ? v : k) + (size_t)tt * row_stride + (size_t)hk * 128;
    const size_t r = (size_t)hk * max_seq + p0 + tt;
    uint8_t* dst = (is_v ? vc : kc) + r * 128;
    uint8_t ca, cb;
    float scale;
    kv8_quant_row((float)src[lane], (float)src[lane + 64], ca, cb, scale);
    dst[lane] = ca;
    dst[lane + 64] = cb;
    if (lane == 0) (is_v ? vs : ks)[r] = scale;
}

hipError_t kv8_store_rows_launch(const void* k, const void* v, int row_stride, void* kc, void* vc, void* ks, void* vs, int n_kv,
                                 int max_seq, int p0, int T, hipStream_t st) {
    hipLaunchKernelGGL(kv8_store_rows_kernel, dim3(n_kv, T), dim3(128), 0, st, (const f16*)k, (const f16*)v, row_stride, (uint8_t*)kc,
                       (uint8_t*)vc, (float*)ks, (float*)vs, max_seq, p0);
    return hipGetLastError();
}

// ---- rotary + quantise + append + attention.  The grid, the dealing of 16-position runs to the 4 S waves of a (row, kv head), the
// GQA chunking, the online softmax, the split merge and the rules for skipped rows are rope_attn_b_kernel's (decode_batch.hip);
// the block merge and the split merge below are its code.  What differs is what a run is: 16 rows of 128 BYTES.  This kernel is
// rope_attn_m_kv8_kernel (decode_verify_kv8.hip) at m = 1 with the slot table and `done` in front, one grid row per sequence and a
// per-row workspace offset.  The two share the host side of the launch (decode_kv8.h); their device code is written out in both
// files, so a fix belongs in both: shared, this kernel ran slower (decode_kv8.h's header, profiles/kv8_attn_core_refactor.log).
//   score role  lane = (position pj = lane / 4, quarter qd = lane % 4): two 16-byte loads, dims qd * 16 + 64 c .. + 16 (the 4 lanes of
//               a position read 64 contiguous bytes per instruction, a wave 1 KB), and the position's two scales;
//   P.V role    lane = (position class pc = lane / 16, dim group dg = lane % 16): four 8-byte loads, dims dg * 8 .. + 8 of positions
//               4 pc .. 4 pc + 3 (16 lanes read one 128-byte row); the 4 classes' partial sums meet once per wave, after its last run.
// Two runs are in flight per wave (the loads of run j + 2 * 4S are issued before run j is computed): a run is half the bytes it
// was in fp16, so the depth is what keeps the bytes in flight the same.  Codes become fp32 by v_cvt_pk_f32_fp8 (K then packs to
// fp16 pairs, exactly, for v_dot2_f32_f16 against the fp16 q in LDS; the conversion is shared by the chunk's hc heads); the K scale
// multiplies the finished score, the V scale the exp weight (e * v_scale[p]).
// This launch's own row is quantised here (wave 0: K after rotary and fp16 rounding, wave 1: V), kept in LDS as codes + scale and
// takes the place of cache row `pos` in the run that holds it, so the token is seen exactly as the cache holds it and no block
// reads another block's stores.
template <int R>
__global__ __launch_bounds__(256) void rope_attn_kv8_kernel(const int* __restrict__ slot_tab, const int* __restrict__ pos_tab,
                                                            const int* __restrict__ done, const int* __restrict__ out_pos,
                                                            const f16* __restrict__ q, const f16* __restrict__ k,
                                                            const f16* __restrict__ v, const float* __restrict__ cs,
                                                            const float* __restrict__ sn, uint8_t* __restrict__ kc,
                                                            uint8_t* __restrict__ vc, float* __restrict__ ksc, float* __restrict__ vsc,
                                                            f16* __restrict__ out, float* __restrict__ ws, int qkv_stride,
                                                            int out_stride, int tab_stride, int tab_rows, int max_seq, int n_slots,
                                                            int n_heads, int n_kv, int S, int hc) {
    constexpr int HD = 128;
    constexpr int NE = (R * HD + 255) / 256;         // (row, dim) pairs per thread
    extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
    f16* qs = (f16*)smem_raw;                        // [R][128] rotated, pre-scaled q
    uint8_t* knew = (uint8_t*)(qs + R * HD);         // [128] codes of this row's rotated k
    uint8_t* vnew = knew + HD;                       // [128]
    float* nsc = (float*)(vnew + HD);                // [4]: k scale, v scale of the new row
    float* pw = nsc + 4;                             // [4 waves][R][16] exp weights of the current run
    float* pwv = pw + 4 * R * 16;                    // [4 waves][R][16] exp weight * v scale
    float* wacc = pwv + 4 * R * 16;                  // [4][R][128] the waves' P.V partials
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
    const size_t sbase = ((size_t)slot * n_kv + hk) * max_seq;
    uint8_t* const kch = kc + sbase * HD;
    uint8_t* const vch = vc + sbase * HD;
    float* const ksh = ksc + sbase;
    float* const vsh = vsc + sbase;
    const bool appender = sp == 0 && chunk == 0;
    const int Lk = pos + 1;
    const f16* const qr0 = q + (size_t)row * qkv_stride;
    const f16* const kr0 = k + (size_t)row * qkv_stride + (size_t)hk * HD;
    const f16* const vr0 = v + (size_t)row * qkv_stride + (size_t)hk * HD;

    // ---- this wave's first two runs: nothing below depends on them until the loop
    const int qd = lane & 3, pj = lane >> 2, dg = lane & 15, pc = lane >> 4;
    const int nrun = (Lk + 15) >> 4;
    auto load_run = [&](Kv8Run& b, int j) {        // rows < max_seq always (pos < max_seq, max_seq % 16 == 0).  A run past the
        const int r0 = (j < nrun ? j : 0) * 16;      // context re-reads run 0 (never used): the load count stays fixed
        const uint8_t* kp = kch + (size_t)(r0 + pj) * HD + qd * 16;
        b.k[0] = *(const u32x4*)kp;
        b.k[1] = *(const u32x4*)(kp + 64);
        const uint8_t* vp = vch + (size_t)(r0 + pc * 4) * HD + dg * 8;
#pragma unroll
        for (int i = 0; i < 4; ++i) b.v[i] = *(const u32x2*)(vp + i * HD);
        b.ks = ksh[r0 + pj];
        b.vs = vsh[r0 + pj];
    };
    Kv8Run bufA, bufB;
    load_run(bufA, gw);
    load_run(bufB, gw + NWH);

    // ---- rotary of the block's q rows; the kv head's new k row (rotary, fp16, quantise) and v row; the appender writes the caches
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
    if (w < 2) {                                     // wave 0: K, wave 1: V
        float a, b;
        if (w == 0) {
            float r0, r1;
            rot(lane, (float)kr0[lane], (float)kr0[lane + 64], r0, r1);
            a = (float)(f16)r0;                      // the fp16 row an fp16 cache would hold
            b = (float)(f16)r1;
        } else {
            a = (float)vr0[lane];
            b = (float)vr0[lane + 64];
        }
        uint8_t ca, cb;
        float scale;
        kv8_quant_row(a, b, ca, cb, scale);
        uint8_t* const nw = w == 0 ? knew : vnew;
        nw[lane] = ca;
        nw[lane + 64] = cb;
        if (lane == 0) nsc[w] = scale;
        if (appender) {
            uint8_t* const dst = (w == 0 ? kch : vch) + (size_t)pos * HD;
            dst[lane] = ca;
            dst[lane + 64] = cb;
            if (lane == 0) (w == 0 ? ksh : vsh)[pos] = scale;
        }
    }
    __syncthreads();

    float Mx[R], ls[R], acc[R][8];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        Mx[r] = -3.0e38f;
        ls[r] = 0.f;
#pragma unroll
        for (int d = 0; d < 8; ++d) acc[r][d] = 0.f;
    }
    float* const pww = pw + w * R * 16;
    float* const pwvw = pwv + w * R * 16;
    const float nks = nsc[0], nvs = nsc[1];

    // one run: `buf` holds run j and is refilled with run j + 2 NWH as soon as its registers are taken over
    auto do_run = [&](Kv8Run& buf, int j) {
        const int r0 = j * 16, p = r0 + pj;
        u32x4 kk[2] = {buf.k[0], buf.k[1]};
        u32x2 vv[4] = {buf.v[0], buf.v[1], buf.v[2], buf.v[3]};
        float ksv = buf.ks, vsv = buf.vs;
        if (r0 + 15 >= pos) {                        // the context's last run: row pos comes from LDS, and so do the rows behind
            const bool fresh = p >= pos;             // it (finite stand-ins: their scores are masked, their weights 0)
#pragma unroll
            for (int c = 0; c < 2; ++c) kk[c] = fresh ? *(const u32x4*)(knew + qd * 16 + 64 * c) : kk[c];
#pragma unroll
            for (int i = 0; i < 4; ++i) vv[i] = r0 + pc * 4 + i >= pos ? *(const u32x2*)(vnew + dg * 8) : vv[i];
            ksv = fresh ? nks : ksv;
            vsv = fresh ? nvs : vsv;
        }
        load_run(buf, j + 2 * NWH);
        // K codes -> fp16 pairs (every e4m3 value is an fp16 value)
        h2 kh[16];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const fx2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)kk[c][e], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)kk[c][e], true);
                kh[c * 8 + e * 2] = __builtin_bit_cast(h2, __builtin_amdgcn_cvt_pkrtz(lo[0], lo[1]));
                kh[c * 8 + e * 2 + 1] = __builtin_bit_cast(h2, __builtin_amdgcn_cvt_pkrtz(hi[0], hi[1]));
            }
        float scl[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float sdot = 0.f;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const h8* qr = (const h8*)(qs + r * HD + qd * 16 + 64 * c);
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const u32x4 qw = __builtin_bit_cast(u32x4, qr[g]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) sdot = dot2(as_h2(qw[e]), kh[c * 8 + g * 4 + e], sdot);
                }
            }
            sdot += dpp_mov<0xB1>(sdot);
            sdot += dpp_mov<0x4E>(sdot);
            sdot *= ksv;                             // the row's scale, once per score
            const bool ok = p <= pos && r < rows;
            const float s = ok ? sdot : -3.0e38f;
            const float mn = fmaxf(Mx[r], wave_max(s));
            const float ev = ok ? __expf(s - mn) : 0.f;
            if (qd == 0) {
                pww[r * 16 + pj] = ev;
                pwvw[r * 16 + pj] = ev * vsv;        // the V row's scale, once per weight
            }
            scl[r] = __expf(Mx[r] - mn);
            Mx[r] = mn;
        }
        __builtin_amdgcn_wave_barrier();              // pw of this wave: written and read by this wave only
        float vf[4][8];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const fx2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)vv[i][e], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)vv[i][e], true);
                vf[i][4 * e] = lo[0];
                vf[i][4 * e + 1] = lo[1];
                vf[i][4 * e + 2] = hi[0];
                vf[i][4 * e + 3] = hi[1];
            }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const f32x4 e4 = *(const f32x4*)(pww + r * 16 + pc * 4), w4 = *(const f32x4*)(pwvw + r * 16 + pc * 4);
            ls[r] = ls[r] * scl[r] + ((e4[0] + e4[1]) + (e4[2] + e4[3]));
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                float a = acc[r][d] * scl[r];
#pragma unroll
                for (int i = 0; i < 4; ++i) a += w4[i] * vf[i][d];
                acc[r][d] = a;
            }
        }
        __builtin_amdgcn_wave_barrier();
    };
    for (int j = gw; j < nrun; j += 2 * NWH) {
        do_run(bufA, j);
        if (j + NWH < nrun) do_run(bufB, j + NWH);
    }
    // the 4 position classes of a wave meet (lanes l, l ^ 16, l ^ 32, l ^ 48 hold the same dims)
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            float a = acc[r][d];
            a += __shfl_xor(a, 16);
            a += __shfl_xor(a, 32);
            acc[r][d] = a;
        }
        float l = ls[r];
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        if (pc == 0) {
            float* dst = wacc + ((size_t)w * R + r) * HD + dg * 8;
            *(f32x4*)dst = f32x4{acc[r][0], acc[r][1], acc[r][2], acc[r][3]};
            *(f32x4*)(dst + 4) = f32x4{acc[r][4], acc[r][5], acc[r][6], acc[r][7]};
        }
        if (lane == 0) {
            wM[w * R + r] = Mx[r];
            wl[w * R + r] = l;
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

size_t attn_kv8_workspace_bytes(int n_heads, int S, int m) {
    return S > 1 ? (attn_b_ctr_floats(n_heads) + (size_t)m * n_heads * S * kAttnRec) * 4 : 0;
}

hipError_t rope_attn_kv8_launch(const AttnRowsArgs& a, hipStream_t st) {
    const int grp = a.n_heads / a.n_kv, hc = kv8_attn_chunk(grp, 1);
    return kv8_attn_dispatch(hc, [&](auto rc) {
        constexpr int R = decltype(rc)::value;
        hipLaunchKernelGGL(rope_attn_kv8_kernel<R>, dim3(a.n_kv * (grp / hc) * a.S, a.m), dim3(256), kv8_attn_smem_bytes<1>(R), st,
                           a.slot_tab, a.pos, a.done, a.out_pos, (const f16*)a.q, (const f16*)a.k, (const f16*)a.v, (const float*)a.cs,
                           (const float*)a.sn, (uint8_t*)a.kc, (uint8_t*)a.vc, (float*)a.ks, (float*)a.vs, (f16*)a.out, (float*)a.ws,
                           a.qkv_stride, a.out_stride, a.tab_stride, a.tab_rows, a.max_seq, a.n_slots, a.n_heads, a.n_kv, a.S, hc);
        return hipGetLastError();
    });
}

}  // namespace qeft
