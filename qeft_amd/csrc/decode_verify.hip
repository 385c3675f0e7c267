// The m-row launches of the verify pass (DecodeEngine.verify): m <= 8 tokens of ONE sequence at positions pos .. pos + m - 1
// scored in one launch sequence, so that every weight byte streams once for all m rows (the GEMV: gemv_v3_multi.hip).
//   token_begin_norm_m   embedding of m tokens -> h32 [m][H], the first norm's producer form per row, rotary rows [m][128]
//   rope_attn_m          rotary + KV append of m rows + causal attention: query i sees keys [0, pos + i]
//   lm_head_m            final RMSNorm + fp16 head for m rows: the head streams once
//   verify_greedy        per-row argmax, longest accepted prefix, next token and position on the device
// Every kernel follows the one-row kernel it extends (decode_aux.hip, decode_attn.h) in its arithmetic, so that a row of an
// m-row launch reproduces the one-row launch where the summation order allows it.  The token-begin body and the block argmax
// are shared with the launches of batched decoding (decode_batch.hip): decode_rows.h.
#include "qeft_common.h"
#include "decode_attn.h"      // wave_max, st_agent / ld_agent, kAttnRec
#include "decode_rows.h"      // token_begin_norm_row, block_argmax_1024, attn_m_ctr_floats
#include "host_launch.h"      // token_begin_norm_blocks

namespace qeft {

typedef float fx2 __attribute__((ext_vector_type(2)));

// ---- token begin, m rows.  grid = (blocks of the one-row launch, m), block 256; row i = blockIdx.y.
__global__ __launch_bounds__(256) void token_begin_norm_m_kernel(const f16* __restrict__ embed, const long long* __restrict__ toks,
                                                                 const float* __restrict__ rope_tab, const int* __restrict__ pos,
                                                                 float* __restrict__ h, float* __restrict__ rope_rows,
                                                                 const f16* __restrict__ gamma, f16* __restrict__ hnorm,
                                                                 float* __restrict__ ssq_out, int hidden, int vocab, int max_seq) {
    token_begin_norm_row(embed, toks, rope_tab, h, rope_rows, gamma, hnorm, ssq_out, hidden, vocab, max_seq,
                         [&](int row) { return *pos + row; });
}

hipError_t token_begin_norm_m_launch(const void* embed, const void* toks, const void* rope_tab, const int* pos, void* h,
                                     void* rope_rows, const void* gamma, void* hnorm, float* ssq_out, int hidden, int vocab,
                                     int max_seq, int m, hipStream_t st) {
    hipLaunchKernelGGL(token_begin_norm_m_kernel, dim3(token_begin_norm_blocks(hidden), m), dim3(256), 0, st, (const f16*)embed,
                       (const long long*)toks, (const float*)rope_tab, pos, (float*)h, (float*)rope_rows, (const f16*)gamma,
                       (f16*)hnorm, ssq_out, hidden, vocab, max_seq);
    return hipGetLastError();
}

// ---- multi-query rotary + KV append + causal attention.
// grid = n_kv * n_chunk * S blocks of 256 threads (4 waves).  A block serves ONE kv head: hc of its group's query heads (a chunk;
// n_chunk = grp / hc) times the m queries = R rows (r = hl * m + i), and split sp of the context.  Keys [0, pos + m) are dealt in
// runs of 16 positions to the 4 S waves of the kv head (run j -> wave j % 4S).  A wave loads a run's K and V ONCE and scores
// it against all R rows; keys at or past `pos` (this launch's own rows) come from LDS, rotated here, so no block depends on
// another block's cache stores.  Query i's causal bound is key <= pos + i.  Per row the wave keeps a running maximum, exp
// sum and its P.V partial (online softmax, per run); the block merges its 4 waves through LDS, and with S > 1 the last block
// of the kv head to arrive merges the S records in split order (ticket counter per (kv head, chunk), as decode_attn.h;
// the counters sit in front of the records).
// Rows (i) of q / k / v are qkv_stride elements apart; out row i is out_stride elements apart, element e of head h at
// out_pos[h * 128 + e] when out_pos is given.  Rotary rows: tab_rows == m: row i of cs / sn (tab_stride floats apart) is
// position pos + i; otherwise the tables are indexed by position.
// workspace: the arrival counters come FIRST, at an offset that does not depend on (m, S) -- passes of different m / split share
// one workspace, and a counter must never land on another configuration's records (attn_m_ctr_floats, decode_rows.h)

template <int R>
__global__ __launch_bounds__(256) void rope_attn_m_kernel(const int* __restrict__ pos_ptr, const int* __restrict__ out_pos,
                                                          const f16* __restrict__ q, const f16* __restrict__ k,
                                                          const f16* __restrict__ v, const float* __restrict__ cs,
                                                          const float* __restrict__ sn, f16* __restrict__ kc, f16* __restrict__ vc,
                                                          f16* __restrict__ out, float* __restrict__ ws, int qkv_stride,
                                                          int out_stride, int tab_stride, int tab_rows, int max_seq,
                                                          int n_heads, int n_kv, int S, int m, int hc) {
    constexpr int HD = 128;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
    f16* qs = (f16*)smem_raw;                        // [R][128] rotated, pre-scaled q
    f16* knew = qs + R * HD;                         // [8][128] this launch's rotated k rows
    f16* vnew = knew + 8 * HD;                       // [8][128]
    float* pw = (float*)(vnew + 8 * HD);             // [4 waves][R][16] exp weights of the current run
    float* wacc = pw + 4 * R * 16;                   // [4][R][128] the waves' P.V partials
    float* wM = wacc + 4 * R * HD;                   // [4][R]
    float* wl = wM + 4 * R;                          // [4][R]
    __shared__ int last_ticket;

    const int grp = n_heads / n_kv, n_chunk = grp / hc;
    const int bid = blockIdx.x, sp = bid % S, hkc = bid / S, chunk = hkc % n_chunk, hk = hkc / n_chunk;
    const int h0 = hk * grp + chunk * hc;            // first query head of this block
    const int rows = hc * m;
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int gw = sp * 4 + w, NWH = 4 * S;
    f16* kch = kc + (size_t)hk * max_seq * HD;
    f16* vch = vc + (size_t)hk * max_seq * HD;
    const bool appender = sp == 0 && chunk == 0;
    const int pos = *pos_ptr;
    if (pos < 0 || pos + m > max_seq) return;        // never index the cache out of range (grid-uniform)
    const int Lk = pos + m;

    // ---- rotary of the block's q rows and of the kv head's m new k rows; the new v rows; the appender writes the caches
    auto rot = [&](int i, int ii, float a, float b, float& r0, float& r1) {
        const size_t ro = tab_rows == m ? (size_t)i * tab_stride : (size_t)(pos + i) * tab_stride;
        const float c = cs[ro + ii], s = sn[ro + ii];
        r0 = a * c - b * s;
        r1 = b * c + a * s;
    };
    for (int e = t; e < rows * 64; e += 256) {
        const int r = e >> 6, ii = e & 63, hl = r / m, i = r - hl * m;
        const f16* src = q + (size_t)i * qkv_stride + (size_t)(h0 + hl) * HD;
        float r0, r1;
        rot(i, ii, (float)src[ii], (float)src[ii + 64], r0, r1);
        const float scale = 0.08838834764831845f;   // 1/sqrt(128)
        qs[r * HD + ii] = (f16)(r0 * scale);
        qs[r * HD + ii + 64] = (f16)(r1 * scale);
    }
    for (int e = t; e < R * 64; e += 256)            // rows past `rows`: zero (their scores are masked anyway)
        if ((e >> 6) >= rows) {
            qs[(e >> 6) * HD + (e & 63)] = (f16)0.f;
            qs[(e >> 6) * HD + (e & 63) + 64] = (f16)0.f;
        }
    for (int e = t; e < m * 64; e += 256) {
        const int i = e >> 6, ii = e & 63;
        const f16* src = k + (size_t)i * qkv_stride + (size_t)hk * HD;
        float r0, r1;
        rot(i, ii, (float)src[ii], (float)src[ii + 64], r0, r1);
        const f16 k0 = (f16)r0, k1 = (f16)r1;
        knew[i * HD + ii] = k0;
        knew[i * HD + ii + 64] = k1;
        if (appender) {
            kch[(size_t)(pos + i) * HD + ii] = k0;
            kch[(size_t)(pos + i) * HD + ii + 64] = k1;
        }
    }
    for (int e = t; e < m * HD; e += 256) {
        const int i = e >> 7, d = e & 127;
        const f16 vv = v[(size_t)i * qkv_stride + (size_t)hk * HD + d];
        vnew[i * HD + d] = vv;
        if (appender) vch[(size_t)(pos + i) * HD + d] = vv;
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
    auto load_run = [&](int j) {        // rows < max_seq always (pos + m <= max_seq, max_seq % 16 == 0); rows >= pos replaced below
        const int r0 = j * 16;
#pragma unroll
        for (int c = 0; c < 4; ++c) kr[c] = *(const h8*)(kch + (size_t)(r0 + pj) * HD + qd * 8 + 32 * c);
#pragma unroll
        for (int p = 0; p < 16; ++p) vr[p] = *(const h2*)(vch + (size_t)(r0 + p) * HD + d0);
    };
    int qlim[R];                                     // query row r sees keys <= pos + r % m; padding rows see none
#pragma unroll
    for (int r = 0; r < R; ++r) qlim[r] = r < rows ? pos + r % m : -1;
    int j = gw;
    if (j < nrun) load_run(j);
    for (; j < nrun; j += NWH) {
        const int r0 = j * 16, p = r0 + pj;
        h8 kk[4];
        h2 vv[16];
#pragma unroll
        for (int c = 0; c < 4; ++c) kk[c] = p >= pos ? *(const h8*)(knew + (p - pos < m ? p - pos : 0) * HD + qd * 8 + 32 * c) : kr[c];
#pragma unroll
        for (int e = 0; e < 16; ++e) vv[e] = r0 + e >= pos ? *(const h2*)(vnew + (r0 + e - pos < m ? r0 + e - pos : 0) * HD + d0) : vr[e];
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
            const bool ok = p <= qlim[r];
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
    constexpr int NE = R * HD / 256;                 // (row, dim) pairs per thread
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
    auto store_out = [&](int e, float val) {
        const int r = e >> 7, d = e & 127, hl = r / m, i = r - hl * m, h = h0 + hl;
        const int op = out_pos ? out_pos[h * HD + d] : h * HD + d;
        out[(size_t)i * out_stride + op] = (f16)val;
    };
    if (S == 1) {
#pragma unroll
        for (int u = 0; u < NE; ++u)
            if (t + 256 * u < nel) store_out(t + 256 * u, mrg[u] / mD[u]);
        return;
    }
    // ---- publish this split's records (one per query row: acc[128], max, sum), take a ticket; the last arriver merges
#pragma unroll
    for (int u = 0; u < NE; ++u) {
        const int e = t + 256 * u, r = e >> 7, d = e & 127;
        if (e < nel) {
            const int hl = r / m, i = r - hl * m;
            float* rec = ws + attn_m_ctr_floats(n_heads) + ((size_t)((h0 + hl) * m + i) * S + sp) * kAttnRec;
            st_agent(rec + d, mrg[u]);
            if (d == 0) {
                st_agent(rec + HD, mM[u]);
                st_agent(rec + HD + 1, mD[u]);
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned* ctr = (unsigned*)ws + hkc;
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
            const int hl = r / m, i = r - hl * m;
            const float* r0 = ws + attn_m_ctr_floats(n_heads) + ((size_t)((h0 + hl) * m + i) * S) * kAttnRec;
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

constexpr int kAttnMRows = 32;      // query rows per block (heads of a chunk x m)
// heads of a chunk: the largest divisor of the group with hc * m <= 32
static int attn_m_chunk(int grp, int m) {
    int hc = 1;
    for (int d = 1; d <= grp; ++d)
        if (grp % d == 0 && d * m <= kAttnMRows) hc = d;
    return hc;
}

size_t attn_m_smem_bytes(int R) { return (size_t)R * 128 * 2 + 2 * 8 * 128 * 2 + 4 * R * 16 * 4 + 4 * R * 128 * 4 + 2 * 4 * R * 4; }

size_t attn_m_workspace_bytes(int n_heads, int S, int m) { return S > 1 ? (attn_m_ctr_floats(n_heads) + (size_t)n_heads * m * S * kAttnRec) * 4 : 0; }

hipError_t rope_attn_m_launch(const AttnRowsArgs& a, hipStream_t st) {
    const int grp = a.n_heads / a.n_kv, hc = attn_m_chunk(grp, a.m), rows = hc * a.m;
    const int R = rows <= 8 ? 8 : rows <= 16 ? 16 : 32;
    const size_t smem = attn_m_smem_bytes(R);
    auto go = [&](auto kern) -> hipError_t {
        if (smem > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, dim3(a.n_kv * (grp / hc) * a.S), dim3(256), smem, st, a.pos, a.out_pos, (const f16*)a.q, (const f16*)a.k,
                           (const f16*)a.v, (const float*)a.cs, (const float*)a.sn, (f16*)a.kc, (f16*)a.vc, (f16*)a.out, (float*)a.ws,
                           a.qkv_stride, a.out_stride, a.tab_stride, a.tab_rows, a.max_seq, a.n_heads, a.n_kv, a.S, a.m, hc);
        return hipGetLastError();
    };
    if (R == 8) return go(rope_attn_m_kernel<8>);
    if (R == 16) return go(rope_attn_m_kernel<16>);
    return go(rope_attn_m_kernel<32>);
}

// ---- final RMSNorm + fp16 head, m rows: logits [m][vocab].  The kernel of decode_aux.hip (lm_head_f16_kernel) with the m
// normalised rows in LDS instead of one in registers: every block normalises the rows itself (wave i: row i, the one-row
// kernel's arithmetic), then each wave streams whole head rows, 16 B per lane per load, the next row in flight, and forms the
// m dot products of a row from the same registers (v_dot2_f32_f16, fp32, one DPP wave sum per product).  H = 512 LPR.
template <int LPR>
__global__ __launch_bounds__(512) void lm_head_m_kernel(const float* __restrict__ h32, const f16* __restrict__ gamma,
                                                        const f16* __restrict__ W, f16* __restrict__ logits, int vocab, float eps,
                                                        int rows_per_block, int m) {
    constexpr int H = 512 * LPR;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
    h8* const xs = (h8*)smem_raw;                    // [m][LPR][64 lanes] normalised rows, in the lanes' own order
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (wave < m) {
        const float* hr = h32 + (size_t)wave * H;
        float xv[LPR][8];
        float ss = 0.f;
#pragma unroll
        for (int c = 0; c < LPR; ++c) {
            const f32x4 a = *(const f32x4*)(hr + c * 512 + lane * 8), b = *(const f32x4*)(hr + c * 512 + lane * 8 + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                xv[c][j] = a[j];
                xv[c][4 + j] = b[j];
                ss += a[j] * a[j] + b[j] * b[j];
            }
        }
        ss = wave_sum(ss);
        const float rs = rsqrtf(ss / (float)H + eps);
#pragma unroll
        for (int c = 0; c < LPR; ++c) {
            const h8 g = *(const h8*)(gamma + c * 512 + lane * 8);
            h8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = mul_f32_to_f16(xv[c][j] * rs, (float)g[j]);
            xs[((size_t)wave * LPR + c) * 64 + lane] = o;
        }
    }
    __syncthreads();
    const int r_end = min(vocab, (int)(blockIdx.x + 1) * rows_per_block);
    int r = blockIdx.x * rows_per_block + wave;
    u32x4 cur[LPR], nxt[LPR];
    auto load_row = [&](int row, u32x4 (&dst)[LPR]) {
        const u32x4* p = (const u32x4*)(W + (size_t)min(row, vocab - 1) * H) + lane;      // clamped: never out of range
#pragma unroll
        for (int c = 0; c < LPR; ++c) dst[c] = __builtin_nontemporal_load(p + c * 64);
    };
    load_row(r, cur);
    for (; r < r_end; r += 8) {
        load_row(r + 8, nxt);
        for (int i = 0; i < m; ++i) {
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < LPR; ++c) {
                const u32x4 xw = __builtin_bit_cast(u32x4, xs[((size_t)i * LPR + c) * 64 + lane]);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_fdot2(as_h2(cur[c][j]), as_h2(xw[j]), acc, false);
            }
            acc = wave_sum(acc);
            if (lane == 0) logits[(size_t)i * vocab + r] = (f16)acc;
        }
#pragma unroll
        for (int c = 0; c < LPR; ++c) cur[c] = nxt[c];
    }
}

hipError_t lm_head_m_launch(const void* h32, const void* gamma, const void* W, void* logits, int H, int vocab, float eps, int m,
                            hipStream_t st) {
    const int blocks = vocab >= 4096 ? 512 : (vocab + 7) / 8, rpb = (vocab + blocks - 1) / blocks;
    const size_t smem = (size_t)m * H * 2;
    auto go = [&](auto kern) -> hipError_t {
        if (smem > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(512), smem, st, (const float*)h32, (const f16*)gamma, (const f16*)W, (f16*)logits,
                           vocab, eps, rpb, m);
        return hipGetLastError();
    };
    switch (H) {
        case 512: return go(lm_head_m_kernel<1>);
        case 1024: return go(lm_head_m_kernel<2>);
        case 2048: return go(lm_head_m_kernel<4>);
        case 4096: return go(lm_head_m_kernel<8>);
        case 5120: return go(lm_head_m_kernel<10>);
        case 8192: return go(lm_head_m_kernel<16>);
        default: return hipErrorInvalidValue;
    }
}

// ---- greedy verify.  One block of 1024.  am[i] = argmax of logits row i (lowest index among equal maxima, as token_end);
// n = the longest prefix with am[i] == tokens[i + 1]; out_tokens[0..n] = tokens[1..n], am[n]; *n_acc = n; *tok = am[n];
// *pos += n + 1.  greedy == 0: *pos += m only (teacher-forced rows).
__global__ __launch_bounds__(1024) void verify_greedy_kernel(const f16* __restrict__ logits, const long long* __restrict__ tokens,
                                                             int m, int vocab, int greedy, long long* __restrict__ out_tokens,
                                                             int* __restrict__ n_acc, long long* __restrict__ tok, int* __restrict__ pos) {
    __shared__ float bv[16];
    __shared__ int bi[16];
    __shared__ int am[8];
    const int t = threadIdx.x;
    if (!greedy) {
        if (t == 0) *pos = *pos + m;
        return;
    }
    for (int row = 0; row < m; ++row) {
        const int a = block_argmax_1024(logits + (size_t)row * vocab, vocab, bv, bi);
        if (t == 0) am[row] = a;
        __syncthreads();
    }
    if (t == 0) {
        int n = 0;
        while (n < m - 1 && (long long)am[n] == tokens[n + 1]) {
            out_tokens[n] = tokens[n + 1];
            ++n;
        }
        out_tokens[n] = am[n];
        *n_acc = n;
        *tok = am[n];
        *pos = *pos + n + 1;
    }
}

hipError_t verify_greedy_launch(const void* logits, const void* tokens, int m, int vocab, int greedy, void* out_tokens, int* n_acc,
                                void* tok, int* pos, hipStream_t st) {
    hipLaunchKernelGGL(verify_greedy_kernel, dim3(1), dim3(1024), 0, st, (const f16*)logits, (const long long*)tokens, m, vocab, greedy,
                       (long long*)out_tokens, n_acc, (long long*)tok, pos);
    return hipGetLastError();
}

}  // namespace qeft
