// The row-owned GPTQ loop (calibrate.gptq_reorder(loop="rows")): every 128-column block of the
// error-feedback loop, the trailing updates and the block-start parameters in ONE launch.  The contract, the split of the work,
// the three phases of a tile and the bounds of every address: calib_rows.h.  Nothing below may be contracted into an FMA (the
// pinned lines of calib.h), hence the pragma over the whole file; the divisions are IEEE (the compiler's default for fp32).
#include <math.h>

#include "qeft_common.h"
#include "calib_mse.h"
#include "calib_rows.h"
#include "quant_pack.h"

#pragma clang fp contract(off)

namespace qeft {

// Steps I .. 127 of the serial sweep, unrolled by recursion so that the row stays in registers and every register index, lane
// index and LDS offset is a constant (a 128-step loop is past the size at which the unroll pragma is obeyed); a column >= count
// is skipped by a uniform branch.  The lines are calib.h's; all 16 lanes of a row compute the same q and e, the owner keeps them.
template <int I>
__device__ __forceinline__ void gr_sweep(float (&w)[8], float (&qv)[8], float (&ev)[8], const float* Hs, float s, float z, float maxq,
                                         int count, int lane, int c) {
    if constexpr (I < GR_B) {
        constexpr int m = I >> 4, o = I & 15;
        if (I < count) {
            const float wi = __shfl(w[m], (lane & 48) | o);
            const float d = Hs[I * GR_B + I];
            const float xs = wi / s;
            const float cc = fminf(fmaxf(rintf(xs) + z, 0.f), maxq);
            const float q = s * (cc - z);
            const float e = (wi - q) / d;
            if (c == o) {
                qv[m] = q;
                ev[m] = e;
            }
#pragma unroll
            for (int mm = m; mm < 8; ++mm)
                if (mm > m || c >= o) {
                    const float p = e * Hs[I * GR_B + c + 16 * mm];
                    w[mm] = w[mm] - p;
                }
        }
        gr_sweep<I + 1>(w, qv, ev, Hs, s, z, maxq, count, lane, c);
    }
}

// The reduce-scatter of the in-launch search, steps lane ^ OFF, OFF / 2, .., 1 (recursion: every register index a constant).  A
// step with OFF < LPR halves the zero points a lane still carries -- lanes with bit OFF keep the upper half -- and adds the
// partner's partial of each kept one; a step with OFF >= LPR (3 bits, lane ^ 8) is a plain exchange-and-add, the same bits on
// both sides.  Afterwards p[0] of lane c is the row's score of zero point c % LPR.
template <int LPR, int OFF>
__device__ __forceinline__ void gr_scatter(float (&p)[LPR], int c) {
    if constexpr (OFF >= 1) {
        if constexpr (OFF < LPR) {
            const bool up = (c & OFF) != 0;
#pragma unroll
            for (int v = 0; v < OFF; ++v) {
                const float keep = up ? p[v + OFF] : p[v], send = up ? p[v] : p[v + OFF];
                p[v] = keep + __shfl_xor(send, OFF);
            }
        } else {
#pragma unroll
            for (int v = 0; v < LPR; ++v) p[v] = p[v] + __shfl_xor(p[v], OFF);
        }
        gr_scatter<LPR, OFF / 2>(p, c);
    }
}

// The row's scores of ONE range of the search over the lane's 8 columns x (a column outside the live ones enters as 0: its
// x_round is 0, no zero point clamps it, d is exactly 0 and its term +0, which leaves every sum's bits).  The lane's partial scores
// of all 2^BITS zero points stay in registers (8 columns, m ascending); a reduce-scatter over lane ^ 8, 4, 2, 1 then leaves lane c
// with the row's score of zero point c % 2^BITS (at 3 bits the first step is a plain exchange-and-add, so lanes c and c ^ 8 hold
// the same bits).  Shared by the per-tile search (gr_mse_pair) and the per-channel one (gr_pc_mse_pair): the order of a tile's sum.
template <int BITS>
__device__ __forceinline__ float gr_mse_score(const float (&x)[8], float delta, int c) {
    constexpr int LPR = 1 << BITS;
    constexpr float MAXQ = (float)(LPR - 1);
    // the zero point of candidate c % LPR, by the pinned lines: one division per lane, read by the row's lanes below
    const float new_min = 0.f - (float)(c & (LPR - 1)) * delta;
    const float zero_own = ms_clamp(0.f - rintf(new_min / delta), MAXQ);
    float xr[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) xr[m] = rintf(x[m] / delta);
    float p[LPR];
#pragma unroll
    for (int zp = 0; zp < LPR; ++zp) {
        const float zero = __shfl(zero_own, zp, 16);
        // clamp(x_round + zero, 0, maxq) - zero == clamp(x_round, -zero, maxq - zero): x_round itself inside the window (small
        // integers, exact; -0 for +0 leaves d), and the same bound outside it, however large x_round is
        const float k_lo = 0.f - zero, k_hi = MAXQ - zero;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const float x_q = delta * __builtin_amdgcn_fmed3f(xr[m], k_lo, k_hi);
            const float term = ms_term(x[m] - x_q);
            p[zp] = m == 0 ? term : p[zp] + term;
        }
    }
    gr_scatter<LPR, 8>(p, c);
    return p[0];
}

// The end of a search: each lane holds the first minimum over i of its zero point as (best, key = i 2^BITS + zp; 0: no candidate
// scored below infinity).  One 16-lane arg-min on (score, key) gives the first minimum in the order (i, zp), the same in all 16
// lanes; every lane then forms the pair from the winning key by the closing lines.
template <int BITS>
__device__ __forceinline__ void gr_mse_close(float best, int key, float step, float xmin, float xmax, float& s, float& z) {
    constexpr int LPR = 1 << BITS;
    constexpr float MAXQ = (float)(LPR - 1);
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
        const float ob = __shfl_xor(best, off);
        const int ok = __shfl_xor(key, off);
        if (ob < best || (ob == best && ok < key)) {
            best = ob;
            key = ok;
        }
    }
    float best_min = xmin, best_max = xmax;                 // the reference's initial pair
    if (key != 0) {
        const float tmp_max = step * (float)(key >> BITS);
        const float delta = fmaxf(tmp_max / MAXQ, MS_EPS);
        const float zd = (float)(key & (LPR - 1)) * delta;
        best_min = 0.f - zd;
        best_max = tmp_max - zd;
    }
    const float mn = fminf(best_min, 0.f), mx = fmaxf(best_max, 0.f);
    s = fmaxf((mx - mn) / MAXQ, MS_EPS);
    z = ms_clamp(0.f - rintf(mn / s), MAXQ);
}

// The MSE search of one tile (qeft_gptq_rows_mse; the contract and the order of every sum: calib_rows.h), between phase 2 and the
// sweep, in registers and cross-lane reads alone: no LDS, no barrier, no global address.  w: the lane's 8 block-start columns
// c + 16 m; xmin / xmax: the row's extremes over the live columns and 0, the same bits in the row's 16 lanes.  Per range i one
// gr_mse_score; the lane keeps the first minimum over i of its zero point, gr_mse_close ends the search.
template <int BITS>
__device__ __forceinline__ void gr_mse_pair(const float (&w)[8], int count, int c, int num, float xmin, float xmax, float& s,
                                            float& z) {
    constexpr int LPR = 1 << BITS;
    constexpr float MAXQ = (float)(LPR - 1);
    float x[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) x[m] = c + 16 * m < count ? w[m] : 0.f;
    const float step = (xmax - xmin) / (float)num;          // xrange / num; tmp_max = step * i
    float best = INFINITY;
    int key = 0;
#pragma unroll 1
    for (int i = 1; i <= num; ++i) {
        const float tmp_max = step * (float)i;
        const float delta = fmaxf(tmp_max / MAXQ, MS_EPS);
        const float sc = gr_mse_score<BITS>(x, delta, c);
        if (sc < best) {                                    // strict: the first i among equal scores
            best = sc;
            key = i * LPR + (c & (LPR - 1));
        }
    }
    gr_mse_close<BITS>(best, key, step, xmin, xmax, s, z);
}

// The per-channel MSE search of phase 0 (qeft_gptq_rows_pc_mse; calib_rows.h): the same candidates over the row's WHOLE live
// width, nn columns of W0 in tiles of 128.  Tiles outer, ranges inner: per (tile, range) one gr_mse_score, whose result lane c
// adds into its own running score slots[(i - 1) * GR_THREADS] -- a table [num][256] in LDS, a lane's slots its own alone (no
// barrier in here, no bank conflict: a wave's 64 lanes touch 64 consecutive words), so no score lives in an indexed register.
// A score is therefore: the tile sum in gr_mse_score's order, then tiles ascending.  The lane then walks its slots, i ascending.
template <int BITS>
__device__ __forceinline__ void gr_pc_mse_pair(const float* __restrict__ wrow, float* slots, int nn, int c, int num, float xmin,
                                               float xmax, float& s, float& z) {
    constexpr int LPR = 1 << BITS;
    constexpr float MAXQ = (float)(LPR - 1);
    const float step = (xmax - xmin) / (float)num;
    for (int cb = 0; cb < nn; cb += GR_B) {
        float x[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) x[m] = cb + c + 16 * m < nn ? wrow[cb + c + 16 * m] : 0.f;
#pragma unroll 1
        for (int i = 1; i <= num; ++i) {
            const float tmp_max = step * (float)i;
            const float delta = fmaxf(tmp_max / MAXQ, MS_EPS);
            const float sc = gr_mse_score<BITS>(x, delta, c);
            float* slot = slots + (i - 1) * GR_THREADS;
            *slot = cb == 0 ? sc : *slot + sc;
        }
    }
    float best = INFINITY;
    int key = 0;
#pragma unroll 1
    for (int i = 1; i <= num; ++i) {
        const float sc = slots[(i - 1) * GR_THREADS];
        if (sc < best) {                                    // strict: the first i among equal scores
            best = sc;
            key = i * LPR + (c & (LPR - 1));
        }
    }
    gr_mse_close<BITS>(best, key, step, xmin, xmax, s, z);
}

// MSE: 0 = the min-max pair (qeft_gptq_rows), 3 / 4 = the search at that width over `num` ranges (qeft_gptq_rows_mse).
// PC: per-channel (qeft_gptq_rows_pc / _pc_mse) -- ONE pair per row, found in phase 0 from W0's live columns before tile 0;
// scale and zero are then [n], phase 2 searches nothing and every tile's sweep runs with the row's pair.
// Err is read AND written (by other threads of the workgroup, a tile earlier): no __restrict__ on it.
template <int MSE, bool PC>
__global__ __launch_bounds__(GR_THREADS) void gptq_rows_kernel(const float* __restrict__ W0, const float* __restrict__ U,
                                                               float* __restrict__ Q, float* Err, float* __restrict__ scale,
                                                               float* __restrict__ zero, GrGeom G, float maxq, int num) {
    extern __shared__ __attribute__((aligned(16))) float gr_smem[];
    float* Us = gr_smem;                                    // [2][32][GR_LDU]   chunks of U[0:depth, tile]
    float* Es = Us + 2 * GR_BK * GR_LDU;                    // [2][16][GR_LDE]   chunks of Err[rows, 0:depth]
    float* Cs = Es + 2 * GR_ROWS * GR_LDE;                  // [16][GR_LDC]      the accumulators on their way to the sweep's layout
    float* Hs = Cs + GR_ROWS * GR_LDC;                      // [128][128]        the diagonal block, zeros below the diagonal
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ml = lane & 15, mg = lane >> 4;               // the matrix unit's view: A row / B column ml, k mg of a step's 4
    const int srow = tid >> 4, c = tid & 15;                // the sweep's view (and the Err staging's): row srow, columns c + 16 m
    const int ur = tid >> 5, uc4 = tid & 31;                // the U staging's: chunk rows ur + 8 p, columns 4 uc4 .. + 3
    const int row = blockIdx.x * GR_ROWS + srow;
    const bool live = row < G.n;
    const int rc = live ? row : G.n - 1;                    // a thread past n repeats the last row and stores nothing
    const int ng = G.k / GR_B, nn = G.n_nonout;
    const float* wrow = W0 + (size_t)rc * G.ld_w;
    float* qrow = Q + (size_t)rc * G.k;
    float* erow = Err + (size_t)rc * nn;
    float s = 1.f, z = 0.f;                                 // the last live group's pair (every call has a live tile 0)

    if constexpr (PC) {
        // ---- phase 0: the row's one pair, from W0's live columns (c + 16 m of every live tile) before any feedback
        float lo = 0.f, hi = 0.f;                           // min and max do not round: any order gives the row's
        for (int cb = 0; cb < nn; cb += GR_B)
#pragma unroll
            for (int m = 0; m < 8; ++m)
                if (cb + c + 16 * m < nn) {
                    const float v = wrow[cb + c + 16 * m];
                    lo = fminf(lo, v);
                    hi = fmaxf(hi, v);
                }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {            // the row's 16 lanes
            lo = fminf(lo, __shfl_xor(lo, off));
            hi = fmaxf(hi, __shfl_xor(hi, off));
        }
        if constexpr (MSE == 0) {
            qp_minmax_pair<true>(lo, hi, maxq, s, z);
        } else {
            // the score table [num][256] lies over Us and Es (GR_PC_TABLE_FLOATS <= their size), idle until tile 1's phase 1
            gr_pc_mse_pair<MSE>(wrow, gr_smem + tid, nn, c, num, lo, hi, s, z);
            __syncthreads();                                // every lane is done with its slots before the region is staged into
        }
        if (live && c == 0) {
            scale[row] = s;
            zero[row] = z;
        }
    }

    for (int t = 0; t < ng; ++t) {
        const int cb = t * GR_B;
        const int count = min(max(nn - cb, 0), GR_B);       // live columns of the tile: the serial phase runs over them
        const bool sweep = count > 0;
        const int depth = sweep ? cb : nn;                  // rows of Err . U that are already final
        const int nch = (depth + GR_BK - 1) / GR_BK;

        float w[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) w[m] = wrow[cb + c + 16 * m];

        // ---- phase 1: acc = Err[rows, 0:depth] . U[0:depth, tile]
        f32x4 acc[2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) acc[sub] = f32x4{0.f, 0.f, 0.f, 0.f};
        float4 ru[4], rt[4];
        float2 re;
        auto load = [&](int kc) {
            const int k0 = kc * GR_BK;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int kr = k0 + ur + 8 * p;
                ru[p] = kr < depth ? *(const float4*)(U + (size_t)kr * G.ld_h + cb + 4 * uc4) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            const int ke = k0 + 2 * c;                      // depth is even: the pair is inside or outside as one
            re = ke < depth ? *(const float2*)(erow + ke) : make_float2(0.f, 0.f);
        };
        auto stage = [&](int kc) {
            float* ub = Us + (kc & 1) * GR_BK * GR_LDU;
#pragma unroll
            for (int p = 0; p < 4; ++p) *(float4*)(ub + (ur + 8 * p) * GR_LDU + 4 * uc4) = ru[p];
            *(float2*)(Es + (kc & 1) * GR_ROWS * GR_LDE + srow * GR_LDE + 2 * c) = re;
        };
        // piece tp of the diagonal block: rows 32 tp + ur + 8 p
        auto tri_load = [&](int tp) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int i = 32 * tp + ur + 8 * p;
                rt[p] = *(const float4*)(U + (size_t)(cb + i) * G.ld_h + cb + 4 * uc4);
            }
        };
        auto tri_store = [&](int tp) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int i = 32 * tp + ur + 8 * p, j = 4 * uc4;
                *(float4*)(Hs + i * GR_B + j) = make_float4(j >= i ? rt[p].x : 0.f, j + 1 >= i ? rt[p].y : 0.f,
                                                            j + 2 >= i ? rt[p].z : 0.f, j + 3 >= i ? rt[p].w : 0.f);
            }
        };

        int tp = sweep ? 0 : 4;                             // an outlier tile has no serial phase and needs no triangle
        if (nch > 0) load(0);
        for (int kc = 0; kc < nch; ++kc) {
            stage(kc);                                      // buffer kc & 1: everyone left it before the barrier of chunk kc - 1
            if (kc + 1 < nch) load(kc + 1);                 // in flight behind this chunk's MFMAs
            if (tp < 4) tri_load(tp);
            __syncthreads();
            const float* ub = Us + (kc & 1) * GR_BK * GR_LDU + mg * GR_LDU + 32 * wave + ml;
            const float* eb = Es + (kc & 1) * GR_ROWS * GR_LDE + ml * GR_LDE + mg;
#pragma unroll
            for (int st = 0; st < GR_BK / 4; ++st) {
                const float a = eb[4 * st];
                const float b0 = ub[4 * st * GR_LDU], b1 = ub[4 * st * GR_LDU + 16];
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc[1], 0, 0, 0);
            }
            if (tp < 4) {
                tri_store(tp);
                ++tp;
            }
        }
        for (; tp < 4; ++tp) {                              // tile 0: no chunk to ride on
            tri_load(tp);
            tri_store(tp);
        }

        // ---- phase 2: the accumulators into the sweep's layout; w = W0 - acc
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int r = 0; r < 4; ++r) Cs[(4 * mg + r) * GR_LDC + 32 * wave + 16 * sub + ml] = acc[sub][r];
        __syncthreads();                                    // Cs, and every piece of Hs
#pragma unroll
        for (int m = 0; m < 8; ++m) w[m] = w[m] - Cs[srow * GR_LDC + c + 16 * m];

        if (sweep) {
            if constexpr (!PC) {
                float lo = 0.f, hi = 0.f;                   // min and max do not round: any order gives the row's
#pragma unroll
                for (int m = 0; m < 8; ++m)
                    if (c + 16 * m < count) {
                        lo = fminf(lo, w[m]);
                        hi = fmaxf(hi, w[m]);
                    }
#pragma unroll
                for (int off = 1; off < 16; off <<= 1) {    // the row's 16 lanes
                    lo = fminf(lo, __shfl_xor(lo, off));
                    hi = fmaxf(hi, __shfl_xor(hi, off));
                }
                if constexpr (MSE == 0)
                    qp_minmax_pair<true>(lo, hi, maxq, s, z);     // the block route's bits: torch's own lines on the device
                else
                    gr_mse_pair<MSE>(w, count, c, num, lo, hi, s, z);
            }

            // ---- phase 3: the serial sweep
            float qv[8], ev[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) qv[m] = ev[m] = 0.f;
            gr_sweep<0>(w, qv, ev, Hs, s, z, maxq, count, lane, c);
            if (live) {
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    const int j = c + 16 * m;
                    if (j < count) {
                        qrow[cb + j] = qv[m];
                        erow[cb + j] = ev[m];
                    } else {
                        qrow[cb + j] = w[m];                // an outlier column that shares the tile: W0 - Err . U, complete
                    }
                }
            }
        } else if (live) {
#pragma unroll
            for (int m = 0; m < 8; ++m) qrow[cb + c + 16 * m] = w[m];
        }
        if (!PC && live && c == 0) {                        // a tile without a live column repeats the last pair
            scale[(size_t)row * ng + t] = s;
            zero[(size_t)row * ng + t] = z;
        }
        __syncthreads();                                    // the tile's err is stored and visible; Us, Es, Cs, Hs are free
    }
}

template <int MSE, bool PC = false>
static hipError_t gr_launch(const char* variant, const void* w0, const void* hinv, void* q, void* err, void* scale, void* zero,
                            const GrGeom& G, float maxq, int num, hipStream_t st) {
    g_last_variant = variant;
    if (hipError_t e = hipFuncSetAttribute((const void*)gptq_rows_kernel<MSE, PC>, hipFuncAttributeMaxDynamicSharedMemorySize, GR_LDS))
        return e;
    hipLaunchKernelGGL((gptq_rows_kernel<MSE, PC>), dim3((unsigned)gr_blocks(G)), dim3(GR_THREADS), GR_LDS, st, (const float*)w0,
                       (const float*)hinv, (float*)q, (float*)err, (float*)scale, (float*)zero, G, maxq, num);
    return hipGetLastError();
}

hipError_t gptq_rows_launch(const void* w0, const void* hinv, void* q, void* err, void* scale, void* zero, const GrGeom& G,
                            float maxq, hipStream_t st) {
    return gr_launch<0>("gptq_rows_16", w0, hinv, q, err, scale, zero, G, maxq, 0, st);
}

hipError_t gptq_rows_mse_launch(const void* w0, const void* hinv, void* q, void* err, void* scale, void* zero, const GrGeom& G,
                                int bits, int num, hipStream_t st) {
    if (bits == 4) return gr_launch<4>("gptq_rows_mse_w4", w0, hinv, q, err, scale, zero, G, 15.f, num, st);
    return gr_launch<3>("gptq_rows_mse_w3", w0, hinv, q, err, scale, zero, G, 7.f, num, st);
}

hipError_t gptq_rows_pc_launch(const void* w0, const void* hinv, void* q, void* err, void* scale, void* zero, const GrGeom& G,
                               float maxq, hipStream_t st) {
    return gr_launch<0, true>("gptq_rows_pc", w0, hinv, q, err, scale, zero, G, maxq, 0, st);
}

hipError_t gptq_rows_pc_mse_launch(const void* w0, const void* hinv, void* q, void* err, void* scale, void* zero, const GrGeom& G,
                                   int bits, int num, hipStream_t st) {
    if (bits == 4) return gr_launch<4, true>("gptq_rows_pc_mse_w4", w0, hinv, q, err, scale, zero, G, 15.f, num, st);
    return gr_launch<3, true>("gptq_rows_pc_mse_w3", w0, hinv, q, err, scale, zero, G, 7.f, num, st);
}

}  // namespace qeft
