// The training update: two launches over the flat fp32 oweight arena of qeft_amd/optim.py.
//
//   launch 1  oweight_grad_stats_kernel   one fp32 sum of squares of the unscaled gradient per block -> partials
//   launch 2  oweight_adamw_kernel        every block folds the partials in double in index order (the same bits everywhere),
//                                         forms the clip coefficient and either skips (a non-finite sum: no element is touched,
//                                         the scale backs off) or applies clipped AdamW; block 0 writes the next state record
//
// Plain streaming: 16-byte accesses, OO_U chunks per thread issued before their first use, a fixed grid stride, no atomics, no
// hand-off between workgroups, no host synchronisation.  The arithmetic is pinned as oweight_optim.h states it: nothing below may
// be contracted into an FMA, hence the pragma over the whole file.
//
// Every global address comes from oweight_optim.h; oweight_optim_count_out_of_range walks the same functions on the CPU.
#include "qeft_common.h"
#include "oweight_optim.h"

#pragma clang fp contract(off)

namespace qeft {

// ---------------------------------------------------------------- launch 1: sum of squares of g / scale, one partial per block
template <int U>
__global__ __launch_bounds__(OO_THREADS) void oweight_grad_stats_kernel(const float* __restrict__ g, long long n,
                                                                        const OoState* __restrict__ state_in,
                                                                        float* __restrict__ partials) {
    __shared__ float sm[4];
    const OoGeom G{n, U};
    const long long chunks = oo_chunks(G);
    const int iters = oo_iters(G), tid = threadIdx.x;
    const float inv = 1.0f / state_in->scale;
    float acc = 0.f;
    for (int it = 0; it < iters; ++it) {
        f32x4 x[U];
#pragma unroll
        for (int s = 0; s < U; ++s) {
            const long long ch = oo_chunk(G, blockIdx.x, tid, it, s);
            x[s] = ch < chunks ? *(const f32x4*)(g + oo_off(ch)) : f32x4{0.f, 0.f, 0.f, 0.f};       // + 0 * 0 changes no bit
        }
#pragma unroll
        for (int s = 0; s < U; ++s)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float t = x[s][j] * inv;
                acc = acc + t * t;
            }
    }
    // a fixed tree: the butterfly within the wave (6 levels, every lane ends with the same bits), then the four waves
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc = acc + __shfl_xor(acc, o);
    if ((tid & 63) == 0) sm[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) partials[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// beta^t in double by repeated squaring: at most 31 squarings, a few ulp of double
__device__ __forceinline__ double oo_powi(double b, int t) {
    double r = 1.0;
    while (t > 0) {
        if (t & 1) r *= b;
        b *= b;
        t >>= 1;
    }
    return r;
}

template <bool NT>
__device__ __forceinline__ f32x4 oo_load_g(const float* p) {
    if constexpr (NT) return __builtin_nontemporal_load((const f32x4*)p);
    else return *(const f32x4*)p;
}

// ---------------------------------------------------------------- launch 2: clip + AdamW, or the skip
template <int U, bool NT>
__global__ __launch_bounds__(OO_THREADS) void oweight_adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                   float* __restrict__ m, float* __restrict__ v, long long n,
                                                                   const OoState* __restrict__ state_in, OoState* __restrict__ state_out,
                                                                   const float* __restrict__ partials, OoHyper H) {
    const OoGeom G{n, U};
    const int nblocks = oo_blocks(G), tid = threadIdx.x;
    const OoState S = *state_in;
    double sum = 0.0;
    for (int b = 0; b < nblocks; ++b) sum += (double)partials[b];         // uniform: the same order, the same bits, in every thread
    if (!(fabs(sum) <= 1.79769313486231570e308)) {                         // inf or NaN: an overflowed or poisoned gradient
        if (blockIdx.x == 0 && tid == 0) {
            OoState O = S;
            O.good_steps = 0;
            O.skipped_last = 1;
            O.n_skipped = S.n_skipped + 1;
            if (H.dynamic) O.scale = S.scale * H.backoff_factor;
            *state_out = O;
        }
        return;
    }
    const float norm = (float)sqrt(sum);
    const float coef = H.max_norm > 0.f ? fminf(1.f, H.max_norm / (norm + 1e-6f)) : 1.f;
    const int t = S.step + 1;
    const double bc1 = 1.0 - oo_powi((double)H.beta1, t), bc2 = 1.0 - oo_powi((double)H.beta2, t);
    const float a = (float)((double)H.lr / bc1), r = (float)sqrt(bc2);
    const float inv = 1.0f / S.scale, decay = 1.f - H.lr * H.weight_decay, c1 = 1.f - H.beta1, c2 = 1.f - H.beta2;
    const float beta2 = H.beta2, eps = H.eps;
    if (blockIdx.x == 0 && tid == 0) {
        OoState O = S;
        O.step = t;
        O.good_steps = S.good_steps + 1;
        O.skipped_last = 0;
        O.grad_norm = norm;
        O.clip_coef = coef;
        if (H.dynamic && O.good_steps >= H.growth_interval) {
            O.scale = S.scale * H.growth_factor;
            O.good_steps = 0;
        }
        *state_out = O;
    }
    const long long chunks = oo_chunks(G);
    const int iters = oo_iters(G);
    for (int it = 0; it < iters; ++it) {
        f32x4 pp[U], gg[U], mm[U], vv[U];
        long long off[U];
        bool live[U];
#pragma unroll
        for (int s = 0; s < U; ++s) {
            const long long ch = oo_chunk(G, blockIdx.x, tid, it, s);
            live[s] = ch < chunks;
            off[s] = oo_off(ch);
            if (live[s]) {
                gg[s] = oo_load_g<NT>(g + off[s]);
                pp[s] = *(const f32x4*)(p + off[s]);
                mm[s] = *(const f32x4*)(m + off[s]);
                vv[s] = *(const f32x4*)(v + off[s]);
            }
        }
#pragma unroll
        for (int s = 0; s < U; ++s) {
            if (!live[s]) continue;
            f32x4 po, mo, vo;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float x = gg[s][j] * inv;
                const float gh = x * coef;
                const float p1 = pp[s][j] * decay;
                const float d = gh - mm[s][j];
                const float m1 = mm[s][j] + d * c1;
                const float sq = gh * gh;
                const float v1 = beta2 * vv[s][j] + c2 * sq;
                const float den = sqrtf(v1) / r + eps;
                const float q = m1 / den;
                po[j] = p1 - a * q;
                mo[j] = m1;
                vo[j] = v1;
            }
            *(f32x4*)(p + off[s]) = po;
            *(f32x4*)(m + off[s]) = mo;
            *(f32x4*)(v + off[s]) = vo;
        }
    }
}

// ---------------------------------------------------------------- launchers
hipError_t oweight_grad_stats_launch(const void* g, const OoGeom& G, const void* state_in, void* partials, hipStream_t st) {
    const dim3 grid((unsigned)oo_blocks(G)), block(OO_THREADS);
    g_last_variant = G.u == 1 ? "oweight_grad_stats_u1" : G.u == 2 ? "oweight_grad_stats_u2" : "oweight_grad_stats_u4";
#define OO_STATS(U) \
    hipLaunchKernelGGL(oweight_grad_stats_kernel<U>, grid, block, 0, st, (const float*)g, G.n, (const OoState*)state_in, (float*)partials)
    if (G.u == 1) OO_STATS(1);
    else if (G.u == 2) OO_STATS(2);
    else OO_STATS(4);
#undef OO_STATS
    return hipGetLastError();
}

hipError_t oweight_adamw_launch(void* p, const void* g, void* m, void* v, const OoGeom& G, const void* state_in, void* state_out,
                                const void* partials, const OoHyper& H, bool nontemporal_g, hipStream_t st) {
    const dim3 grid((unsigned)oo_blocks(G)), block(OO_THREADS);
    g_last_variant = G.u == 1 ? (nontemporal_g ? "oweight_adamw_u1_nt" : "oweight_adamw_u1")
                   : G.u == 2 ? (nontemporal_g ? "oweight_adamw_u2_nt" : "oweight_adamw_u2")
                              : (nontemporal_g ? "oweight_adamw_u4_nt" : "oweight_adamw_u4");
#define OO_ADAMW(U, NT)                                                                                                       \
    hipLaunchKernelGGL((oweight_adamw_kernel<U, NT>), grid, block, 0, st, (float*)p, (const float*)g, (float*)m, (float*)v, G.n, \
                       (const OoState*)state_in, (OoState*)state_out, (const float*)partials, H)
    if (G.u == 1) { if (nontemporal_g) OO_ADAMW(1, true); else OO_ADAMW(1, false); }
    else if (G.u == 2) { if (nontemporal_g) OO_ADAMW(2, true); else OO_ADAMW(2, false); }
    else { if (nontemporal_g) OO_ADAMW(4, true); else OO_ADAMW(4, false); }
#undef OO_ADAMW
    return hipGetLastError();
}

// ---------------------------------------------------------------- address enumeration (host)
// How many of the 16-byte accesses a launch forms fall outside [0, n), over every thread of every block of every iteration, plus
// the chunks of the arena that are not visited exactly once (a hole or an overlap in the map is as wrong as a stray address).
// Both launches form the same addresses in g; launch 2 forms them in p, m and v too; block b touches partials[b], b < blocks.
long long oweight_optim_count_out_of_range(const OoGeom& G) {
    const long long chunks = oo_chunks(G);
    long long bad = 0, visited = 0, prev_end = 0;
    bool in_order = true;
    // the map is monotone in (it, block, s, tid): walking it in that order must enumerate 0, 1, 2, ... without a gap
    for (int it = 0; it < oo_iters(G); ++it)
        for (int block = 0; block < oo_blocks(G); ++block)
            for (int s = 0; s < G.u; ++s)
                for (int tid = 0; tid < OO_THREADS; ++tid) {
                    const long long ch = oo_chunk(G, block, tid, it, s);
                    if (ch >= chunks) continue;                            // the kernels' own guard
                    const long long off = oo_off(ch);
                    if (off < 0 || off + 4 > G.n) ++bad;
                    if (ch != prev_end) in_order = false;
                    prev_end = ch + 1;
                    ++visited;
                }
    if (!in_order || visited != chunks) bad += 1 + (visited > chunks ? visited - chunks : chunks - visited);
    return bad;
}

}  // namespace qeft
