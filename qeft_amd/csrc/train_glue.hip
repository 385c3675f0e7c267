// The glue of a training step between the linears, attention and the head: RMSNorm with the residual
// add in front of it and SiLU(gate) * up -- forwards over a [B T] batch of rows and a backward for each.
// finetune.causal_lm_loss(glue="fused") runs them through qeft_amd/glue.py; decode_aux.hip keeps the inference forms.
//
// All of them are memory-bound row kernels: 16-byte loads and stores, fp32 math, every output rounded to fp16 exactly once, no
// atomics, no workspace, nothing saved between forward and backward beyond the operands themselves.  A row's results depend on
// that row's operands alone, bit for bit: a norm row is one block with a fixed reduction order, a SwiGLU chunk is one lane's
// work.  The forwards reproduce the arithmetic of qeft_rmsnorm and qeft_silu_mul (decode_aux.hip) operation for operation, so
// their bits are those kernels' bits.  The rotary of q and k (rope_qk_kernel, section 4.17; finetune.causal_lm_loss(rope="fused"))
// is the exception to "rounded once": it owes the torch expression of finetune._rope bit equality and rounds where that does.
//
// Every global address comes from train_glue.h; train_glue_count_out_of_range below walks the same functions on the CPU.
#include "qeft_common.h"
#include "train_glue.h"

namespace qeft {

// decode_aux.hip's block_sum_256, order for order: the forward norm must give qeft_rmsnorm's bits
__device__ __forceinline__ float tg_block_sum(float v, float* sm) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sm[wave] = v;
    __syncthreads();
    return sm[0] + sm[1] + sm[2] + sm[3];
}

// ---------------------------------------------------------------- RMSNorm, forward
// s = fp16(h + add) (h itself without add), y = fp16(s * rsqrt(mean s^2 + eps) * gamma): rmsnorm_kernel's two passes.
__global__ __launch_bounds__(TG_THREADS) void add_rmsnorm_fwd_kernel(const f16* __restrict__ h, const f16* __restrict__ add,
                                                                     const f16* __restrict__ gamma, f16* __restrict__ sum_out,
                                                                     f16* __restrict__ y, TgNorm G, float eps) {
    __shared__ float sm[4];
    const int row = blockIdx.x, nch = tg_norm_chunks(G);
    float ss = 0.f;
    for (int ch = threadIdx.x; ch < nch; ch += TG_THREADS) {
        const long long off = tg_norm_off(G, row, ch);
        h8 v = *(const h8*)(h + off);
        if (add) {
            const h8 w = *(const h8*)(add + off);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (f16)((float)v[j] + (float)w[j]);
            *(h8*)(sum_out + off) = v;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += (float)v[j] * (float)v[j];
    }
    ss = tg_block_sum(ss, sm);
    const float rs = rsqrtf(ss / (float)G.hidden + eps);
    for (int ch = threadIdx.x; ch < nch; ch += TG_THREADS) {
        const long long off = tg_norm_off(G, row, ch);
        h8 v = *(const h8*)(h + off);
        if (add) {
            const h8 w = *(const h8*)(add + off);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (f16)((float)v[j] + (float)w[j]);
        }
        const h8 g = *(const h8*)(gamma + tg_gamma_off(ch));
        h8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = mul_f32_to_f16((float)v[j] * rs, (float)g[j]);
        *(h8*)(y + off) = o;
    }
}

// ---------------------------------------------------------------- RMSNorm, backward
// The sum of 8 values as a tree of depth 3: the backward's two reductions are kept shallow (chunk tree, one add per pass, the
// wave's DPP tree, a tree over the 4 waves) because their depth is what the error bound of the result counts.
__device__ __forceinline__ float tg_tree8(const float (&v)[8]) {
    return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
}

// dsum = fp16(dres + r (gamma dy - s cc)), r = rsqrt(mean s^2 + eps), cc = r^2 / hidden * sum_k gamma_k dy_k s_k
// (= xhat c of the header comment: xhat = s r).  gamma is frozen: no reduction across rows.  Pass 1 forms both sums from one
// read of the row, pass 2 reads it again (from the cache the first pass filled) and stores; dy == NULL: dsum = dres.
__global__ __launch_bounds__(TG_THREADS) void add_rmsnorm_bwd_kernel(const f16* __restrict__ s, const f16* __restrict__ gamma,
                                                                     const f16* __restrict__ dy, const f16* __restrict__ dres,
                                                                     f16* __restrict__ dsum, TgNorm G, float eps) {
    __shared__ float sm[8];
    const int row = blockIdx.x, nch = tg_norm_chunks(G);
    if (!dy) {
        for (int ch = threadIdx.x; ch < nch; ch += TG_THREADS) {
            const long long off = tg_norm_off(G, row, ch);
            *(u32x4*)(dsum + off) = *(const u32x4*)(dres + off);
        }
        return;
    }
    float ss = 0.f, dot = 0.f;
    for (int ch = threadIdx.x; ch < nch; ch += TG_THREADS) {
        const long long off = tg_norm_off(G, row, ch);
        const h8 v = *(const h8*)(s + off), d = *(const h8*)(dy + off), g = *(const h8*)(gamma + tg_gamma_off(ch));
        float sq[8], pr[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float sf = (float)v[j];
            sq[j] = sf * sf;
            pr[j] = ((float)g[j] * (float)d[j]) * sf;
        }
        ss += tg_tree8(sq);
        dot += tg_tree8(pr);
    }
    ss = wave_sum(ss);
    dot = wave_sum(dot);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        sm[wave] = ss;
        sm[4 + wave] = dot;
    }
    __syncthreads();
    ss = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    dot = (sm[4] + sm[5]) + (sm[6] + sm[7]);
    const float r = rsqrtf(ss / (float)G.hidden + eps);
    const float cc = dot * (r * r) * (1.f / (float)G.hidden);
    for (int ch = threadIdx.x; ch < nch; ch += TG_THREADS) {
        const long long off = tg_norm_off(G, row, ch);
        const h8 v = *(const h8*)(s + off), d = *(const h8*)(dy + off), g = *(const h8*)(gamma + tg_gamma_off(ch));
        h8 dr = {0, 0, 0, 0, 0, 0, 0, 0};
        if (dres) dr = *(const h8*)(dres + off);
        h8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (f16)((float)dr[j] + r * ((float)g[j] * (float)d[j] - (float)v[j] * cc));
        *(h8*)(dsum + off) = o;
    }
}

// ---------------------------------------------------------------- SwiGLU
// out = fp16(silu(gate) * up): silu_mul_kernel's arithmetic over rows at their own strides.
__global__ __launch_bounds__(TG_THREADS) void swiglu_fwd_kernel(const f16* __restrict__ gate, const f16* __restrict__ up,
                                                                f16* __restrict__ out, TgSwiglu G) {
    const long long chunk = tg_swiglu_chunk(blockIdx.x, threadIdx.x);
    if (chunk >= tg_swiglu_chunks(G)) return;
    const h8 g = *(const h8*)(gate + tg_swiglu_off(G, chunk, G.gate_stride)), u = *(const h8*)(up + tg_swiglu_off(G, chunk, G.up_stride));
    h8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = mul_f32_to_f16(silu_f32((float)g[j]), (float)u[j]);
    *(h8*)(out + tg_swiglu_off(G, chunk, G.n)) = o;
}

// dup = fp16(dact g sigma), dgate = fp16(dact u sigma (1 + g (1 - sigma))), sigma = 1 / (1 + e^-g).  sigma and 1 - sigma come
// from ONE __expf and ONE hardware reciprocal without a cancellation and without an overflow: z = e^-|g| in (0, 1],
// p = 1 / (1 + z) = sigma(|g|), z p = sigma(-|g|) = 1 - p; the sign of g says which is which.  1.f - sigma would lose all its
// digits from g ~ 17 on, exactly where g (1 - sigma) still matters, and e^-g alone is inf below g ~ -88.
__global__ __launch_bounds__(TG_THREADS) void swiglu_bwd_kernel(const f16* __restrict__ gate, const f16* __restrict__ up,
                                                                const f16* __restrict__ dact, f16* __restrict__ dgate,
                                                                f16* __restrict__ dup, TgSwiglu G) {
    const long long chunk = tg_swiglu_chunk(blockIdx.x, threadIdx.x);
    if (chunk >= tg_swiglu_chunks(G)) return;
    const h8 g8 = *(const h8*)(gate + tg_swiglu_off(G, chunk, G.gate_stride)), u8 = *(const h8*)(up + tg_swiglu_off(G, chunk, G.up_stride));
    const h8 d8 = *(const h8*)(dact + tg_swiglu_off(G, chunk, G.dact_stride));
    h8 og, ou;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float g = (float)g8[j], u = (float)u8[j], d = (float)d8[j];
        const float z = __expf(-fabsf(g));
        const float p = __builtin_amdgcn_rcpf(1.f + z), zp = z * p;
        const float sig = g >= 0.f ? p : zp, oms = g >= 0.f ? zp : p;
        ou[j] = (f16)(d * g * sig);
        og[j] = (f16)((d * u * sig) * (1.f + g * oms));
    }
    *(h8*)(dgate + tg_swiglu_off(G, chunk, G.dgate_stride)) = og;
    *(h8*)(dup + tg_swiglu_off(G, chunk, G.dup_stride)) = ou;
}

// ---------------------------------------------------------------- rotary of q and k
// NeoX pairs (a, b) = (x[i], x[i + 64]) of every head of q and k in one launch: lo = a c - b s, hi = b c + a s; the backward
// is the transpose, the same kernel on the output gradients with the sign of sin flipped (exact: b (-s) = -(b s)).
// The arithmetic is pinned to what the torch expression of finetune._rope and its autograd compute, one rounding per torch op:
// each product rounded to fp32 on its own, their sum rounded to fp32, that converted to fp16.  tg_pin keeps every
// intermediate in a register of its own, so that no product is contracted into an FMA and no sum into v_fma_mixlo_f16
// (mul_f32_to_f16's idiom, qeft_common.h); a head's bits then depend on its 128 values and its position alone.
// One more torch op stands behind the backward: autograd sums the gradients of the two half-slices x[..., :64] and x[..., 64:],
// each padded with +0, in fp16, and (-0) + (+0) = +0 -- the torch route never hands on a gradient of -0.  So the inverse adds
// +0 to its fp16 results (`zero`: +0 in both halves; the forward adds -0, which changes no value), nothing else differs.
__device__ __forceinline__ float tg_pin(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

__device__ __forceinline__ void tg_rope_head(const f16* __restrict__ x, f16* __restrict__ out, long long in_lo, long long in_hi,
                                             long long out_lo, long long out_hi, const float (&c)[8], const float (&s)[8], h2 zero) {
    const h8 a8 = *(const h8*)(x + in_lo), b8 = *(const h8*)(x + in_hi);
    h8 lo, hi;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float a = (float)a8[j], b = (float)b8[j];
        const float ac = tg_pin(a * c[j]), bs = tg_pin(b * s[j]), bc = tg_pin(b * c[j]), as = tg_pin(a * s[j]);
        lo[j] = (f16)tg_pin(ac - bs);
        hi[j] = (f16)tg_pin(bc + as);
    }
    const h8 zero8 = {zero[0], zero[1], zero[0], zero[1], zero[0], zero[1], zero[0], zero[1]};
    *(h8*)(out + out_lo) = lo + zero8;
    *(h8*)(out + out_hi) = hi + zero8;
}

__global__ __launch_bounds__(TG_THREADS) void rope_qk_kernel(const f16* __restrict__ q, const f16* __restrict__ k,
                                                             const float* __restrict__ cos_tab, const float* __restrict__ sin_tab,
                                                             f16* __restrict__ q_out, f16* __restrict__ k_out, TgRope G, int inverse) {
    const int slots = tg_rope_slots(G), lane = tg_rope_lane(threadIdx.x);
    const int row = tg_rope_row(blockIdx.x, threadIdx.x, slots);
    if (row >= G.rows) return;
    float c[8], s[8];
#pragma unroll
    for (int part = 0; part < 2; ++part) {
        const f32x4 cv = *(const f32x4*)(cos_tab + tg_rope_tab_off(G, row, lane, part));
        const f32x4 sv = *(const f32x4*)(sin_tab + tg_rope_tab_off(G, row, lane, part));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c[part * 4 + j] = cv[j];
            s[part * 4 + j] = inverse ? -sv[j] : sv[j];
        }
    }
    uint32_t zbits = inverse ? 0u : 0x80008000u;
    asm volatile("" : "+v"(zbits));                    // opaque: the add below is not an identity the compiler may drop
    const h2 zero = as_h2(zbits);
    const int heads = tg_rope_heads(G);
    for (int head = tg_rope_slot(threadIdx.x, slots); head < heads; head += slots) {
        if (head < G.n_heads)
            tg_rope_head(q, q_out, tg_rope_off(row, head, lane, 0, G.q_stride), tg_rope_off(row, head, lane, 1, G.q_stride),
                         tg_rope_off(row, head, lane, 0, G.n_heads * 128), tg_rope_off(row, head, lane, 1, G.n_heads * 128), c, s, zero);
        else
            tg_rope_head(k, k_out, tg_rope_off(row, head - G.n_heads, lane, 0, G.k_stride),
                         tg_rope_off(row, head - G.n_heads, lane, 1, G.k_stride),
                         tg_rope_off(row, head - G.n_heads, lane, 0, G.n_kv_heads * 128),
                         tg_rope_off(row, head - G.n_heads, lane, 1, G.n_kv_heads * 128), c, s, zero);
    }
}

// ---------------------------------------------------------------- launchers
hipError_t rope_qk_launch(const void* q, const void* k, const void* cos_tab, const void* sin_tab, void* q_out, void* k_out,
                          const TgRope& G, bool inverse, hipStream_t st) {
    hipLaunchKernelGGL(rope_qk_kernel, dim3((unsigned)tg_rope_blocks(G)), dim3(TG_THREADS), 0, st, (const f16*)q, (const f16*)k,
                       (const float*)cos_tab, (const float*)sin_tab, (f16*)q_out, (f16*)k_out, G, inverse ? 1 : 0);
    return hipGetLastError();
}

hipError_t add_rmsnorm_fwd_launch(const void* h, const void* add, const void* gamma, void* sum_out, void* y, const TgNorm& G, float eps,
                                  hipStream_t st) {
    hipLaunchKernelGGL(add_rmsnorm_fwd_kernel, dim3(G.m), dim3(TG_THREADS), 0, st, (const f16*)h, (const f16*)add, (const f16*)gamma,
                       (f16*)sum_out, (f16*)y, G, eps);
    return hipGetLastError();
}

hipError_t add_rmsnorm_bwd_launch(const void* s, const void* gamma, const void* dy, const void* dres, void* dsum, const TgNorm& G,
                                  float eps, hipStream_t st) {
    hipLaunchKernelGGL(add_rmsnorm_bwd_kernel, dim3(G.m), dim3(TG_THREADS), 0, st, (const f16*)s, (const f16*)gamma, (const f16*)dy,
                       (const f16*)dres, (f16*)dsum, G, eps);
    return hipGetLastError();
}

hipError_t swiglu_fwd_launch(const void* gate, const void* up, void* out, const TgSwiglu& G, hipStream_t st) {
    hipLaunchKernelGGL(swiglu_fwd_kernel, dim3((unsigned)tg_swiglu_blocks(G)), dim3(TG_THREADS), 0, st, (const f16*)gate, (const f16*)up,
                       (f16*)out, G);
    return hipGetLastError();
}

hipError_t swiglu_bwd_launch(const void* gate, const void* up, const void* dact, void* dgate, void* dup, const TgSwiglu& G,
                             hipStream_t st) {
    hipLaunchKernelGGL(swiglu_bwd_kernel, dim3((unsigned)tg_swiglu_blocks(G)), dim3(TG_THREADS), 0, st, (const f16*)gate, (const f16*)up,
                       (const f16*)dact, (f16*)dgate, (f16*)dup, G);
    return hipGetLastError();
}

// ---------------------------------------------------------------- address enumeration (host)
namespace {
struct TgWorst {
    long long worst = 0;
    void operator()(long long b, long long bytes, long long operand_bytes) {
        if (b < 0 && -b > worst) worst = -b;
        if (b + bytes - operand_bytes > worst) worst = b + bytes - operand_bytes;
    }
};
inline long long tg_bytes(long long rows, int stride, int width) { return 2 * ((rows - 1) * stride + width); }
}  // namespace

// The largest number of bytes by which an address of a launch passes the end of its operand or runs in front of it, 0 when none
// does.  Every thread of every block is walked through the index functions the kernels use.
long long train_glue_norm_count_out_of_range(const TgNorm& G) {        // forward and backward form the same addresses
    const long long rows_bytes = 2ll * G.m * G.hidden, gamma_bytes = 2ll * G.hidden;
    TgWorst w;
    for (int row = 0; row < G.m; ++row)
        for (int tid = 0; tid < TG_THREADS; ++tid)
            for (int ch = tid; ch < tg_norm_chunks(G); ch += TG_THREADS) {
                w(2 * tg_norm_off(G, row, ch), 16, rows_bytes);
                w(2ll * tg_gamma_off(ch), 16, gamma_bytes);
            }
    return w.worst;
}

long long train_glue_swiglu_count_out_of_range(const TgSwiglu& G, bool backward) {
    TgWorst w;
    for (long long block = 0; block < tg_swiglu_blocks(G); ++block)
        for (int tid = 0; tid < TG_THREADS; ++tid) {
            const long long chunk = tg_swiglu_chunk(block, tid);
            if (chunk >= tg_swiglu_chunks(G)) continue;
            w(2 * tg_swiglu_off(G, chunk, G.gate_stride), 16, tg_bytes(G.m, G.gate_stride, G.n));
            w(2 * tg_swiglu_off(G, chunk, G.up_stride), 16, tg_bytes(G.m, G.up_stride, G.n));
            if (backward) {
                w(2 * tg_swiglu_off(G, chunk, G.dact_stride), 16, tg_bytes(G.m, G.dact_stride, G.n));
                w(2 * tg_swiglu_off(G, chunk, G.dgate_stride), 16, tg_bytes(G.m, G.dgate_stride, G.n));
                w(2 * tg_swiglu_off(G, chunk, G.dup_stride), 16, tg_bytes(G.m, G.dup_stride, G.n));
            } else {
                w(2 * tg_swiglu_off(G, chunk, G.n), 16, tg_bytes(G.m, G.n, G.n));
            }
        }
    return w.worst;
}

long long train_glue_rope_count_out_of_range(const TgRope& G) {        // both directions form the same addresses
    const long long q_bytes = tg_bytes(G.rows, G.q_stride, G.n_heads * 128), k_bytes = tg_bytes(G.rows, G.k_stride, G.n_kv_heads * 128);
    const long long qo_bytes = tg_bytes(G.rows, G.n_heads * 128, G.n_heads * 128), ko_bytes = tg_bytes(G.rows, G.n_kv_heads * 128, G.n_kv_heads * 128);
    const long long tab_bytes = 4ll * G.t_len * 64;
    const int slots = tg_rope_slots(G);
    TgWorst w;
    for (int block = 0; block < tg_rope_blocks(G); ++block)
        for (int tid = 0; tid < TG_THREADS; ++tid) {
            const int row = tg_rope_row(block, tid, slots), lane = tg_rope_lane(tid);
            if (row >= G.rows) continue;
            for (int part = 0; part < 2; ++part) w(4ll * tg_rope_tab_off(G, row, lane, part), 16, tab_bytes);      // cos and sin alike
            for (int head = tg_rope_slot(tid, slots); head < tg_rope_heads(G); head += slots)
                for (int half = 0; half < 2; ++half) {
                    if (head < G.n_heads) {
                        w(2 * tg_rope_off(row, head, lane, half, G.q_stride), 16, q_bytes);
                        w(2 * tg_rope_off(row, head, lane, half, G.n_heads * 128), 16, qo_bytes);
                    } else {
                        w(2 * tg_rope_off(row, head - G.n_heads, lane, half, G.k_stride), 16, k_bytes);
                        w(2 * tg_rope_off(row, head - G.n_heads, lane, half, G.n_kv_heads * 128), 16, ko_bytes);
                    }
                }
        }
    return w.worst;
}

}  // namespace qeft
