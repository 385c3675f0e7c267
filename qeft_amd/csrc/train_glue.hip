// The glue of a training step between the linears, attention and the head: RMSNorm with the residual
// add in front of it and SiLU(gate) * up -- forwards over a [B T] batch of rows and a backward for each.
// finetune.causal_lm_loss(glue="fused") runs them through qeft_amd/glue.py; decode_aux.hip keeps the inference forms.
//
// All of them are memory-bound row kernels: 16-byte loads and stores, fp32 math, every output rounded to fp16 exactly once, no
// atomics, no workspace, nothing saved between forward and backward beyond the operands themselves.  A row's results depend on
// that row's operands alone, bit for bit: a norm row is one block with a fixed reduction order, a SwiGLU chunk is one lane's
// work.  The forwards reproduce the arithmetic of qeft_rmsnorm and qeft_silu_mul (decode_aux.hip) operation for operation, so
// their bits are those kernels' bits.
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

// ---------------------------------------------------------------- launchers
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

}  // namespace qeft
