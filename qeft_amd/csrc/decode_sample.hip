// Sampled token end of the decode engine (qeft_amd/sampling.py): temperature, top-k and top-p over one fp16
// logits row per block, and a draw from a counter-based RNG, so that the whole step stays on the device inside captured graphs.
//   sample             row r of `logits` with parameter record r, drawn at positions[r] -> tokens[r]      (m rows, any m >= 1)
//   token_end_sample   token_end's contract (tok, *pos += 1) with a draw at *pos + 1                       (one row)
//   token_end_sample_b token_end_b's contract (slot table, out / counter tickets, stops) with params[slot]  (m <= 8 rows)
//   verify_sample      verify_greedy's contract with row i of ONE sequence drawn at *pos + i + 1            (m <= 8 rows)
// Parameter record (int32 [8]): temperature (fp32 bits), top_k, top_p (fp32 bits), seed lo, seed hi, 3 reserved.
//
// Method, per row (one block of 1024 threads): every fp16 logit maps to an order-preserving 16-bit key (NaN -> 0, never kept;
// -0 -> +0).  The k-th largest key and the top-p threshold key come from two-level radix selects (256 bins on the high byte,
// then 256 on the low byte inside the chosen bin) over LDS histograms: counts for top-k, fixed-point weights round(w * 2^40)
// summed in u64 for top-p.  Integer sums do not depend on the order of the adds, so the kept set, its mass and the inverse-CDF
// search are exact and the token is a function of (row, record, position) alone.  Rows up to 32768 entries keep their keys in
// registers across the passes; longer rows are re-read from global memory (L2-resident after the first pass).
#include "qeft_common.h"
#include "host_launch.h"

namespace qeft {

typedef unsigned long long u64;

namespace {

constexpr int kThreads = 1024;
constexpr int kChunk = kThreads * 8;        // row entries per chunk (8 consecutive entries per thread)
constexpr int kRegChunks = 4;               // rows up to 4 chunks (32768 entries) keep their keys in registers
constexpr u64 kOne = 1ull << 40;            // fixed-point weight of the row's maximum
constexpr uint32_t kKeyNegInf = 0x03ffu;    // key of -inf: a row whose largest key is this has no value above -inf

// Random123 Philox4x32-10: x0, the first output word, of counter (p, 0, 0, 0) under key (k0, k1)
__device__ __forceinline__ uint32_t philox_x0(uint32_t p, uint32_t k0, uint32_t k1) {
    uint32_t c0 = p, c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// order-preserving key of an fp16 bit pattern: NaN -> 0 (below every value), -0 -> the key of +0
__device__ __forceinline__ uint32_t key_of(uint32_t b) {
    if ((b & 0x7fffu) > 0x7c00u) return 0;
    if (b == 0x8000u) b = 0;
    return b & 0x8000u ? (~b & 0xffffu) : (b | 0x8000u);
}

__device__ __forceinline__ float value_of(uint32_t key) {
    const uint32_t b = key & 0x8000u ? (key & 0x7fffu) : (~key & 0xffffu);
    return (float)__builtin_bit_cast(f16, (unsigned short)b);
}

struct Filter {
    uint32_t kmax;      // largest key of the row
    float lmax, T;
};

// round(w * 2^40) of a key, w = exp((l - max) / T) in fp32; the row's maximum weighs exactly 1, NaN nothing
__device__ __forceinline__ u64 weight_of(uint32_t key, const Filter& f) {
    if (key == 0) return 0;
    if (key == f.kmax) return kOne;
    const float w = expf((value_of(key) - f.lmax) / f.T);
    return w == w ? (u64)rintf(w * 0x1p40f) : 0;
}

// the 8 keys of chunk c of this thread (entries c * kChunk + 8 t + j; entries past the row -> 0)
__device__ __forceinline__ void load_keys(const f16* __restrict__ lg, int vocab, int c, uint32_t (&k)[8]) {
    const int i = c * kChunk + threadIdx.x * 8;
    if ((vocab & 7) == 0 && i + 8 <= vocab) {
        const u32x4 v = *(const u32x4*)(lg + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            k[2 * j] = key_of(v[j] & 0xffffu);
            k[2 * j + 1] = key_of(v[j] >> 16);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) k[j] = i + j < vocab ? key_of(__builtin_bit_cast(unsigned short, lg[i + j])) : 0;
    }
}

// The keys of one row: held in registers (REG) or re-read per pass.  each(f) calls f(c, keys[8]) for every chunk in order.
template <bool REG>
struct Row {
    const f16* lg;
    int vocab, nchunk;
    uint32_t kr[REG ? kRegChunks : 1][8];

    __device__ __forceinline__ void init(const f16* l, int v) {
        lg = l;
        vocab = v;
        nchunk = (v + kChunk - 1) / kChunk;
        if constexpr (REG) {
#pragma unroll
            for (int c = 0; c < kRegChunks; ++c) {
                if (c < nchunk) {
                    load_keys(lg, vocab, c, kr[c]);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) kr[c][j] = 0;
                }
            }
        }
    }
    template <class F>
    __device__ __forceinline__ void each(F&& f) {
        if constexpr (REG) {
#pragma unroll
            for (int c = 0; c < kRegChunks; ++c)
                if (c < nchunk) f(c, kr[c]);
        } else {
            for (int c = 0; c < nchunk; ++c) {
                uint32_t k[8];
                load_keys(lg, vocab, c, k);
                f(c, k);
            }
        }
    }
};

struct Smem {
    uint32_t cnt[256];
    u64 wt[256];
    u64 part[16];        // per-wave values of block reductions / scans
    u64 res[4];          // broadcast slots
};

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 x = __shfl_xor(v, o);
        v = x > v ? x : v;
    }
    return v;
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sum over the block of one u64 per thread (fixed order: waves, then wave totals 0..15); every thread gets it
__device__ __forceinline__ u64 block_sum_u64(Smem& sm, u64 v) {
    v = wave_sum_u64(v);
    if ((threadIdx.x & 63) == 0) sm.part[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 s = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) s += sm.part[w];
    __syncthreads();
    return s;
}

__device__ __forceinline__ void clear_hist(Smem& sm) {
    if (threadIdx.x < 256) {
        sm.cnt[threadIdx.x] = 0;
        sm.wt[threadIdx.x] = 0;
    }
    __syncthreads();
}

// Wave 0 walks the 256 bins from the top.  Lane l owns bins 4l .. 4l + 3; above(b) = base + the sum of v over the bins > b.
//   by count (mass == false, v = cnt): the bin with above(b) < target <= above(b) + cnt[b]
//   by mass  (mass == true,  v = wt):  the LOWEST bin with cnt[b] > 0 and above(b) < thr
// res[0] = the bin (256: none), res[1] = above(bin).  The caller synchronises before and after.
__device__ __forceinline__ void select_bin(Smem& sm, bool mass, u64 base, u64 target, double thr) {
    if (threadIdx.x >= 64) return;
    const int l = threadIdx.x;
    u64 v[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = mass ? sm.wt[4 * l + j] : (u64)sm.cnt[4 * l + j];
        s += v[j];
    }
    u64 incl = s;            // sum over lanes >= l
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 y = __shfl_down(incl, d);
        if (l + d < 64) incl += y;
    }
    u64 above = base + incl - s;
    int found = 256;
    u64 fa = 0;
#pragma unroll
    for (int j = 3; j >= 0; --j) {
        const int b = 4 * l + j;
        const bool hit = mass ? (sm.cnt[b] > 0 && (double)above < thr) : (above < target && target <= above + v[j]);
        if (hit) {
            found = b;
            fa = above;
        }
        above += v[j];
    }
    int best = found;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
    if (best < 256 && found == best) {
        sm.res[0] = (u64)best;
        sm.res[1] = fa;
    } else if (best == 256 && l == 0) {
        sm.res[0] = 256;
        sm.res[1] = 0;
    }
}

// The token of one row; every thread of the block calls it and gets the result.  x0: the row's Philox word.
template <bool REG>
__device__ __forceinline__ int sample_row(Smem& sm, const f16* __restrict__ lg, int vocab, const int* __restrict__ rec, uint32_t x0) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    Row<REG> row;
    row.init(lg, vocab);

    // ---- pass 1: the largest key and the lowest index holding it (token_end's argmax), as one u64 maximum
    u64 best = 0;
    row.each([&](int c, const uint32_t(&k)[8]) __attribute__((always_inline)) {
        const uint32_t i0 = (uint32_t)(c * kChunk + t * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const u64 v = ((u64)k[j] << 32) | (0xffffffffu - (i0 + j));
            best = v > best ? v : best;
        }
    });
    best = wave_max_u64(best);
    if (lane == 0) sm.part[wave] = best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 16; ++w) best = sm.part[w] > best ? sm.part[w] : best;
    __syncthreads();
    const uint32_t kmax = (uint32_t)(best >> 32);
    const int greedy_tok = kmax > kKeyNegInf ? (int)(0xffffffffu - (uint32_t)best) : 0;   // no value above -inf: 0, as token_end
    const float T = __builtin_bit_cast(float, rec[0]);
    if (!(T > 0.f) || kmax == 0) return greedy_tok;        // T == 0: greedy; a row of NaN: token_end's 0
    const int top_k = rec[1];
    const float top_p = __builtin_bit_cast(float, rec[2]);
    const Filter f{kmax, value_of(kmax), T};

    // ---- top-k: the k-th largest key (two levels of count histograms); every key >= tau survives
    uint32_t tau = 1;
    if (top_k > 0 && top_k < vocab) {
        clear_hist(sm);
        row.each([&](int, const uint32_t(&k)[8]) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (k[j]) atomicAdd(&sm.cnt[k[j] >> 8], 1u);
        });
        __syncthreads();
        select_bin(sm, false, 0, (u64)top_k, 0.0);
        __syncthreads();
        const uint32_t hb = (uint32_t)sm.res[0];
        const u64 above = sm.res[1];
        __syncthreads();
        if (hb < 256) {                  // (none: fewer than k values, every one survives)
            clear_hist(sm);
            row.each([&](int, const uint32_t(&k)[8]) __attribute__((always_inline)) {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (k[j] && (k[j] >> 8) == hb) atomicAdd(&sm.cnt[k[j] & 255], 1u);
            });
            __syncthreads();
            select_bin(sm, false, above, (u64)top_k, 0.0);
            __syncthreads();
            tau = (hb << 8) | (uint32_t)sm.res[0];
            __syncthreads();
        }
    }

    // ---- the survivors' mass Z (binned by high byte for top-p); top-p: the lowest key v with W(> v) < p Z (two levels of bins)
    const bool use_p = top_p < 1.f;
    clear_hist(sm);
    u64 zt = 0;
    row.each([&](int, const uint32_t(&k)[8]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (k[j] >= tau) {
                const u64 w = weight_of(k[j], f);
                zt += w;
                if (use_p) {
                    atomicAdd(&sm.cnt[k[j] >> 8], 1u);
                    if (w) atomicAdd(&sm.wt[k[j] >> 8], w);
                }
            }
    });
    const u64 Z = block_sum_u64(sm, zt);                   // (its barriers also complete the histogram)
    u64 zkept = Z;
    if (use_p) {
        const double thr = (double)top_p * (double)Z;
        select_bin(sm, true, 0, 0, thr);
        __syncthreads();
        const uint32_t hb = (uint32_t)sm.res[0];
        const u64 above = sm.res[1];
        __syncthreads();
        if (hb < 256) {
            clear_hist(sm);
            row.each([&](int, const uint32_t(&k)[8]) __attribute__((always_inline)) {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (k[j] >= tau && (k[j] >> 8) == hb) {
                        const u64 w = weight_of(k[j], f);
                        atomicAdd(&sm.cnt[k[j] & 255], 1u);
                        if (w) atomicAdd(&sm.wt[k[j] & 255], w);
                    }
            });
            __syncthreads();
            select_bin(sm, true, above, 0, thr);
            __syncthreads();
            const uint32_t lb = (uint32_t)sm.res[0];
            tau = (hb << 8) | lb;
            // kept mass: the bins above hb plus this bin's low bytes >= lb
            zkept = above + block_sum_u64(sm, t < 256 && (uint32_t)t >= lb ? sm.wt[t] : 0);
        } else {                         // (top_p <= 0: the maximum alone)
            tau = kmax;
            u64 n = 0;
            row.each([&](int, const uint32_t(&k)[8]) __attribute__((always_inline)) {
#pragma unroll
                for (int j = 0; j < 8; ++j) n += k[j] == kmax ? kOne : 0;
            });
            zkept = block_sum_u64(sm, n);
        }
    }

    // ---- draw: the first kept entry (index order) whose inclusive cumulative weight exceeds floor(x0 * Z_kept / 2^32)
    const u64 target = (u64)x0 * (zkept >> 32) + (((u64)x0 * (zkept & 0xffffffffull)) >> 32);
    if (t == 0) sm.res[2] = (u64)(unsigned)greedy_tok;
    u64 base = 0;
    bool found = false;
    row.each([&](int c, const uint32_t(&k)[8]) __attribute__((always_inline)) {
        if (found) return;                              // (uniform: base is the same in every thread)
        u64 w8[8], s = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            w8[j] = k[j] >= tau ? weight_of(k[j], f) : 0;
            s += w8[j];
        }
        u64 incl = s;                                   // inclusive scan over the wave's lanes
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u64 y = __shfl_up(incl, d);
            if (lane >= d) incl += y;
        }
        if (lane == 63) sm.part[wave] = incl;
        __syncthreads();
        u64 before = base, total = base;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const u64 p = sm.part[w];
            if (w < wave) before += p;
            total += p;
        }
        before += incl - s;
        if (before <= target && target < before + s) {   // this thread holds the crossing entry (its weight is > 0)
            u64 cum = before;
            int hit = -1;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                cum += w8[j];
                if (hit < 0 && cum > target) hit = j;
            }
            sm.res[2] = (u64)(c * kChunk + t * 8 + hit);
        }
        __syncthreads();
        base = total;
        found = total > target;
    });
    const int a = (int)sm.res[2];
    __syncthreads();
    return a;
}

__device__ __forceinline__ uint32_t row_x0(const int* rec, int p) {
    return philox_x0((uint32_t)p, (uint32_t)rec[3], (uint32_t)rec[4]);
}

template <bool REG>
__global__ __launch_bounds__(1024) void sample_kernel(const f16* __restrict__ logits, int vocab, const int* __restrict__ params,
                                                      const int* __restrict__ positions, long long* __restrict__ tokens) {
    __shared__ Smem sm;
    const int row = blockIdx.x;
    const int* rec = params + (size_t)row * 8;
    const int a = sample_row<REG>(sm, logits + (size_t)row * vocab, vocab, rec, row_x0(rec, positions[row]));
    if (threadIdx.x == 0) tokens[row] = a;
}

template <bool REG>
__global__ __launch_bounds__(1024) void token_end_sample_kernel(const f16* __restrict__ logits, long long* __restrict__ tok,
                                                                int* __restrict__ pos, const int* __restrict__ params, int vocab) {
    __shared__ Smem sm;
    const int p = *pos;
    const int a = sample_row<REG>(sm, logits, vocab, params, row_x0(params, p + 1));   // (every thread has read *pos by now)
    if (threadIdx.x == 0) {
        *tok = a;
        *pos = p + 1;
    }
}

// token_end_b_kernel (decode_batch.hip) with the row's token drawn with params[slot] at pos[slot] + 1
template <bool REG>
__global__ __launch_bounds__(1024) void token_end_sample_b_kernel(const f16* __restrict__ logits, const int* __restrict__ slot_tab,
                                                                  long long* __restrict__ tok, int* __restrict__ pos_tab,
                                                                  const int* __restrict__ limit, const int* __restrict__ eos,
                                                                  int* __restrict__ done, long long* __restrict__ out,
                                                                  int* __restrict__ ctr, const int* __restrict__ params, int vocab,
                                                                  int out_cap, int n_slots) {
    __shared__ Smem sm;
    const int t = threadIdx.x, row = blockIdx.x;
    const int s0 = slot_tab[row];
    const int s = s0 >= 0 && s0 < n_slots ? s0 : -1;
    const bool active = s >= 0 && done[s] == 0;       // uniform over the block
    int a = 0;
    if (active) {
        const int* rec = params + (size_t)s * 8;
        a = sample_row<REG>(sm, logits + (size_t)row * vocab, vocab, rec, row_x0(rec, pos_tab[s] + 1));
    }
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

// verify_greedy_kernel's contract (decode_verify.hip) with the argmax of row i replaced by the draw at *pos + i + 1 with the
// sequence's record: what token_end_sample would draw there.  One block per row, so the m rows run side by side.  Block i leaves
// a[i] in work[i] and takes a ticket in work[kVerifyTicket]; the last arriver forms the accepted prefix and re-arms the ticket.
// Every thread has read *pos before its block arrives (sample_row synchronises), so the last arriver's store races with nothing.
constexpr int kVerifyTicket = 8;

template <bool REG>
__global__ __launch_bounds__(1024) void verify_sample_kernel(const f16* __restrict__ logits, const long long* __restrict__ tokens,
                                                             int vocab, const int* __restrict__ params, int* __restrict__ work,
                                                             long long* __restrict__ out_tokens, int* __restrict__ n_acc,
                                                             long long* __restrict__ tok, int* __restrict__ pos) {
    __shared__ Smem sm;
    const int row = blockIdx.x, m = gridDim.x;
    const int p0 = *pos;
    const int a = sample_row<REG>(sm, logits + (size_t)row * vocab, vocab, params, row_x0(params, p0 + row + 1));
    if (threadIdx.x != 0) return;
    __hip_atomic_store(work + row, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int ticket = __hip_atomic_fetch_add(work + kVerifyTicket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket != m - 1) return;
    __hip_atomic_store(work + kVerifyTicket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int n = 0;
    int an = __hip_atomic_load(work, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (n < m - 1 && (long long)an == tokens[n + 1]) {
        out_tokens[n] = tokens[n + 1];
        ++n;
        an = __hip_atomic_load(work + n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    out_tokens[n] = an;
    *n_acc = n;
    *tok = an;
    *pos = p0 + n + 1;
}

}  // namespace

hipError_t sample_launch(const void* logits, int vocab, int m, const int* params, const int* positions, void* tokens, hipStream_t st) {
    auto kern = vocab <= kRegChunks * kChunk ? sample_kernel<true> : sample_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(m), dim3(kThreads), 0, st, (const f16*)logits, vocab, params, positions, (long long*)tokens);
    return hipGetLastError();
}

hipError_t token_end_sample_launch(const void* logits, void* tok, int* pos, const int* params, int vocab, hipStream_t st) {
    auto kern = vocab <= kRegChunks * kChunk ? token_end_sample_kernel<true> : token_end_sample_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(1), dim3(kThreads), 0, st, (const f16*)logits, (long long*)tok, pos, params, vocab);
    return hipGetLastError();
}

hipError_t token_end_sample_b_launch(const void* logits, const int* slot_tab, void* tok, int* pos_tab, const int* limit, const int* eos,
                                     int* done, void* out, int* ctr, const int* params, int vocab, int out_cap, int n_slots, int m,
                                     hipStream_t st) {
    auto kern = vocab <= kRegChunks * kChunk ? token_end_sample_b_kernel<true> : token_end_sample_b_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(m), dim3(kThreads), 0, st, (const f16*)logits, slot_tab, (long long*)tok, pos_tab, limit, eos, done,
                       (long long*)out, ctr, params, vocab, out_cap, n_slots);
    return hipGetLastError();
}

hipError_t verify_sample_launch(const void* logits, const void* tokens, int m, int vocab, const int* params, int* work, void* out_tokens,
                                int* n_acc, void* tok, int* pos, hipStream_t st) {
    auto kern = vocab <= kRegChunks * kChunk ? verify_sample_kernel<true> : verify_sample_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(m), dim3(kThreads), 0, st, (const f16*)logits, (const long long*)tokens, vocab, params, work,
                       (long long*)out_tokens, n_acc, (long long*)tok, pos);
    return hipGetLastError();
}

}  // namespace qeft
