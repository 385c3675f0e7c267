// Decode GEMV for the QEFT packed W4 (+ fp16 outlier slice) linear on gfx950, and its 3-bit extension: launch logic.
//
// Replaces gemv_kernel / gemv_kernel_qeft (+ perchannel twins) of
// qeft/kernel/quantization_new/gemv/gemv_cuda{,_qeft}.cu.  Not a translation: the reference tiles for 32-wide warps
// (8 rows x 2048 k per 256-thread block, fp16 accumulation).  Two device implementations live in headers:
//
//  * gemv_w4_mfma.h   the production path (K % 128 == 0, n_out % 128 == 0, group 128 or per-channel, N % 16 == 0): one
//                     wave-wide 16 B/lane load = 16 rows x 128 k = the B operand of v_mfma_f32_16x16x32_f16; x, the
//                     scale shadow and the de-interleaved outlier slab staged in LDS once per long-lived block; fused
//                     gather / RMSNorm / SiLU*up / bias / residual; 1..16 batch rows per weight pass.  With BITS = 3 the same
//                     kernels read the 3-bit EXTENSION layout (BASELINE config 5; the reference has no 3-bit pack or kernel,
//                     QuantLinear asserts bits == 4, qlinear.py:127; the layout is this build's own, oracle/qeft_oracle.py:
//                     pack_w3): one wave-wide 12 B/lane load = 16 rows x 128 k, 24 integer ops per 32 weights instead of
//                     20, 25 % fewer weight bytes.  Also n_out < K there.
//  * gemv_w4_kernel.h the first (VALU, v_dot2c) formulation, kept for everything the MFMA path does not take at 4 bits: other
//                     group sizes, n_out in {32, 64, 96}, ragged N.  Bit-identical fp16 dequantisation to the
//                     reference (one rounded FMA per weight), fp32 accumulation.
//
// gemv_w4_plan picks the kernel, the grid (row sets per block, XCD-contiguous) and the ring depth, slices a batch that
// does not fit the LDS, and lays out the grouped (q|k|v, gate|up) launches; launch_planned is the one launch site.  The lab
// switches QEFT_GEMV_BLOCKS and QEFT_GEMV_DEPTH (gemv_w4_overrides) apply to both bit widths.
#include <cstdlib>
#include <type_traits>

#include "gemv_w4.h"
#include "gemv_w4_mfma.h"

namespace qeft {

namespace {
constexpr int kNW = 8;  // waves per block
constexpr size_t kLdsDefault = 64 * 1024, kLdsMax = 160 * 1024;   // dynamic LDS without / with the opt-in

int ceil_div(int a, int b) { return (a + b - 1) / b; }
size_t mfma_lds(int M, int K, int n_out, int rs = 1) { return gemv_mfma_smem_bytes(kNW, M, K, n_out, rs); }

bool mfma_ok(int bits, int N, int K, int G, int n_out) {
    // no lower bound on N: a row's arithmetic must not depend on how many rows share its launch (row-sharding, §8e)
    return K % 128 == 0 && n_out % 128 == 0 && (G == 128 || G == K) && N % 16 == 0 && (bits == 4 || n_out < K);
}

// Blocks for a layer with `nsets` 16-row sets.  Every block pays ~1 us of start-up plus the x staging before its
// first MFMA (tools/gemv_lab.hip timeline), so wide layers run as 256*k long-lived blocks that each walk ~3 row sets
// with the ring never draining; narrow layers (< 2 sets per CU) keep one block per set.
int mfma_grid(int nsets, const GemvOverrides& ov) {
    if (ov.blocks > 0) return nsets < ov.blocks ? nsets : ov.blocks;
    if (nsets < 512) return nsets;
    const int k = (nsets + 384) / 768;
    return 256 * (k < 1 ? 1 : k);
}

// Ring depth (steps in flight per wave), measured with tools/gemv_lab.hip and bench.py.  VALU: 2 when the wave only has a
// handful of steps (K <= 6144 with 8 waves), 4 for long rows.  MFMA: 4, 6 for K > 6144; deeper is slower -- at 3 bits, where a
// step is 768 bytes per wave instead of 1024, depth 4 / 6 / 8 gave 661 / 643 / 623 tokens/s (bench.py --bits 3): the launch is
// bound by its fixed costs and request latency, not by bytes, so there is no depth-8 instance.
int ring_depth(bool mfma, int K, const GemvOverrides& ov) {
    if (mfma && ov.depth) return ov.depth;
    return (mfma ? 4 : 2) + (K > 6144 ? 2 : 0);
}

// VALU row-groups per wave-load: 4 (16 rows per block) when that still gives >= 1 block per CU and divides every part, fewer
// for small (e.g. row-sharded) layers so they still cover the 256 CUs.
int valu_rgi(int nparts, const int* N) {
    int total = 0, rgi = 4;
    for (int p = 0; p < nparts; ++p) total += N[p] / 4;
    for (; rgi > 1; rgi >>= 1) {
        bool ok = total / rgi >= 256;
        for (int p = 0; p < nparts; ++p) ok = ok && (N[p] / 4) % rgi == 0;
        if (ok) break;
    }
    return rgi;
}

// Blocks per part proportional to its units of `unit` rows (every part gets >= 1 and <= its units): blk_end[] cumulative, the
// most units any block walks returned.  `total` = all units: one block per unit.
int split_blocks(int nparts, const int* N, int unit, int total, int* blk_end) {
    int units = 0, acc = 0, cap = 1;
    for (int p = 0; p < nparts; ++p) units += N[p] / unit;
    if (total <= 0) total = units;
    for (int p = 0; p < 3; ++p) {
        if (p < nparts) {
            const int sp = N[p] / unit;
            int bp = (int)((long long)total * sp / units);
            bp = bp < 1 ? 1 : bp > sp ? sp : bp;
            acc += bp;
            if (ceil_div(sp, bp) > cap) cap = ceil_div(sp, bp);
        }
        blk_end[p] = acc;
    }
    return cap;
}

// the most rows per launch, from `first` down to `floor`, whose LDS fits 160 KB (a batch that does not fit is processed in
// slices: the weights are then streamed once per slice)
template <class Lds>
int fit_rows(int first, int floor, Lds lds) {
    while (first > floor && lds(first) > kLdsMax) --first;
    return first;
}
}  // namespace

GemvOverrides gemv_w4_overrides() {
    static const GemvOverrides once = [] {
        const char* b = getenv("QEFT_GEMV_BLOCKS"), * d = getenv("QEFT_GEMV_DEPTH");
        return GemvOverrides{b ? atoi(b) : 0, d ? (atoi(d) == 6 ? 6 : 4) : 0};
    }();
    return once;
}

GemvPlan gemv_w4_plan(int kind, int bits, int m, int nparts, const int* N, int K, int G, int n_out, bool gather, bool xt_aux,
                      const GemvOverrides& ov) {
    const auto refuse = [](hipError_t e) { GemvPlan r; r.rc = e; return r; };
    const bool fused = kind == kGemvGroup || kind == kGemvSilu, small = kind == kGemvSmallM;   // fused: x transformed while staged, batch 1
    if (fused) m = 1;
    int ntot = 0;
    bool mfma = !(bits == 3 && gather);             // the gather is the caller's at 3 bits
    for (int p = 0; p < nparts; ++p) ntot += N[p], mfma = mfma && N[p] % 16 == 0;
    mfma = mfma && mfma_ok(bits, ntot, K, G, n_out) && !(fused && K > 16384);        // the transforms work on register-held x
    // rows per launch.  4-bit rows: all m in one fixed-M launch if they fit; small-M and 3-bit m >= 2: the run-time-M instance, up to 16
    const bool rt16 = small || (bits == 3 && m != 1);
    const int first = rt16 ? 16 : m;
    int mmax = first;
    if (mfma) {
        mmax = fit_rows(first, small ? 4 : 1, [&](int r) { return mfma_lds(r, K, n_out); });
        // what does not fit (fused: the default 64 KB) leaves the MFMA family -- but 3-bit rows and silu go on and are refused
        // below, launch by launch, at 160 KB
        if (mfma_lds(mmax, K, n_out) > (fused ? kLdsDefault : kLdsMax) && (bits == 4 || kind == kGemvGroup)) mfma = false;
    }
    if (!mfma && (bits == 3 || small)) return refuse(hipErrorNotSupported);           // no VALU fallback
    GemvPlan p;
    p.mfma = mfma, p.bits = bits, p.outl = n_out > 0, p.xg = gather && kind == kGemvRows, p.threads = kNW * 64;
    p.xt = kind == kGemvSilu ? 2 : kind == kGemvGroup && xt_aux ? 1 : 0;
    p.D = rt16 ? 4 : ring_depth(mfma, K, ov);      // (the run-time-M instance exists at depth 4 only, and takes the small-M tail along)
    if (!mfma) {
        p.rgi = valu_rgi(nparts, N);
        if (kind != kGemvGroup && p.outl && p.rgi == 1 && ((N[0] / 4) & 1)) return refuse(hipErrorInvalidValue);  // interleave pairs need N % 8 == 0
        mmax = fit_rows(first, 1, [&](int r) { return gemv_smem_bytes(kNW, p.rgi, r, K, G, n_out); });
        if (gemv_smem_bytes(kNW, p.rgi, mmax, K, G, n_out) > (fused ? kLdsDefault : kLdsMax)) return refuse(hipErrorInvalidValue);
        if (p.xt && K > 4 * 8 * kNW * 64) return refuse(hipErrorInvalidValue);        // transform works on register-held x
    }
    if (m > 0) p.body.count = m / mmax, p.body.rows = mmax, p.tail.count = m % mmax ? 1 : 0, p.tail.rows = m % mmax;
    for (GemvLaunch* l : {&p.body, &p.tail}) {
        if (!l->count) continue;
        l->M = rt16 ? (small && l->rows < 4 ? l->rows : 16) : l->rows < 7 ? l->rows : 7;       // (small-M tail of 1..3 rows: fixed M)
        const int mr = l->M == 16 ? l->rows : l->M;
        if (mfma) {
            // batch 1: long-lived blocks (mfma_grid); if their LDS passes 64 KB, and for more rows, one block per row set
            l->rs_cap = split_blocks(nparts, N, 16, l->M == 1 ? mfma_grid(ntot / 16, ov) : 0, p.blk_end);
            if (mfma_lds(mr, K, n_out, l->rs_cap) > kLdsDefault) l->rs_cap = split_blocks(nparts, N, 16, 0, p.blk_end);
            if (mfma_lds(mr, K, n_out, l->rs_cap) > kLdsMax) return refuse(hipErrorInvalidValue);
            l->lds = (int)mfma_lds(mr, K, n_out, l->rs_cap);
        } else {
            split_blocks(nparts, N, 4 * p.rgi, 0, p.blk_end);
            l->lds = (int)gemv_smem_bytes(kNW, p.rgi, mr, K, G, n_out);
        }
        l->grid = p.blk_end[2];
    }
    static_assert(kGemvValuGroup == kGemvValu + 1 && kGemvValuSilu == kGemvValu + 2 && kGemvMfmaGroup == kGemvMfma + 1 &&
                  kGemvMfmaSilu == kGemvMfma + 2, "family, then + kind");
    p.variant = m < 1 && !small ? kGemvNone
              : bits == 3 ? (kind == kGemvGroup ? kGemvW3Group : kind == kGemvSilu ? kGemvW3Silu : m == 1 ? kGemvW3 : kGemvW3Rows)
              : small ? kGemvMfmaSmallM : (mfma ? kGemvMfma : kGemvValu) + (kind == kGemvGroup ? 1 : kind == kGemvSilu ? 2 : 0);   // (the enum's order)
    return p;
}

// variant -> name, written as the launchers' assignment of g_last_variant: the statement tests/test_variant_census.py reads the names from
static const char* set_last_variant(int v) {
    return g_last_variant =
        v == kGemvValu ? "gemv_valu" : v == kGemvValuGroup ? "gemv_valu_group" : v == kGemvValuSilu ? "gemv_valu_silu" :
        v == kGemvMfma ? "gemv_mfma" : v == kGemvMfmaSmallM ? "gemv_smallm" : v == kGemvMfmaGroup ? "gemv_mfma_group" :
        v == kGemvMfmaSilu ? "gemv_mfma_silu" : v == kGemvW3 ? "gemv_w3" : v == kGemvW3Rows ? "gemv_w3_rows" :
        v == kGemvW3Group ? "gemv_w3_group" : v == kGemvW3Silu ? "gemv_w3_silu" : "";
}
const char* gemv_w4_variant(int v) {      // the same table as a query: the calling thread's last variant stays what it was
    const char* const last = g_last_variant, * const name = set_last_variant(v);
    g_last_variant = last;
    return name;
}

// f(std::integral_constant<int, V>) for the V among Vs that v equals: a run-time selector becomes a template argument over
// exactly the listed values, so the launch site below instantiates the kernels the plans can name and no others
template <int... Vs, class F>
static hipError_t pick(int v, F f) {
    hipError_t e = hipErrorInvalidValue;
    (void)((v == Vs ? (e = f(std::integral_constant<int, Vs>{}), true) : false) || ...);
    return e;
}

// The launch site: one planned launch on its arguments (GemvArgs, or GemvGroupArgs for a group plan).
template <class Args>
static hipError_t launch_planned(const GemvPlan& p, const GemvLaunch& l, const Args& a, hipStream_t st) {
    const auto go = [&](auto kern, auto... tail) -> hipError_t {
        if (l.lds > (int)kLdsDefault)
            if (hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, l.lds)) return e;
        hipLaunchKernelGGL(kern, dim3(l.grid), dim3(p.threads), l.lds, st, a, tail...);
        return hipGetLastError();
    };
    const auto outl = [&](auto f) { return pick<0, 1>(p.outl, f); };
    const auto rgi_d = [&](auto f) { return pick<1, 2, 4>(p.rgi, [&](auto R) { return pick<2, 4>(p.D, [&](auto D) { return f(R, D); }); }); };
    const auto bits_d = [&](auto f) { return pick<3, 4>(p.bits, [&](auto B) { return pick<4, 6>(p.D, [&](auto D) { return f(B, D); }); }); };
    if constexpr (std::is_same<Args, GemvGroupArgs>::value) {
        if (p.mfma) return bits_d([&](auto B, auto D) { return outl([&](auto O) { return pick<0, 1>(p.xt, [&](auto T) {
            return go(gemv_w4_mfma_group_kernel<kNW, D, O != 0, T, B>, l.rs_cap); }); }); });
        return rgi_d([&](auto R, auto D) { return outl([&](auto O) { return pick<0, 1>(p.xt, [&](auto T) {
            return go(gemv_w4_group_kernel<kNW, R, 1, D, O != 0, T>); }); }); });
    } else if (!p.mfma) {
        if (p.xt) return rgi_d([&](auto R, auto D) { return outl([&](auto O) { return go(gemv_w4_kernel<kNW, R, 1, D, O != 0, false, 0, 2>); }); });
        return rgi_d([&](auto R, auto D) { return pick<1, 2, 3, 4, 5, 6, 7>(l.M, [&](auto M) { return outl([&](auto O) {
            return pick<0, 1>(p.xg, [&](auto X) { return go(gemv_w4_kernel<kNW, R, M, D, O != 0, X != 0, 0, 0>); }); }); }); });
    } else if (l.M == 16) {       // the run-time-M instance
        return pick<3, 4>(p.bits, [&](auto B) { return outl([&](auto O) { return go(gemv_w4_mfma_kernel<kNW, 16, 4, O != 0, false, 0, 0, B>, l.rs_cap); }); });
    } else if (p.bits == 4 && p.xt == 0) {      // 1..7 fixed rows, optional gather
        return pick<4, 6>(p.D, [&](auto D) { return pick<1, 2, 3, 4, 5, 6, 7>(l.M, [&](auto M) { return outl([&](auto O) {
            return pick<0, 1>(p.xg, [&](auto X) { return go(gemv_w4_mfma_kernel<kNW, M, D, O != 0, X != 0, 0, 0, 4>, l.rs_cap); }); }); }); });
    } else {                      // batch 1, no gather: the SiLU staging, 3 bits
        return bits_d([&](auto B, auto D) { return outl([&](auto O) { return pick<0, 2>(p.xt, [&](auto T) {
            return go(gemv_w4_mfma_kernel<kNW, 1, D, O != 0, false, T, 0, B>, l.rs_cap); }); }); });
    }
}

hipError_t gemv_w4_launch(int kind, int bits, const GemvArgs& a0, int m, hipStream_t st) {
    const GemvPlan p = gemv_w4_plan(kind, bits, m, 1, &a0.N, a0.K, a0.G, a0.n_out, a0.ids != nullptr, false, gemv_w4_overrides());
    if (p.rc != hipSuccess) return p.rc;
    if (p.variant) set_last_variant(p.variant);
    int m0 = 0;
    for (const GemvLaunch* l : {&p.body, &p.tail})
        for (int i = 0; i < l->count; ++i, m0 += l->rows) {
            GemvArgs a = a0;
            a.x = a0.x + (size_t)m0 * a0.K;
            a.y = a0.y + (size_t)m0 * a0.N;
            if (a0.residual) a.residual = a0.residual + (size_t)m0 * a0.N;
            if (l->M == 16) a.m_rt = l->rows;
            if (hipError_t e = launch_planned(p, *l, a, st)) return e;
        }
    return hipSuccess;
}

hipError_t gemv_w4_group_launch(int bits, GemvGroupArgs g, int nparts, hipStream_t st) {
    const GemvPlan p = gemv_w4_plan(kGemvGroup, bits, 1, nparts, g.N, g.K, g.G, g.n_out, false, g.xt_aux != nullptr, gemv_w4_overrides());
    if (p.rc != hipSuccess) return p.rc;
    set_last_variant(p.variant);
    for (int i = 0; i < 3; ++i) g.blk_end[i] = p.blk_end[i];
    return launch_planned(p, p.body, g, st);
}

// 3-bit stream -> 4-bit checkpoint layout (qlinear.py:81-121 nibble order; the fp16 columns get dead zero nibbles): what the GEMM
// forward, dX and the dense dequant run on where they have no 3-bit tile of their own -- a scratch buffer, 3/8 byte read and 1/2
// byte written per weight, a few us per layer.  One thread per (row, 32-k chunk): 12 bytes in, 16 bytes out.
__global__ __launch_bounds__(256) void expand_w3_kernel(const uint32_t* __restrict__ q3, uint8_t* __restrict__ q4, int N,
                                                        int K, int n_out) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int chunks = K / 32;
    if (idx >= (size_t)N * chunks) return;
    const int n = (int)(idx / chunks), c = (int)(idx % chunks);
    const int k0 = c * 32, kq = K - n_out, nfull = kq / 128;
    u32x4 out = {0u, 0u, 0u, 0u};
    if (k0 < kq) {
        const int step = k0 / 128, lane = ((k0 >> 5) & 3) * 16 + (n & 15);
        const uint32_t* w = q3 + (((size_t)(n >> 4) * nfull + step) * 64 + lane) * 3;
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
        uint32_t ext[16];   // pair e: low half = value of k = 2e, high half = value of k = 2e + 1
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint32_t v = i == 0 ? w0 : i == 1 ? w1 : w2;
#pragma unroll
            for (int t = 0; t < 5; ++t) ext[5 * i + t] = (v >> (3 * t)) & 0x00070007u;
        }
        ext[15] = ((w0 >> 15) & 0x00010001u) | ((w1 >> 14) & 0x00020002u) | ((w2 >> 13) & 0x00040004u);
        // 4-bit word wd holds pairs e = 4 j + wd (j = 0..3) at bits 4 j (low half) and 16 + 4 j (high half)
#pragma unroll
        for (int wd = 0; wd < 4; ++wd)
#pragma unroll
            for (int j = 0; j < 4; ++j) out[wd] |= ext[4 * j + wd] << (4 * j);
    }
    uint8_t* dst = q4 + (size_t)(n >> 2) * K * 2 + (size_t)(k0 >> 6) * 128 + (n & 3) * 32 + ((k0 >> 5) & 1) * 16;
    *(u32x4*)dst = out;
}

hipError_t expand_w3_launch(const void* q3, void* q4, int N, int K, int n_out, hipStream_t st) {
    if (!mfma_ok(3, N, K, 128, n_out)) return hipErrorNotSupported;
    const size_t total = (size_t)N * (K / 32);
    hipLaunchKernelGGL(expand_w3_kernel, dim3((int)((total + 255) / 256)), dim3(256), 0, st, (const uint32_t*)q3,
                       (uint8_t*)q4, N, K, n_out);
    return hipGetLastError();
}

}  // namespace qeft
