// The device quantise-and-pack kernel (qeft_cuda.quant_pack, QuantLinear.pack_device,
// calibrate.rtn_linear).  The contract, the pinned arithmetic, the split of the work and the bounds: quant_pack.h.  Nothing below
// may be contracted into an FMA, hence the pragma over the whole file; the divisions are IEEE (the compiler's default for fp32).
#include <math.h>

#include "qeft_common.h"
#include "quant_pack.h"

#pragma clang fp contract(off)

namespace qeft {

union QpLoad {                                          // one 16-byte load = 8 fp16 columns
    uint4 v;
    _Float16 h[8];
};

template <int BITS>
__device__ __forceinline__ float qp_clamp(float v) {
    return fminf(fmaxf(v, 0.f), (float)((1 << BITS) - 1));          // NaN -> 0
}

// A lane's 32 columns col0 .. col0 + 31 of the operand as fp32, the first n_read of them (1 .. 32; the others stay 0 on the
// gather route and are read but unused on the 16-byte route: col0 + 32 <= k).
template <bool GATHER>
__device__ __forceinline__ void qp_read32(const _Float16* __restrict__ wrow, const int* __restrict__ col_ids, int col0, int n_read,
                                          int k, float (&x)[32]) {
    if (GATHER) {
#pragma unroll
        for (int j = 0; j < 32; ++j)
            if (j < n_read) x[j] = (float)wrow[min(max(col_ids[col0 + j], 0), k - 1)];
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            QpLoad l;
            l.v = *reinterpret_cast<const uint4*>(wrow + col0 + 8 * i);
#pragma unroll
            for (int j = 0; j < 8; ++j) x[8 * i + j] = (float)l.h[j];
        }
    }
}

// The lane's 32 codes into qweight: 16 bytes of the 4-bit layout, or (group < live / 128) 3 words of the 3-bit stream.
template <int BITS>
__device__ __forceinline__ void qp_emit(const unsigned (&c)[32], void* __restrict__ qweight, const QpGeom& G, int row, int group,
                                        int chunk, int lane) {
    if (BITS == 4) {
        uint4 o;
        unsigned* ow = reinterpret_cast<unsigned*>(&o);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {                            // int16 j holds columns j, 8 + j, 16 + j, 24 + j of the chunk
            const unsigned a = c[2 * jj] | (c[8 + 2 * jj] << 4) | (c[16 + 2 * jj] << 8) | (c[24 + 2 * jj] << 12);
            const unsigned b = c[2 * jj + 1] | (c[9 + 2 * jj] << 4) | (c[17 + 2 * jj] << 8) | (c[25 + 2 * jj] << 12);
            ow[jj] = a | (b << 16);
        }
        *reinterpret_cast<uint4*>(reinterpret_cast<short*>(qweight) + qp_q4_off(G, row, group, chunk)) = o;
    } else if (group < qp_live(G) / QP_GROUP) {                     // the 3-bit stream ends with the live columns
        unsigned o[3] = {0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 15; ++e)
#pragma unroll
            for (int h = 0; h < 2; ++h) o[e / 5] |= c[2 * e + h] << (16 * h + 3 * (e % 5));
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int b = 0; b < 3; ++b) o[b] |= ((c[30 + h] >> b) & 1u) << (15 + 16 * h);
        unsigned* dst = reinterpret_cast<unsigned*>(qweight) + qp_q3_off(G, row, group, lane);
        dst[0] = o[0];
        dst[1] = o[1];
        dst[2] = o[2];
    }
}

template <int BITS, bool FIND, bool GATHER>
__global__ __launch_bounds__(QP_THREADS) void quant_pack_kernel(const _Float16* __restrict__ w, const int* __restrict__ col_ids,
                                                                const float* __restrict__ scale_in, const float* __restrict__ zero_in,
                                                                void* __restrict__ qweight, _Float16* __restrict__ scales,
                                                                _Float16* __restrict__ scaled_zeros, float* __restrict__ scale_out,
                                                                float* __restrict__ zero_out, QpGeom G) {
    constexpr float MAXQ = (float)((1 << BITS) - 1);
    const int lane = threadIdx.x & 63;
    const int group = blockIdx.y * QP_WAVES + (threadIdx.x >> 6);
    const int ng = qp_groups(G);
    if (group >= ng) return;                                        // no barrier below: a wave may leave alone
    const int chunk = lane >> 4;
    const int row = blockIdx.x * QP_ROWS + (lane & 15);             // < n: n % 16 == 0
    const int live = qp_live(G);
    // the group whose columns are read: the wave's own, or (find mode, no live column of its own) the last that has one
    const int rgroup = FIND ? min(group, qp_last_live_group(G)) : group;
    const int col0 = rgroup * QP_GROUP + chunk * 32;                // col0 + 32 <= k
    const int n_read = min(max(live - col0, 0), 32);                // live columns among the lane's 32 of the group read
    const int n_code = min(max(live - (group * QP_GROUP + chunk * 32), 0), 32);      // ... of the wave's own group

    float x[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) x[j] = 0.f;
    const _Float16* wrow = w + (size_t)row * G.ld_w;
    if (n_read > 0) qp_read32<GATHER>(wrow, col_ids, col0, n_read, G.k, x);

    float s, z;
    if (FIND) {
        float lo = 0.f, hi = 0.f;                                   // min and max do not round: any order gives the row's
#pragma unroll
        for (int j = 0; j < 32; ++j)
            if (j < n_read) {
                lo = fminf(lo, x[j]);
                hi = fmaxf(hi, x[j]);
            }
#pragma unroll
        for (int off = 16; off < 64; off <<= 1) {                   // the row's 4 lanes: lane ^ 16, lane ^ 32
            lo = fminf(lo, __shfl_xor(lo, off));
            hi = fmaxf(hi, __shfl_xor(hi, off));
        }
        qp_minmax_pair(lo, hi, MAXQ, s, z);
    } else {
        s = scale_in[(size_t)row * ng + group];
        z = zero_in[(size_t)row * ng + group];
    }
    const float zs = z * s;
    const unsigned zcode = (unsigned)(int)qp_clamp<BITS>(z);        // what a dead column's nibble holds

    unsigned c[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const float q = FIND ? rintf(x[j] / s) + z : rintf((x[j] + zs) / s);
        c[j] = j < n_code ? (unsigned)(int)qp_clamp<BITS>(q) : zcode;
    }

    qp_emit<BITS>(c, qweight, G, row, group, chunk, lane);

    if (chunk == 0) {                                               // 16 lanes, 16 consecutive rows: the [n][G] -> [G][n] turn
        scales[(size_t)group * G.n + row] = (_Float16)s;
        scaled_zeros[(size_t)group * G.n + row] = (_Float16)(-zs);
        if (scale_out) scale_out[(size_t)row * ng + group] = s;
        if (zero_out) zero_out[(size_t)row * ng + group] = z;
    }
}

// Per-channel (qeft_quant_pack_pc; the contract and the split of the work: quant_pack.h): ONE pair per row.  A workgroup owns 16
// rows, its QPC_WAVES waves take the rows' 128-column groups in turn (wave, wave + QPC_WAVES, ..), lane = chunk * 16 + row as above.
template <int BITS, bool FIND, bool GATHER>
__global__ __launch_bounds__(QPC_THREADS) void quant_pack_pc_kernel(const _Float16* __restrict__ w, const int* __restrict__ col_ids,
                                                                    const float* __restrict__ scale_in, const float* __restrict__ zero_in,
                                                                    void* __restrict__ qweight, _Float16* __restrict__ scales,
                                                                    _Float16* __restrict__ scaled_zeros, float* __restrict__ scale_out,
                                                                    float* __restrict__ zero_out, QpGeom G) {
    constexpr float MAXQ = (float)((1 << BITS) - 1);
    __shared__ float ext[2][QPC_WAVES][QP_ROWS];                    // every wave's (min, max) of its groups, per row
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int chunk = lane >> 4, r16 = lane & 15;
    const int row = blockIdx.x * QP_ROWS + r16;                     // < n: n % 16 == 0
    const int live = qp_live(G);
    const _Float16* wrow = w + (size_t)row * G.ld_w;

    float s, z;
    if (FIND) {
        // ---- pass 1: the wave's extremes over the live columns of its groups, then one exchange through LDS
        float lo = 0.f, hi = 0.f;                                   // min and max do not round: any order gives the row's
        for (int group = wave; group * QP_GROUP < live; group += QPC_WAVES) {
            const int col0 = group * QP_GROUP + chunk * 32;         // col0 + 32 <= k
            const int n_read = min(max(live - col0, 0), 32);
            if (n_read > 0) {
                float x[32];
#pragma unroll
                for (int j = 0; j < 32; ++j) x[j] = 0.f;
                qp_read32<GATHER>(wrow, col_ids, col0, n_read, G.k, x);
#pragma unroll
                for (int j = 0; j < 32; ++j)
                    if (j < n_read) {
                        lo = fminf(lo, x[j]);
                        hi = fmaxf(hi, x[j]);
                    }
            }
        }
#pragma unroll
        for (int off = 16; off < 64; off <<= 1) {                   // the row's 4 lanes: lane ^ 16, lane ^ 32
            lo = fminf(lo, __shfl_xor(lo, off));
            hi = fmaxf(hi, __shfl_xor(hi, off));
        }
        if (chunk == 0) {
            ext[0][wave][r16] = lo;
            ext[1][wave][r16] = hi;
        }
        __syncthreads();                                            // the only barrier; every wave reaches it, with or without a group
#pragma unroll
        for (int v = 0; v < QPC_WAVES; ++v) {
            lo = fminf(lo, ext[0][v][r16]);
            hi = fmaxf(hi, ext[1][v][r16]);
        }
        qp_minmax_pair(lo, hi, MAXQ, s, z);
    } else {
        s = scale_in[row];
        z = zero_in[row];
    }
    const float zs = z * s;
    const unsigned zcode = (unsigned)(int)qp_clamp<BITS>(z);        // what a dead column's nibble holds

    // ---- pass 2: quantise and pack the wave's groups (find mode reads w a second time); the 3-bit stream ends with the live ones
    const int ngroups = BITS == 4 ? qp_groups(G) : live / QP_GROUP;
    for (int group = wave; group < ngroups; group += QPC_WAVES) {
        const int col0 = group * QP_GROUP + chunk * 32;
        const int n_code = min(max(live - col0, 0), 32);
        float x[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) x[j] = 0.f;
        if (n_code > 0) qp_read32<GATHER>(wrow, col_ids, col0, n_code, G.k, x);
        unsigned c[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const float q = FIND ? rintf(x[j] / s) + z : rintf((x[j] + zs) / s);
            c[j] = j < n_code ? (unsigned)(int)qp_clamp<BITS>(q) : zcode;
        }
        qp_emit<BITS>(c, qweight, G, row, group, chunk, lane);
    }

    if (wave == 0 && chunk == 0) {                                  // 16 lanes, 16 consecutive rows
        scales[row] = (_Float16)s;
        scaled_zeros[row] = (_Float16)(-zs);
        if (scale_out) scale_out[row] = s;
        if (zero_out) zero_out[row] = z;
    }
}

template <int BITS, bool FIND, bool GATHER>
static void qpc_launch(const void* w, const void* col_ids, const void* scale_in, const void* zero_in, void* qweight, void* scales,
                       void* scaled_zeros, void* scale_out, void* zero_out, const QpGeom& G, hipStream_t st) {
    hipLaunchKernelGGL((quant_pack_pc_kernel<BITS, FIND, GATHER>), dim3((unsigned)qp_grid_x(G)), dim3(QPC_THREADS), 0, st,
                       (const _Float16*)w, (const int*)col_ids, (const float*)scale_in, (const float*)zero_in, qweight,
                       (_Float16*)scales, (_Float16*)scaled_zeros, (float*)scale_out, (float*)zero_out, G);
}

hipError_t quant_pack_pc_launch(const void* w, const void* col_ids, const void* scale_in, const void* zero_in, void* qweight,
                                void* scales, void* scaled_zeros, void* scale_out, void* zero_out, const QpGeom& G, hipStream_t st) {
    const bool find = scale_in == nullptr, gather = col_ids != nullptr;
    g_last_variant = G.bits == 4 ? "quant_pack_pc_w4" : "quant_pack_pc_w3";
#define QPC_CASE(B, F, I) \
    if ((G.bits == B) && find == F && gather == I) qpc_launch<B, F, I>(w, col_ids, scale_in, zero_in, qweight, scales, scaled_zeros, scale_out, zero_out, G, st)
    QPC_CASE(3, false, false);
    QPC_CASE(3, false, true);
    QPC_CASE(3, true, false);
    QPC_CASE(3, true, true);
    QPC_CASE(4, false, false);
    QPC_CASE(4, false, true);
    QPC_CASE(4, true, false);
    QPC_CASE(4, true, true);
#undef QPC_CASE
    return hipGetLastError();
}

template <int BITS, bool FIND, bool GATHER>
static void qp_launch(const void* w, const void* col_ids, const void* scale_in, const void* zero_in, void* qweight, void* scales,
                      void* scaled_zeros, void* scale_out, void* zero_out, const QpGeom& G, hipStream_t st) {
    const dim3 grid((unsigned)qp_grid_x(G), (unsigned)qp_grid_y(G)), block(QP_THREADS);
    hipLaunchKernelGGL((quant_pack_kernel<BITS, FIND, GATHER>), grid, block, 0, st, (const _Float16*)w, (const int*)col_ids,
                       (const float*)scale_in, (const float*)zero_in, qweight, (_Float16*)scales, (_Float16*)scaled_zeros,
                       (float*)scale_out, (float*)zero_out, G);
}

hipError_t quant_pack_launch(const void* w, const void* col_ids, const void* scale_in, const void* zero_in, void* qweight, void* scales,
                             void* scaled_zeros, void* scale_out, void* zero_out, const QpGeom& G, hipStream_t st) {
    static const char* const names[8] = {"quant_pack_w3_given", "quant_pack_w3_given_ids", "quant_pack_w3_find", "quant_pack_w3_find_ids",
                                         "quant_pack_w4_given", "quant_pack_w4_given_ids", "quant_pack_w4_find", "quant_pack_w4_find_ids"};
    const bool find = scale_in == nullptr, gather = col_ids != nullptr;
    g_last_variant = names[(G.bits == 4) * 4 + find * 2 + gather];
#define QP_CASE(B, F, I) \
    if ((G.bits == B) && find == F && gather == I) qp_launch<B, F, I>(w, col_ids, scale_in, zero_in, qweight, scales, scaled_zeros, scale_out, zero_out, G, st)
    QP_CASE(3, false, false);
    QP_CASE(3, false, true);
    QP_CASE(3, true, false);
    QP_CASE(3, true, true);
    QP_CASE(4, false, false);
    QP_CASE(4, false, true);
    QP_CASE(4, true, false);
    QP_CASE(4, true, true);
#undef QP_CASE
    return hipGetLastError();
}

}  // namespace qeft
