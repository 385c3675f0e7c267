// Calibration kernels (qeft_amd/calibrate.py): the Hessian accumulation H <- beta H + alpha X^T X and one
// block of the GPTQ error-feedback loop.  Contracts, grids and the pinned arithmetic: calib.h.  Nothing below may be contracted
// into an FMA (the epilogue of the first kernel, every line of the second), hence the pragma over the whole file.
//
// Every global address comes from calib.h; hessian_accum_count_out_of_range walks the same functions on the CPU.
#include <vector>

#include "qeft_common.h"
#include "calib.h"

#pragma clang fp contract(off)

namespace qeft {

// ---------------------------------------------------------------- H <- beta H + alpha X^T X
// The 8 transposing reads of one k-step (a: tile ti, 2 subtiles x 2 row quads; b: tile tj likewise) and their wait in ONE asm
// statement: the compiler does not count asm loads in lgkmcnt, so nothing may sit between the reads and the wait.  The read
// needs EXEC all ones: the row-tile loop and the k-steps are uniform, and every lane's address is inside the image.
__device__ __forceinline__ void ha_read_step(const uint32_t (&aa)[4], const uint32_t (&ba)[4], uint32_t step, u32x2 (&fa)[4],
                                             u32x2 (&fb)[4]) {
    asm volatile(
        "ds_read_b64_tr_b16 %0, %8\n"
        "ds_read_b64_tr_b16 %1, %9\n"
        "ds_read_b64_tr_b16 %2, %10\n"
        "ds_read_b64_tr_b16 %3, %11\n"
        "ds_read_b64_tr_b16 %4, %12\n"
        "ds_read_b64_tr_b16 %5, %13\n"
        "ds_read_b64_tr_b16 %6, %14\n"
        "ds_read_b64_tr_b16 %7, %15\n"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(fa[0]), "=&v"(fa[1]), "=&v"(fa[2]), "=&v"(fa[3]), "=&v"(fb[0]), "=&v"(fb[1]), "=&v"(fb[2]), "=&v"(fb[3])
        : "v"(aa[0] + step), "v"(aa[1] + step), "v"(aa[2] + step), "v"(aa[3] + step), "v"(ba[0] + step), "v"(ba[1] + step),
          "v"(ba[2] + step), "v"(ba[3] + step)
        : "memory");
}

__global__ __launch_bounds__(HA_THREADS) void hessian_accum_kernel(const f16* __restrict__ x, float* __restrict__ H, HaGeom G,
                                                                   float alpha, float beta) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * 2 * HA_IMG_BYTES];       // [2 buffers][image of ti | image of tj]
    const uint32_t lds0 = (uint32_t)(uintptr_t)lds;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int r = lane & 31, h = lane >> 5;
    int ti, tj;
    ha_block_tile(G, blockIdx.x, ti, tj);
    const bool diag = ti == tj;                             // one image serves both operands
    const int ktiles = ha_row_tiles(G);

    u32x4 ra[4], rb[4];
    auto load = [&](int kt) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int trow = ha_stage_row(p, tid), slot = ha_stage_slot(p, tid);
            const long long oa = ha_x_off(G, ti, trow, slot, kt);
            ra[p] = oa >= 0 ? *(const u32x4*)(x + oa) : u32x4{0u, 0u, 0u, 0u};
            if (!diag) {
                const long long ob = ha_x_off(G, tj, trow, slot, kt);
                rb[p] = ob >= 0 ? *(const u32x4*)(x + ob) : u32x4{0u, 0u, 0u, 0u};
            }
        }
    };
    auto stage = [&](int kt) {
        unsigned char* base = lds + (kt & 1) * 2 * HA_IMG_BYTES;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int off = ha_stage_row(p, tid) * 256 + ha_stage_slot(p, tid) * 16;
            *(u32x4*)(base + off) = ra[p];
            if (!diag) *(u32x4*)(base + HA_IMG_BYTES + off) = rb[p];
        }
    };

    f32x16 acc[2][2];                                       // [a subtile nt][b subtile tt] of the wave's 64 x 64
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[nt][tt][e] = 0.f;

    uint32_t aoff[4], boff[4];                              // [2 sub + quad]
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int quad = 0; quad < 2; ++quad) {
            aoff[2 * s + quad] = (uint32_t)ha_frag_off(lane, wm, s, quad);
            boff[2 * s + quad] = (uint32_t)((diag ? 0 : HA_IMG_BYTES) + ha_frag_off(lane, wn, s, quad));
        }

    load(0);
    for (int kt = 0; kt < ktiles; ++kt) {
        stage(kt);                                          // buffer kt & 1: everyone left it before the barrier of tile kt - 1
        if (kt + 1 < ktiles) load(kt + 1);                  // in flight behind this tile's MFMAs
        __syncthreads();
        const uint32_t tb = lds0 + (uint32_t)(kt & 1) * 2 * HA_IMG_BYTES;
        uint32_t aa[4], ba[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            aa[i] = tb + aoff[i];
            ba[i] = tb + boff[i];
        }
#pragma unroll
        for (int ks = 0; ks < HA_BT / 16; ++ks) {
            u32x2 fa[4], fb[4];
            ha_read_step(aa, ba, (uint32_t)(ks * 16 * 256), fa, fb);
            h8 a[2], b[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                a[s] = __builtin_bit_cast(h8, u32x4{fa[2 * s][0], fa[2 * s][1], fa[2 * s + 1][0], fa[2 * s + 1][1]});
                b[s] = __builtin_bit_cast(h8, u32x4{fb[2 * s][0], fb[2 * s][1], fb[2 * s + 1][0], fb[2 * s + 1][1]});
            }
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) acc[nt][tt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[nt], b[tt], acc[nt][tt], 0, 0, 0);
        }
    }

    // ---- epilogue: register e of acc[nt][tt] is S[ha_acc_row][ha_acc_col]; 4 consecutive registers are 4 consecutive rows i of
    // one column j, i.e. 4 adjacent elements of row j of the mirrored tile
    const bool keep = beta != 0.f;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int j = ha_acc_col(tj, wn, tt, r);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i0 = ha_acc_row(ti, wm, nt, h, 4 * q);
                f32x4 v;
                bool live[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int i = i0 + c;
                    live[c] = i < G.k && j < G.k && i <= j;              // (off the diagonal tiles i < j always)
                    v[c] = 0.f;
                    if (live[c]) {
                        const float old = keep ? H[ha_h_off(G, i, j)] : 0.f;
                        const float bh = beta * old;
                        const float as = alpha * acc[nt][tt][4 * q + c];
                        v[c] = bh + as;
                        H[ha_h_off(G, i, j)] = v[c];
                    }
                }
                if (live[3] && i0 + 3 < j) {                            // live[3] implies the other three
                    *(f32x4*)(H + ha_h_off(G, j, i0)) = v;
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (live[c] && i0 + c < j) H[ha_h_off(G, j, i0 + c)] = v[c];
                }
            }
        }
}

hipError_t hessian_accum_launch(const void* x, void* h, const HaGeom& G, float alpha, float beta, hipStream_t st) {
    g_last_variant = "hessian_accum_128x128";
    hipLaunchKernelGGL(hessian_accum_kernel, dim3((unsigned)ha_blocks(G)), dim3(HA_THREADS), 0, st, (const f16*)x, (float*)h, G, alpha,
                       beta);
    return hipGetLastError();
}

// Every global address a launch forms, on the CPU: how many of the 16-byte reads of X leave [0, T K) and how many of the accesses
// of H leave [0, K K), plus the elements of H that are not written exactly once (a hole or an overlap in the tile map is as wrong
// as a stray address; an element read must be the one its thread then writes, so reads are counted with the direct stores).
long long hessian_accum_count_out_of_range(const HaGeom& G) {
    const long long x_n = (long long)G.t * G.k, h_n = (long long)G.k * G.k;
    long long bad = 0;
    std::vector<unsigned char> written((size_t)h_n, 0);
    auto write = [&](long long off, int n) {
        if (off < 0 || off + n > h_n) {
            ++bad;
            return;
        }
        for (int c = 0; c < n; ++c)
            if (written[(size_t)(off + c)] < 255) ++written[(size_t)(off + c)];
    };
    for (int block = 0; block < ha_blocks(G); ++block) {
        int ti, tj;
        ha_block_tile(G, block, ti, tj);
        if (ti < 0 || tj < ti || tj >= ha_tiles(G)) ++bad;
        for (int kt = 0; kt < ha_row_tiles(G); ++kt)
            for (int p = 0; p < 4; ++p)
                for (int tid = 0; tid < HA_THREADS; ++tid)
                    for (int tile : {ti, tj}) {
                        const long long o = ha_x_off(G, tile, ha_stage_row(p, tid), ha_stage_slot(p, tid), kt);
                        if (o == -1) continue;                           // the kernel's own guard: zeros, no address
                        if (o < 0 || o + 8 > x_n) ++bad;
                    }
        for (int wave = 0; wave < 4; ++wave)
            for (int lane = 0; lane < 64; ++lane)
                for (int nt = 0; nt < 2; ++nt)
                    for (int tt = 0; tt < 2; ++tt)
                        for (int q = 0; q < 4; ++q) {
                            const int j = ha_acc_col(tj, wave & 1, tt, lane & 31), i0 = ha_acc_row(ti, wave >> 1, nt, lane >> 5, 4 * q);
                            bool live[4];
                            for (int c = 0; c < 4; ++c) {
                                live[c] = i0 + c < G.k && j < G.k && i0 + c <= j;
                                if (live[c]) write(ha_h_off(G, i0 + c, j), 1);
                            }
                            if (live[3] && i0 + 3 < j) {
                                if (ha_h_off(G, j, i0) % 4 != 0) ++bad;  // a 16-byte store
                                write(ha_h_off(G, j, i0), 4);
                            } else {
                                for (int c = 0; c < 4; ++c)
                                    if (live[c] && i0 + c < j) write(ha_h_off(G, j, i0 + c), 1);
                            }
                        }
    }
    for (long long e = 0; e < h_n; ++e)
        if (written[(size_t)e] != 1) ++bad;
    return bad;
}

// ---------------------------------------------------------------- one block of the error-feedback loop
// The loop over the block's columns is unrolled in full so that the row stays in registers; a column >= count is skipped by a
// uniform branch and its triangle entries are zeros that nothing stores.
__global__ __launch_bounds__(GB_THREADS) void gptq_block_kernel(float* __restrict__ W1, const float* __restrict__ Hinv1,
                                                                const float* __restrict__ scale, const float* __restrict__ zero,
                                                                float* __restrict__ Q1, float* __restrict__ Err1, GbGeom G, float maxq) {
    __shared__ __attribute__((aligned(16))) float hs[GB_MAX_COUNT * GB_MAX_COUNT];          // row i: Hinv1[i][i ..], zeros elsewhere
    const int tid = threadIdx.x, count = G.count;
    for (int idx = tid; idx < GB_MAX_COUNT * GB_MAX_COUNT; idx += GB_THREADS) {
        const int i = idx / GB_MAX_COUNT, j = idx % GB_MAX_COUNT;
        hs[idx] = (i < count && j < count && j >= i) ? Hinv1[(size_t)i * G.ld_h + j] : 0.f;
    }
    __syncthreads();
    const int row = blockIdx.x * GB_THREADS + tid;
    const bool live = row < G.n;
    const int rc = live ? row : G.n - 1;                    // a thread past N repeats the last row and stores nothing
    float* wrow = W1 + (size_t)rc * G.ld_w;
    float w[GB_MAX_COUNT];
#pragma unroll
    for (int j = 0; j < GB_MAX_COUNT; ++j) w[j] = j < count ? wrow[j] : 0.f;
    const float s = scale[rc], z = zero[rc];
    float* qrow = Q1 + (size_t)rc * count;
    float* erow = Err1 + (size_t)rc * count;
#pragma unroll
    for (int i = 0; i < GB_MAX_COUNT; ++i) {
        if (i < count) {
            const float d = hs[i * GB_MAX_COUNT + i];
            const float xs = w[i] / s;
            const float c = fminf(fmaxf(rintf(xs) + z, 0.f), maxq);
            const float q = s * (c - z);
            const float e = (w[i] - q) / d;
            if (live) {
                qrow[i] = q;
                erow[i] = e;
            }
#pragma unroll
            for (int j = i; j < GB_MAX_COUNT; ++j) {
                const float p = e * hs[i * GB_MAX_COUNT + j];
                w[j] = w[j] - p;
            }
        }
    }
    if (live) {
#pragma unroll
        for (int j = 0; j < GB_MAX_COUNT; ++j)
            if (j < count) wrow[j] = w[j];
    }
}

hipError_t gptq_block_launch(void* w1, const void* hinv1, const void* scale, const void* zero, void* q1, void* err1, const GbGeom& G,
                             float maxq, hipStream_t st) {
    g_last_variant = "gptq_block_row_per_lane";
    hipLaunchKernelGGL(gptq_block_kernel, dim3((unsigned)gb_blocks(G)), dim3(GB_THREADS), 0, st, (float*)w1, (const float*)hinv1,
                       (const float*)scale, (const float*)zero, (float*)q1, (float*)err1, G, maxq);
    return hipGetLastError();
}

}  // namespace qeft
