// The blocked factor of the inverse Hessian (qeft_amd/calibrate.py: hinv_factor, factor="own").  The
// algorithm, the split of the work and the launch sequence: calib_factor.h.
//
// Every global address is a block origin (bi * 128) * ld + bj * 128 with bi, bj < nb = k / 128, plus row * ld + column with
// row, column < 128: inside [k][ld] whatever the values are, so a matrix that is not positive definite costs a status, not a fault.
#include <float.h>
#include <math.h>

#include "qeft_common.h"
#include "calib_factor.h"

namespace qeft {

typedef float hf_acc_t __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------- the diagonal block: V_jj and D_j = V_jj^-1 in one sweep
__global__ __launch_bounds__(HF_DIAG_THREADS) void hf_diag_kernel(const float* A, int ld, float* U, int k, int j, int nb, int* info) {
    extern __shared__ __attribute__((aligned(16))) float hf_smem[];
    float* X = hf_smem;                                     // [128][129]: S left of the sweep, T / D from it on
    float* E = X + HF_B * HF_DIAG_LD;                       // [128][129]: the compensation of X's running sums (the value is X - E)
    float* vs = E + HF_B * HF_DIAG_LD;                      // column c of V_jj above the diagonal
    float* ws = vs + HF_B;                                  // the row the rank-1 update multiplies by: -v left of c, D[c][.] from c on
    __shared__ int bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* Ajj = A + ((size_t)j * HF_B) * ld + (size_t)j * HF_B;
    float* Ujj = U + ((size_t)j * HF_B) * k + (size_t)j * HF_B;
    for (int idx = tid; idx < HF_B * HF_B; idx += HF_DIAG_THREADS) {
        const int r = idx >> 7, l = idx & 127;
        X[r * HF_DIAG_LD + l] = l >= r ? Ajj[(size_t)r * ld + l] : 0.f;
        E[r * HF_DIAG_LD + l] = 0.f;
    }
    if (tid == 0) bad = 0;
    __syncthreads();
    for (int c = HF_B - 1; c >= 0; --c) {
        const float p = X[c * HF_DIAG_LD + c] - E[c * HF_DIAG_LD + c];
        if (tid == 0 && bad == 0 && !(p > 0.f && p <= FLT_MAX)) bad = c + 1;
        const float rinv = 1.0f / sqrtf(p);
        if (tid < HF_B) {
            if (tid < c) {
                const float v = (X[tid * HF_DIAG_LD + c] - E[tid * HF_DIAG_LD + c]) * rinv;
                vs[tid] = v;
                ws[tid] = -v;
            } else {
                ws[tid] = tid == c ? rinv : -(X[c * HF_DIAG_LD + tid] - E[c * HF_DIAG_LD + tid]) * rinv;
            }
        }
        __syncthreads();
        if (tid >= c && tid < HF_B) {                       // row c of D is final
            X[c * HF_DIAG_LD + tid] = ws[tid];
            E[c * HF_DIAG_LD + tid] = 0.f;
        }
        for (int r = wave; r < c; r += HF_DIAG_THREADS / 64) {
            const float vr = vs[r];
            for (int l = lane; l < HF_B; l += 64)
                if (l >= r) {                               // a Kahan step: 128 rank-1 terms per element, summed as if in one rounding
                    const float x = l == c ? 0.f : X[r * HF_DIAG_LD + l], e = l == c ? 0.f : E[r * HF_DIAG_LD + l];
                    const float y = vr * ws[l] - e, s = x + y;
                    E[r * HF_DIAG_LD + l] = (s - x) - y;
                    X[r * HF_DIAG_LD + l] = s;
                }
        }
        __syncthreads();
    }
    for (int idx = tid; idx < HF_B * HF_B; idx += HF_DIAG_THREADS) {
        const int r = idx >> 7, l = idx & 127;
        Ujj[(size_t)r * k + l] = l >= r ? X[r * HF_DIAG_LD + l] - E[r * HF_DIAG_LD + l] : 0.f;
    }
    if (tid == 0) {                                         // the first step of the sweep starts the status; no memset
        int cur = j == nb - 1 ? 0 : *info;
        if (cur == 0 && bad != 0) cur = j * HF_B + bad;
        *info = cur;
    }
}

// ---------------------------------------------------------------- one 128 x 128 tile: C = alpha * A op(B) (+ C)
// A [128][128] row-major (k contiguous).  B: NN = false -> [c][k] (the product is A B^T), NN = true -> [k][c].  C may be A or B
// itself: every chunk of both is in registers or LDS before the first store.
template <bool NN>
__device__ __forceinline__ void hf_tile(const float* Ap, int lda, const float* Bp, int ldb, float* Cp, int ldc, float alpha,
                                        bool add_c, float* As, float* Bs) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int kq = tid & 7, r0 = tid >> 3;                  // row-major operand: 8 float4 per row of a chunk, 32 rows per pass
    const int cq = tid & 31, kr0 = tid >> 5;                // k-major operand: 32 float4 per k, 8 k per pass
    hf_acc_t acc[2][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mt][nt][e] = 0.f;
    float4 ra[4], rb[4];
    auto load = [&](int k0) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            ra[p] = *(const float4*)(Ap + (size_t)(r0 + 32 * p) * lda + k0 + 4 * kq);
            if (NN)
                rb[p] = *(const float4*)(Bp + (size_t)(k0 + kr0 + 8 * p) * ldb + 4 * cq);
            else
                rb[p] = *(const float4*)(Bp + (size_t)(r0 + 32 * p) * ldb + k0 + 4 * kq);
        }
    };
    auto store_t = [&](float* S, const float4& v, int r) {  // a row-major piece, transposed into the k-major image
        S[(4 * kq + 0) * HF_LDP + r] = v.x;
        S[(4 * kq + 1) * HF_LDP + r] = v.y;
        S[(4 * kq + 2) * HF_LDP + r] = v.z;
        S[(4 * kq + 3) * HF_LDP + r] = v.w;
    };
    load(0);
    for (int k0 = 0; k0 < HF_B; k0 += HF_BK) {
        __syncthreads();                                    // the last chunk's readers have left the images
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            store_t(As, ra[p], r0 + 32 * p);
            if (NN) {
                float* d = Bs + (kr0 + 8 * p) * HF_LDP + 4 * cq;          // 8-byte aligned: HF_LDP is even
                *(float2*)d = make_float2(rb[p].x, rb[p].y);
                *(float2*)(d + 2) = make_float2(rb[p].z, rb[p].w);
            } else {
                store_t(Bs, rb[p], r0 + 32 * p);
            }
        }
        __syncthreads();
        if (k0 + HF_BK < HF_B) load(k0 + HF_BK);
#pragma unroll
        for (int kk = 0; kk < HF_BK; kk += 2) {
            const int kl = kk + (lane >> 5);
            float a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t] = As[kl * HF_LDP + wm * 64 + t * 32 + (lane & 31)];
                b[t] = Bs[kl * HF_LDP + wn * 64 + t * 32 + (lane & 31)];
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
        }
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = wm * 64 + mt * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5), col = wn * 64 + nt * 32 + (lane & 31);
                float* c = Cp + (size_t)row * ldc + col;
                float v = alpha * acc[mt][nt][e];
                if (add_c) v += *c;
                *c = v;
            }
}

// phase 0: the row launch of step j (hf_row_blocks workgroups); phase 1: the trailing launch (hf_trail_blocks workgroups)
__global__ __launch_bounds__(HF_TILE_THREADS) void hf_tile_kernel(float* A, int ld, float* U, int k, int j, int nb, int phase) {
    __shared__ __attribute__((aligned(16))) float As[HF_BK * HF_LDP];
    __shared__ __attribute__((aligned(16))) float Bs[HF_BK * HF_LDP];
    const int b = blockIdx.x;
    auto a_blk = [&](int bi, int bj) { return A + ((size_t)bi * HF_B) * ld + (size_t)bj * HF_B; };
    auto u_blk = [&](int bi, int bj) { return U + ((size_t)bi * HF_B) * k + (size_t)bj * HF_B; };
    if (phase == 0) {
        if (b < j) {                                        // the panel V[b][j] = A[b][j] D_j^T, and the zero block U[j][b]
            hf_tile<false>(a_blk(b, j), ld, u_blk(j, j), k, a_blk(b, j), ld, 1.f, false, As, Bs);
            float* z = u_blk(j, b);
            for (int idx = threadIdx.x; idx < HF_B * HF_B / 4; idx += HF_TILE_THREADS)
                *(float4*)(z + (size_t)(idx >> 5) * k + 4 * (idx & 31)) = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {                                            // U[j][l] = -D_j T[j][l]
            const int l = b + 1;
            hf_tile<true>(u_blk(j, j), k, u_blk(j, l), k, u_blk(j, l), k, -1.f, false, As, Bs);
        }
        return;
    }
    if (b < hf_tri(j)) {                                    // A[i][l] -= V[i][j] V[l][j]^T, i <= l < j
        int l = 0;
        while (b >= hf_tri(l + 1)) ++l;
        const int i = b - hf_tri(l);
        hf_tile<false>(a_blk(i, j), ld, a_blk(l, j), ld, a_blk(i, l), ld, -1.f, true, As, Bs);
    } else {                                                // T[i][l] (+)= V[i][j] U[j][l], i < j <= l
        const int bb = b - hf_tri(j), i = bb % j, l = j + bb / j;
        hf_tile<true>(a_blk(i, j), ld, u_blk(j, l), k, u_blk(i, l), k, 1.f, l != j, As, Bs);
    }
}

hipError_t hinv_factor_launch(void* a, void* u, int* info, const HfGeom& G, hipStream_t st) {
    g_last_variant = "hinv_factor_b128";
    if (hipError_t e = hipFuncSetAttribute((const void*)hf_diag_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, HF_DIAG_LDS)) return e;
    const int nb = hf_nb(G);
    float* A = (float*)a;
    float* U = (float*)u;
    for (int j = nb - 1; j >= 0; --j) {
        hipLaunchKernelGGL(hf_diag_kernel, dim3(1), dim3(HF_DIAG_THREADS), HF_DIAG_LDS, st, (const float*)A, G.ld, U, G.k, j, nb, info);
        if (nb > 1)
            hipLaunchKernelGGL(hf_tile_kernel, dim3((unsigned)hf_row_blocks(nb)), dim3(HF_TILE_THREADS), 0, st, A, G.ld, U, G.k, j, nb, 0);
        if (j > 0)
            hipLaunchKernelGGL(hf_tile_kernel, dim3((unsigned)hf_trail_blocks(nb, j)), dim3(HF_TILE_THREADS), 0, st, A, G.ld, U, G.k, j, nb, 1);
    }
    return hipGetLastError();
}

}  // namespace qeft
