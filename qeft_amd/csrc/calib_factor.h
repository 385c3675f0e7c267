// Geometry of the blocked factor of the inverse Hessian (calib_factor.hip; calibrate.hinv_factor).
//
// qeft_hinv_factor    A fp32 [k][k] (leading dimension ld), symmetric positive definite, k % 128 == 0 -> the upper-triangular U
//   with A^-1 = U^T U, what cholesky(cholesky_inverse(cholesky(A)), upper=True) returns, from ONE factorisation and one triangular
//   inverse: A = V V^T with V upper-triangular (a Cholesky factorisation that starts at the bottom-right corner), U = V^-1.
//
//   128-column blocks, nb = k / 128, swept j = nb - 1 .. 0; the steps are ordered by kernel boundaries alone (no flag, no ticket, no
//   atomics).  V overwrites the upper block triangle of A; the upper block triangle of U doubles as the accumulator T of the
//   inverse (T[i][l] = sum over m = i + 1 .. l of V[i][m] U[m][l], the sum U[i][l] = -D_i T[i][l] needs).  Step j, three launches:
//     diag   ONE workgroup of 1024 threads takes the reduced block A[j][j] (its upper triangle) into LDS and sweeps its columns
//            c = 127 .. 0: pivot check, d = sqrt(pivot), column c of V_jj = A[.][c] / d, the rank-1 update of the columns left of
//            c -- and in the same sweep, in place, the inverse D_j = V_jj^-1: row c of D is -T[c][.] / d, and the rank-1 update
//            v[r] * D[c][l] of the rows above feeds T for the columns c .. 127 (the element [r][c], whose V value has just been
//            consumed, starts that sum).  One array, two syncs per column; each element's 128 rank-1 terms are summed with a
//            Kahan compensation in fp32 (a second array): sequential fp32 sums at the magnitude of the diagonal cost 3 - 4 x
//            the error of the whole factor at K = 128.  D_j goes to U[j][j] with zeros below the diagonal.
//     row    nb - 1 workgroups: block i < j forms the panel V[i][j] = A[i][j] D_j^T in place (a multiply by the inverted diagonal
//            block, not a substitution) and writes the zero block U[j][i]; block l > j finishes U[j][l] = -D_j T[j][l] in place.
//     trail  j (j + 1) / 2 workgroups A[i][l] -= V[i][j] V[l][j]^T for i <= l < j, and j (nb - j) workgroups
//            T[i][l] (+)= V[i][j] U[j][l] for i < j <= l (l == j writes, it is the sum's first term).
//   row and trail are one kernel: a 128 x 128 output tile per workgroup of 4 waves (2 x 2, 64 x 64 each = 2 x 2 accumulators of
//   v_mfma_f32_32x32x2f32), depth 128 in chunks of HF_BK = 32 staged k-major through LDS ([32][130] floats per operand: the
//   matrix unit's operand read is then 32 consecutive words per half-wave, and the transposing store of a row-major operand
//   spreads over the banks), the next chunk's global loads in flight during the MFMAs.  fp32 throughout; every sum has one order
//   (ascending k inside a tile, descending j across steps).  3 nb - 1 launches (1 for nb == 1).
//
//   Every element of U is written exactly once as a final value (diag: U[j][j]; row: U[j][l != j]); A is destroyed.
#pragma once
#include <hip/hip_runtime.h>

namespace qeft {

constexpr int HF_B = 128;                               // block edge
constexpr int HF_MAX_K = 1 << 15;
constexpr int HF_DIAG_THREADS = 1024;
constexpr int HF_DIAG_LD = HF_B + 1;                    // row stride of the diagonal block in LDS: a column walk hits every bank
constexpr int HF_DIAG_LDS = (2 * HF_B * HF_DIAG_LD + 2 * HF_B) * 4;  // the block, its compensation, v and w: 133 120 bytes
constexpr int HF_TILE_THREADS = 256;
constexpr int HF_BK = 32;                               // depth of a staged chunk
constexpr int HF_LDP = HF_B + 2;                        // row stride of a staged chunk (k-major)

struct HfGeom {
    int k, ld;
};

inline int hf_nb(const HfGeom& G) { return G.k / HF_B; }
inline int hf_launches(const HfGeom& G) { return hf_nb(G) == 1 ? 1 : 3 * hf_nb(G) - 1; }
__host__ __device__ inline int hf_row_blocks(int nb) { return nb - 1; }
__host__ __device__ inline int hf_tri(int j) { return j * (j + 1) / 2; }
__host__ __device__ inline int hf_trail_blocks(int nb, int j) { return hf_tri(j) + j * (nb - j); }

// ---- host side: calib_factor.hip
hipError_t hinv_factor_launch(void* a, void* u, int* info, const HfGeom& G, hipStream_t st);

}  // namespace qeft
