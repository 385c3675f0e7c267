// Fused lm_head + cross-entropy pieces (qeft_lm_head_nll).
//
// logit[i][j] = sum_k x[i][k] w[j][k] in fp32 by v_mfma_f32_32x32x16_f16, never stored: per row the launch pair returns
// lse = log sum_j exp(logit), the logit at the row's target and the first argmax.  Both operands are K-contiguous (the NT GEMM), so
// both tiles reach LDS as they lie, by 16-byte LDS-DMA from source addresses that carry the bank swizzle.
//
//   launch 1  lm_head_nll_kernel<NW>: a block of NW waves owns 32 NW rows x 128 vocabulary columns, the columns at an ABSOLUTE
//             multiple of 128.  The vocabulary is the MFMA's row index and the token its column index, so a lane ends with 64
//             logits of ONE token in registers (lane ^ 32 holds the tile's other 64): the tile's max, first argmax and
//             sum exp(l - max) are register work plus one exchange with lane ^ 32.  One partial {max, sum, arg} per (row, tile)
//             goes to the workspace; the tile that owns the target column stores tgt_logit.
//   launch 2  lm_head_nll_reduce_kernel: one thread per row folds the row's partials in ascending tile order.
//
// A wave's work is the same instruction sequence on the same values whatever NW, t, the row's place in the launch or x_stride
// are: a row's three results depend on that row and the weight alone, bit for bit.  No atomics, no arrival order.
// Rows >= t and columns >= vocab are loaded from the clamped row / column (never past an operand's end) and never stored.
// Every global offset comes from the ln_* functions (lm_head_nll_body.h, ln_ws_off below); lm_head_nll_count_out_of_range walks
// the same functions on the CPU.  The k loop lives in lm_head_nll_body.h, shared with the backward (lm_head_nll_grad.hip).
#include "lm_head_nll_body.h"
#include "host_launch.h"

namespace qeft {

// workspace: three planes [col tile][t] of 4-byte words -- max, sum exp(l - max), first argmax
LN_HD long long ln_ws_off(const LnGeom& G, int plane, int col_tile, int row) {
    return ((long long)plane * ln_col_tiles(G) + col_tile) * G.t + row;
}

size_t lm_head_nll_workspace_bytes(int t, int vocab) {
    return (size_t)12 * t * ((vocab + LN_BN - 1) / LN_BN);
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void lm_head_nll_kernel(const f16* __restrict__ x, const f16* __restrict__ w,
                                                               const int* __restrict__ targets, float* __restrict__ tgt_logit,
                                                               float* __restrict__ ws, LnGeom G) {
    constexpr int BM = LnTile<NW>::BM;
    __shared__ __attribute__((aligned(16))) unsigned char lds[LnTile<NW>::LDS_BYTES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int row_tile = ln_block_row_tile(G, NW, blockIdx.x), col_tile = ln_block_col_tile(G, NW, blockIdx.x);

    f32x16 acc[4];
    ln_logit_tile<NW>(x, w, G, row_tile, col_tile, lds, acc);      // the k loop (lm_head_nll_body.h)

    // ---- epilogue: register e of tile vt is the logit of column col0 + 32 vt + (e & 3) + 8 (e >> 2) + 4 h, token row0 + r
    const int row = row_tile * BM + wave * 32 + r;
    const bool row_ok = row < G.t;
    const int col0 = col_tile * LN_BN;
    const int tg = targets != nullptr && row_ok ? targets[row] : -1;
    const int tloc = ln_target_ok(G, tg) ? tg - col0 : -1;     // the target's column in this tile (this lane's or not), or outside
    const float ninf = -__builtin_inff();
    float mx = ninf, tval = 0.f;
    int arg = col0;
    bool mine = false;
#pragma unroll
    for (int vt = 0; vt < 4; ++vt)
#pragma unroll
        for (int e = 0; e < 16; ++e) {                         // ascending columns: > keeps the lowest index among equal maxima
            const int c = vt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            const float v = col0 + c < G.vocab ? acc[vt][e] : ninf;
            acc[vt][e] = v;
            if (v > mx) { mx = v; arg = col0 + c; }
            if (c == tloc) { tval = v; mine = true; }
        }
    {
        const float omx = __shfl_xor(mx, 32);
        const int oarg = __shfl_xor(arg, 32);
        if (omx > mx || (omx == mx && oarg < arg)) { mx = omx; arg = oarg; }
    }
    float s = 0.f;
#pragma unroll
    for (int vt = 0; vt < 4; ++vt)
#pragma unroll
        for (int e = 0; e < 16; ++e) s += __expf(acc[vt][e] - mx);        // exp(-inf) = 0 on the masked columns
    s += __shfl_xor(s, 32);
    if (row_ok && h == 0) {
        ws[ln_ws_off(G, 0, col_tile, row)] = mx;
        ws[ln_ws_off(G, 1, col_tile, row)] = s;
        ((int*)ws)[ln_ws_off(G, 2, col_tile, row)] = arg;
    }
    if (row_ok && mine) tgt_logit[row] = tval;
}

__global__ __launch_bounds__(LN_RED_THREADS) void lm_head_nll_reduce_kernel(const float* __restrict__ ws, const int* __restrict__ targets,
                                                                            float* __restrict__ lse, float* __restrict__ tgt_logit,
                                                                            int* __restrict__ argmax, LnGeom G) {
    const int row = blockIdx.x * LN_RED_THREADS + threadIdx.x;
    if (row >= G.t) return;
    const int tiles = ln_col_tiles(G);
    float mx = ws[ln_ws_off(G, 0, 0, row)];
    int arg = ((const int*)ws)[ln_ws_off(G, 2, 0, row)];
    for (int j = 1; j < tiles; ++j) {                           // ascending tiles: > keeps the lowest index
        const float m = ws[ln_ws_off(G, 0, j, row)];
        if (m > mx) { mx = m; arg = ((const int*)ws)[ln_ws_off(G, 2, j, row)]; }
    }
    float s = 0.f;
    for (int j = 0; j < tiles; ++j) s += ws[ln_ws_off(G, 1, j, row)] * expf(ws[ln_ws_off(G, 0, j, row)] - mx);
    lse[row] = mx + logf(s);
    if (argmax != nullptr) argmax[row] = arg;
    if (targets != nullptr && !ln_target_ok(G, targets[row])) tgt_logit[row] = 0.f;
}

hipError_t lm_head_nll_launch(const void* x, const void* w, const int* targets, float* lse, float* tgt_logit, int* argmax, void* ws,
                              int x_stride, int t, int hidden, int vocab, hipStream_t st) {
    const LnGeom G{x_stride, t, hidden, vocab};
    g_last_variant = "lm_head_nll";
    const int nw = ln_waves(G);
    const dim3 grid((unsigned)(ln_row_tiles(G, nw) * ln_col_tiles(G)));
    if (nw == 2)
        hipLaunchKernelGGL(lm_head_nll_kernel<2>, grid, dim3(128), 0, st, (const f16*)x, (const f16*)w, targets, tgt_logit, (float*)ws, G);
    else
        hipLaunchKernelGGL(lm_head_nll_kernel<4>, grid, dim3(256), 0, st, (const f16*)x, (const f16*)w, targets, tgt_logit, (float*)ws, G);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lm_head_nll_reduce_kernel, dim3((t + LN_RED_THREADS - 1) / LN_RED_THREADS), dim3(LN_RED_THREADS), 0, st,
                       (const float*)ws, targets, lse, tgt_logit, argmax, G);
    return hipGetLastError();
}

// Every global address the two launches form, on the CPU: the largest number of bytes by which one of them passes the end of its
// operand (x: t rows at x_stride, the last `hidden` wide; w: [vocab][hidden]; the workspace: lm_head_nll_workspace_bytes; targets
// and the three outputs: t words), or runs in front of it; 0 when none does.  An x address does not depend on the block's
// column tile, nor a weight address on its row tile, so each is visited once per row tile / column tile.
long long lm_head_nll_count_out_of_range(int x_stride, int t, int hidden, int vocab) {
    const LnGeom G{x_stride, t, hidden, vocab};
    const int nw = ln_waves(G), ktiles = hidden / LN_BK, rts = ln_row_tiles(G, nw), cts = ln_col_tiles(G);
    const long long x_bytes = 2 * ((long long)(t - 1) * x_stride + hidden), w_bytes = 2 * (long long)vocab * hidden;
    const long long ws_bytes = (long long)lm_head_nll_workspace_bytes(t, vocab), row_bytes = 4 * (long long)t;
    long long worst = 0;
    auto touch = [&](long long b, int bytes, long long operand_bytes) {
        if (b < 0 && -b > worst) worst = -b;
        if (b + bytes - operand_bytes > worst) worst = b + bytes - operand_bytes;
    };
    for (int rt = 0; rt < rts; ++rt)
        for (int trow = 0; trow < 32 * nw; ++trow)
            for (int slot = 0; slot < 8; ++slot)
                for (int kt = 0; kt < ktiles; ++kt) touch(2 * ln_x_off(G, rt, nw, trow, slot, kt), 16, x_bytes);
    for (int ct = 0; ct < cts; ++ct)
        for (int trow = 0; trow < LN_BN; ++trow)
            for (int slot = 0; slot < 8; ++slot)
                for (int kt = 0; kt < ktiles; ++kt) touch(2 * ln_w_off(G, ct, trow, slot, kt), 16, w_bytes);
    for (int block = 0; block < rts * cts; ++block) {
        const int rt = ln_block_row_tile(G, nw, block), ct = ln_block_col_tile(G, nw, block);
        for (int i = 0; i < 32 * nw; ++i) {
            const int row = rt * 32 * nw + i;
            if (row >= t) continue;
            touch(4 * (long long)row, 4, row_bytes);                                  // targets[row], tgt_logit[row]
            for (int plane = 0; plane < 3; ++plane) touch(4 * ln_ws_off(G, plane, ct, row), 4, ws_bytes);
        }
    }
    for (int block = 0; block < (t + LN_RED_THREADS - 1) / LN_RED_THREADS; ++block)
        for (int i = 0; i < LN_RED_THREADS; ++i) {
            const int row = block * LN_RED_THREADS + i;
            if (row >= t) continue;
            touch(4 * (long long)row, 4, row_bytes);                                  // lse, argmax, targets, tgt_logit
            for (int j = 0; j < cts; ++j)
                for (int plane = 0; plane < 3; ++plane) touch(4 * ln_ws_off(G, plane, j, row), 4, ws_bytes);
        }
    return worst;
}

}  // namespace qeft
