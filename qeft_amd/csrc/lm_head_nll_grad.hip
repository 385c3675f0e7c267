// Backward of the fused lm_head + cross-entropy (qeft_lm_head_nll_grad).
//
// dx[i][k] = grad_nll[i] * sum_j (p_ij - [j == targets[i]]) w[j][k],  p_ij = exp(logit_ij - lse[i]),  0 on rows with an ignored
// target.  The lm_head is frozen in QEFT: there is no d(weight).  Rows are taken in chunks of LG_R; per chunk two launches:
//
//   launch A  lm_head_nll_grad_g_kernel: the forward's logit tile (lm_head_nll_body.h: the same k loop, so the same fp32 logits bit
//             for bit), then g_ij = fp16(exp(logit - lse_i) - onehot), formed in fp32 and rounded once, into the workspace as
//             [chunk rows][vocab rounded up to 128]; 0 in the padding columns and in every column of an ignored row.  grad_nll is
//             NOT applied here: g stays in [-1, 1], clear of fp16's subnormals.
//   launch B  lm_head_nll_grad_dx_kernel: dx_chunk = g W as a 128 x 128 tile per block of 4 waves (2 x 2, 64 x 64 each), the sum
//             running over the vocabulary in tiles of 64.  W [vocab][hidden] is read where it lies: a W tile [64 j][128 k] reaches
//             LDS by 16-byte LDS-DMA as plain 256-byte rows under the XOR of lg_w_chunk and leaves it through
//             ds_read_b64_tr_b16, which hands a lane the 8 consecutive j of ONE k that the MFMA operand wants.  fp32 accumulators;
//             the epilogue multiplies row i by grad_nll[i] in fp32 and writes fp32, or rounds once to fp16.
//
// A wave's work is the same instruction sequence on the same values wherever its rows sit: a row of dx depends on that row of x,
// its lse, target and grad_nll and on the weight alone, bit for bit -- not on t, the row's index or chunk, either stride or the
// grid.  One block per output tile sums the whole vocabulary in ascending order: no split, no atomics, no arrival order.
// Rows >= the chunk's rows, vocabulary rows >= vocab and hidden columns >= hidden are loaded from the clamped row / column and
// never stored.  Every global offset comes from the ln_* / lg_* functions; lm_head_nll_grad_count_out_of_range walks them on the
// CPU.  The transposing read needs EXEC all ones and 8-byte aligned in-bounds addresses in every lane: the k loop has no
// lane-dependent branch, and the tiles are full (clamped loads), never masked.
#include "lm_head_nll_body.h"
#include "host_launch.h"

namespace qeft {

constexpr int LG_R = 1024;      // rows of a chunk: launch B is 8 x hidden / 128 blocks, one round of 256 CUs at hidden 4096
constexpr int LG_BM = 128;      // token rows of launch B's tile
constexpr int LG_BN = 128;      // hidden columns of launch B's tile
constexpr int LG_BK = 64;       // vocabulary rows of a staged tile
constexpr int LG_G_BYTES = LG_BM * LG_BK * 2, LG_W_BYTES = LG_BK * LG_BN * 2, LG_BUF_BYTES = LG_G_BYTES + LG_W_BYTES;

struct LgGeom {                 // one chunk
    int dx_stride, rows, hidden, vocab;
};

LN_HD int lg_vp(int vocab) { return (vocab + LN_BN - 1) / LN_BN * LN_BN; }            // width of a g row
LN_HD int lg_row_tiles(const LgGeom& G) { return (G.rows + LG_BM - 1) / LG_BM; }
LN_HD int lg_n_tiles(const LgGeom& G) { return (G.hidden + LG_BN - 1) / LG_BN; }
// launch B's blocks in the forward's XCD order: the row tiles that share a W column slab are adjacent and in one L2
LN_HD int lg_block_row_tile(const LgGeom& G, int block) {
    return ln_tile_order(lg_row_tiles(G) * lg_n_tiles(G), block) % lg_row_tiles(G);
}
LN_HD int lg_block_n_tile(const LgGeom& G, int block) {
    return ln_tile_order(lg_row_tiles(G) * lg_n_tiles(G), block) / lg_row_tiles(G);
}
// element offset of g[row][col] in the workspace (launch A's stores: 4 columns, 8 bytes)
LN_HD long long lg_g_off(const LgGeom& G, int row, int col) { return (long long)row * lg_vp(G.vocab) + col; }
// launch B's g tile is the forward's x tile: 128-byte rows, slot swizzle of ln_chunk; rows past the chunk read its last row
LN_HD long long lg_g_src_off(const LgGeom& G, int row_tile, int trow, int slot, int kt) {
    const int row = min(row_tile * LG_BM + trow, G.rows - 1);
    return lg_g_off(G, row, kt * LG_BK + ln_chunk(trow, slot) * 8);
}
// W tile: 256-byte rows [j][128 k]; LDS slot `slot` (16 bytes) of tile row jrow holds k-chunk slot ^ ((jrow & 3) << 2 | (jrow >> 2) & 3):
// the 4 rows x 2 blocks of 16 columns that a 32-lane half of the transposing read touches then cover the 64 banks exactly once
LN_HD int lg_w_chunk(int jrow, int slot) { return slot ^ (((jrow & 3) << 2) | ((jrow >> 2) & 3)); }
LN_HD long long lg_w_src_off(const LgGeom& G, int n_tile, int jrow, int slot, int kt) {
    const int j = min(kt * LG_BK + jrow, G.vocab - 1);
    const int ch = min(n_tile * (LG_BN / 8) + lg_w_chunk(jrow, slot), G.hidden / 8 - 1);
    return (long long)j * G.hidden + ch * 8;
}
LN_HD long long lg_dx_off(const LgGeom& G, int row, int col) { return (long long)row * G.dx_stride + col; }

int lm_head_nll_grad_chunk_rows() { return LG_R; }
size_t lm_head_nll_grad_workspace_bytes(int t, int vocab) { return (size_t)2 * min(t, LG_R) * lg_vp(vocab); }

// ---- launch A: g = fp16(exp(logit - lse) - onehot) of one chunk
__global__ __launch_bounds__(256) void lm_head_nll_grad_g_kernel(const f16* __restrict__ x, const f16* __restrict__ w,
                                                                 const int* __restrict__ targets, const float* __restrict__ lse,
                                                                 f16* __restrict__ g, LnGeom G) {
    constexpr int NW = 4;
    __shared__ __attribute__((aligned(16))) unsigned char lds[LnTile<NW>::LDS_BYTES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int row_tile = ln_block_row_tile(G, NW, blockIdx.x), col_tile = ln_block_col_tile(G, NW, blockIdx.x);

    f32x16 acc[4];
    ln_logit_tile<NW>(x, w, G, row_tile, col_tile, lds, acc);

    // register e of tile vt is the logit of column col0 + 32 vt + (e & 3) + 8 (e >> 2) + 4 h, token row: a register quad is 4
    // adjacent columns of one token, one 8-byte store
    const LgGeom GG{0, G.t, G.hidden, G.vocab};
    const int row = row_tile * LnTile<NW>::BM + wave * 32 + r;
    const int rc = min(row, G.t - 1);
    const int tg = targets[rc];
    const float l = lse[rc];
    const bool live = ln_target_ok(G, tg);
    const int col0 = col_tile * LN_BN;
#pragma unroll
    for (int vt = 0; vt < 4; ++vt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = col0 + vt * 32 + 8 * q + 4 * h;
            h4 out;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v = __expf(acc[vt][4 * q + i] - l) - (c + i == tg ? 1.f : 0.f);
                if (!live || c + i >= G.vocab) v = 0.f;
                asm volatile("" : "+v"(v));                    // the fp32 difference, then ONE rounding (no v_fma_mixlo_f16)
                out[i] = (f16)v;
            }
            if (row < G.t) *(h4*)(g + lg_g_off(GG, row, c)) = out;
        }
}

// ---- launch B: dx = grad_nll * (g W) of one chunk
__device__ __forceinline__ u32x2 lg_lds_read_tr(uint32_t addr) {
    u32x2 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(addr) : "memory");
    return v;
}

template <bool FP32>
__global__ __launch_bounds__(256) void lm_head_nll_grad_dx_kernel(const f16* __restrict__ g, const f16* __restrict__ w,
                                                                  const int* __restrict__ targets,
                                                                  const float* __restrict__ grad_nll, void* __restrict__ dx,
                                                                  LgGeom G) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * LG_BUF_BYTES];     // [2][g tile | W tile]
    const uint32_t lds0 = (uint32_t)(uintptr_t)lds;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int r = lane & 31, h = lane >> 5;
    const int row_tile = lg_block_row_tile(G, blockIdx.x), n_tile = lg_block_n_tile(G, blockIdx.x);
    const int ktiles = lg_vp(G.vocab) / LG_BK;

    // DMA pieces of 1 KB, 4 of each tile per wave.  g piece p = tile rows 8 p .. 8 p + 7, lane -> (row lane / 8, slot lane % 8),
    // its offset linear in kt; W piece p = tile rows 4 p .. 4 p + 3, lane -> (row lane / 16, slot lane % 16), its vocabulary row
    // clamped per k-tile
    const f16* gsrc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) gsrc[i] = g + lg_g_src_off(G, row_tile, (wave * 4 + i) * 8 + (lane >> 3), lane & 7, 0);
    auto stage = [&](int kt) {
        unsigned char* base = lds + (kt & 1) * LG_BUF_BYTES;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(gsrc[i] + (size_t)kt * LG_BK),
                                             (void __attribute__((address_space(3)))*)(base + (wave * 4 + i) * 1024), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_global_load_lds(
                (const void __attribute__((address_space(1)))*)(w + lg_w_src_off(G, n_tile, (wave * 4 + i) * 4 + (lane >> 4), lane & 15, kt)),
                (void __attribute__((address_space(3)))*)(base + LG_G_BYTES + (wave * 4 + i) * 1024), 16, 0, 0);
    };

    f32x16 acc[2][2];                                          // [hidden tile nt][token tile tt] of the wave's 64 x 64
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[nt][tt][e] = 0.f;

    // g fragment (token tile tt, k-step ks): tile row 64 wm + 32 tt + r, the 8 j of chunk 2 ks + h -- the forward's x fragment
    uint32_t goff[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) goff[ks] = (uint32_t)((wm * 64 + r) * 128 + (ln_chunk(r, 2 * ks + h) << 4));
    // W fragment (hidden tile nt, k-step ks): rows 16 ks + 8 h + {0..3} and + {4..7} of column 64 wn + 32 nt + r by two
    // transposing reads.  Lane 4 q + p of a 16-lane group addresses row q, columns 4 p .. 4 p + 3 of the group's 16: chunk
    // (p >> 1) of the group's two, its half p & 1.  A k-step is 16 rows = 4096 bytes further on, the XOR unchanged.
    uint32_t woff[2][2];
    {
        const int q = (lane & 15) >> 2, p = lane & 3;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int jrow = 8 * h + 4 * half + q;
                const int ch = wn * 8 + nt * 4 + ((lane >> 4) & 1) * 2 + (p >> 1);
                woff[nt][half] = (uint32_t)(LG_G_BYTES + jrow * 256 + (lg_w_chunk(jrow, ch) << 4) + (p & 1) * 8);
            }
    }
    auto read_g = [&](uint32_t tb, int ks, u32x4 (&fg)[2]) {
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) fg[tt] = ln_lds_read16(tb + goff[ks] + tt * 32 * 128);
    };
    auto read_w = [&](uint32_t tb, int ks, u32x2 (&fw)[2][2]) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int half = 0; half < 2; ++half) fw[nt][half] = lg_lds_read_tr(tb + woff[nt][half] + ks * 16 * 256);
    };

    stage(0);
    for (int kt = 0; kt < ktiles; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's pieces of tile kt landed
        __builtin_amdgcn_s_barrier();                          // ... and everyone's; everyone has read tile kt - 1
        if (kt + 1 < ktiles) stage(kt + 1);                    // into the buffer of tile kt - 1
        const uint32_t tb = lds0 + (uint32_t)(kt & 1) * LG_BUF_BYTES;
        u32x4 fg[2][2];
        u32x2 fw[2][2][2];
        read_g(tb, 0, fg[0]);
        read_w(tb, 0, fw[0]);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            ln_lds_wait();
            if (ks + 1 < 4) {                                  // the next k-step's fragments, in flight behind these MFMAs
                read_g(tb, ks + 1, fg[(ks + 1) & 1]);
                read_w(tb, ks + 1, fw[(ks + 1) & 1]);
            }
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const u32x2 lo = fw[ks & 1][nt][0], hi = fw[ks & 1][nt][1];
                const h8 a = __builtin_bit_cast(h8, u32x4{lo[0], lo[1], hi[0], hi[1]});
#pragma unroll
                for (int tt = 0; tt < 2; ++tt)
                    acc[nt][tt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, __builtin_bit_cast(h8, fg[ks & 1][tt]), acc[nt][tt], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: register e of acc[nt][tt] is hidden column n0 + 32 nt + (e & 3) + 8 (e >> 2) + 4 h of token row0 + 32 tt + r
    const int n0 = n_tile * LG_BN + wn * 64;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        const int row = row_tile * LG_BM + wm * 64 + tt * 32 + r;
        const int rc = min(row, G.rows - 1);
        const float s = grad_nll[rc];
        const int tg = targets[rc];
        const bool live = tg >= 0 && tg < G.vocab;             // an ignored row is +0.0 whatever grad_nll holds
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int col = n0 + nt * 32 + 8 * q + 4 * h;
                f32x4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float p = acc[nt][tt][4 * q + i] * s;      // rounded to fp32 before anything else: opaque, or hipcc folds the
                    asm volatile("" : "+v"(p));                // product into the fp16 conversion (v_fma_mixlo_f16, ONE rounding)
                    v[i] = live ? p : 0.f;
                }
                if (row < G.rows && col < G.hidden) {
                    if (FP32) {
                        *(f32x4*)((float*)dx + lg_dx_off(G, row, col)) = v;
                    } else {
                        h4 o;
#pragma unroll
                        for (int i = 0; i < 4; ++i) o[i] = (f16)v[i];
                        *(h4*)((f16*)dx + lg_dx_off(G, row, col)) = o;
                    }
                }
            }
    }
}

hipError_t lm_head_nll_grad_launch(const void* x, const void* w, const int* targets, const float* lse, const float* grad_nll, void* dx,
                                   void* ws, int x_stride, int dx_stride, int dx_fp32, int t, int hidden, int vocab, hipStream_t st) {
    g_last_variant = "lm_head_nll_grad";
    for (int c0 = 0; c0 < t; c0 += LG_R) {
        const int rows = min(LG_R, t - c0);
        const LnGeom GA{x_stride, rows, hidden, vocab};
        const LgGeom GB{dx_stride, rows, hidden, vocab};
        const f16* xc = (const f16*)x + (size_t)c0 * x_stride;
        hipLaunchKernelGGL(lm_head_nll_grad_g_kernel, dim3((unsigned)(ln_row_tiles(GA, 4) * ln_col_tiles(GA))), dim3(256), 0, st, xc,
                           (const f16*)w, targets + c0, lse + c0, (f16*)ws, GA);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        const dim3 grid((unsigned)(lg_row_tiles(GB) * lg_n_tiles(GB)));
        if (dx_fp32)
            hipLaunchKernelGGL(lm_head_nll_grad_dx_kernel<true>, grid, dim3(256), 0, st, (const f16*)ws, (const f16*)w, targets + c0,
                               grad_nll + c0, (void*)((float*)dx + (size_t)c0 * dx_stride), GB);
        else
            hipLaunchKernelGGL(lm_head_nll_grad_dx_kernel<false>, grid, dim3(256), 0, st, (const f16*)ws, (const f16*)w, targets + c0,
                               grad_nll + c0, (void*)((f16*)dx + (size_t)c0 * dx_stride), GB);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// Every global address the launches of all chunks form, on the CPU, in ELEMENTS of the operand's type (dx offsets are the same for
// fp16 and fp32): the largest number of elements by which one passes the end of its operand (x: t rows at x_stride, the last
// `hidden` wide; w: [vocab][hidden]; g: the workspace as fp16; dx: t rows at dx_stride, the last `hidden` wide; targets, lse and
// grad_nll: t words), or runs in front of it; 0 when none does.  Weight addresses depend on neither the chunk nor the row tile,
// x and g addresses not on the column tile: each is visited once.
long long lm_head_nll_grad_count_out_of_range(int x_stride, int dx_stride, int t, int hidden, int vocab) {
    const long long x_n = (long long)(t - 1) * x_stride + hidden, dx_n = (long long)(t - 1) * dx_stride + hidden;
    const long long w_n = (long long)vocab * hidden, g_n = (long long)lm_head_nll_grad_workspace_bytes(t, vocab) / 2;
    long long worst = 0;
    auto touch = [&](long long b, int n, long long operand_n) {
        if (b < 0 && -b > worst) worst = -b;
        if (b + n - operand_n > worst) worst = b + n - operand_n;
    };
    {   // the weight: launch A's tiles (the forward's), launch B's tiles
        const LnGeom GA{x_stride, min(t, LG_R), hidden, vocab};
        const LgGeom GB{dx_stride, min(t, LG_R), hidden, vocab};
        for (int ct = 0; ct < ln_col_tiles(GA); ++ct)
            for (int trow = 0; trow < LN_BN; ++trow)
                for (int slot = 0; slot < 8; ++slot)
                    for (int kt = 0; kt < hidden / LN_BK; ++kt) touch(ln_w_off(GA, ct, trow, slot, kt), 8, w_n);
        for (int nt = 0; nt < lg_n_tiles(GB); ++nt)
            for (int kt = 0; kt < lg_vp(vocab) / LG_BK; ++kt)
                for (int jrow = 0; jrow < LG_BK; ++jrow)
                    for (int slot = 0; slot < 16; ++slot) touch(lg_w_src_off(GB, nt, jrow, slot, kt), 8, w_n);
    }
    for (int c0 = 0; c0 < t; c0 += LG_R) {
        const int rows = min(LG_R, t - c0);
        const LnGeom GA{x_stride, rows, hidden, vocab};
        const LgGeom GB{dx_stride, rows, hidden, vocab};
        const long long xb = (long long)c0 * x_stride, dxb = (long long)c0 * dx_stride;
        for (int rt = 0; rt < ln_row_tiles(GA, 4); ++rt)
            for (int trow = 0; trow < 128; ++trow) {
                for (int slot = 0; slot < 8; ++slot)
                    for (int kt = 0; kt < hidden / LN_BK; ++kt) touch(xb + ln_x_off(GA, rt, 4, trow, slot, kt), 8, x_n);
                const int row = rt * 128 + trow;
                touch(c0 + min(row, rows - 1), 1, t);                                  // targets, lse
                if (row >= rows) continue;
                for (int c = 0; c < lg_vp(vocab); c += 4) touch(lg_g_off(GB, row, c), 4, g_n);
            }
        for (int block = 0; block < lg_row_tiles(GB) * lg_n_tiles(GB); ++block) {
            const int rt = lg_block_row_tile(GB, block), nt = lg_block_n_tile(GB, block);
            if (nt == 0)
                for (int trow = 0; trow < LG_BM; ++trow)
                    for (int slot = 0; slot < 8; ++slot)
                        for (int kt = 0; kt < lg_vp(vocab) / LG_BK; ++kt) touch(lg_g_src_off(GB, rt, trow, slot, kt), 8, g_n);
            for (int trow = 0; trow < LG_BM; ++trow) {
                const int row = rt * LG_BM + trow;
                touch(c0 + min(row, rows - 1), 1, t);                                  // targets, grad_nll
                if (row >= rows) continue;
                for (int c = nt * LG_BN; c < (nt + 1) * LG_BN; c += 4)
                    if (c < hidden) touch(dxb + lg_dx_off(GB, row, c), 4, dx_n);
            }
        }
    }
    return worst;
}

}  // namespace qeft
