// Geometry, state record and index arithmetic of the training update (oweight_optim.hip): global-norm
// clipping and loss-scaled AdamW over ONE flat fp32 arena that holds every oweight of the model (qeft_amd/optim.py).  Shared by
// the two kernels and by the host-side address enumeration behind qeft_oweight_optim_check_extents: every global address a
// launch forms comes out of oo_chunk / oo_off below.
//
//   p, g, m, v   fp32 [n], n % 64 == 0 (every tensor of the arena starts at a multiple of 64 elements, gaps hold zero)
//   partials     fp32 [oo_blocks(G)]: launch 1 writes one sum of squares per block, launch 2 reads them all
//   state        two OoState records; a step reads one and writes the other
//
// The element -> (block, thread, iteration, slot) map depends on n (and the compile-time OO_U) alone, never on the device.
#pragma once
#include <hip/hip_runtime.h>

namespace qeft {

constexpr int OO_THREADS = 256;
constexpr int OO_MAX_BLOCKS = 2048;
constexpr int OO_U = 2;                                     // 16-byte chunks per thread per iteration (measured: DESIGN.md 4.19)
constexpr long long OO_MAX_N = (1ll << 31) - (1ll << 20);

// The optimiser's state on the device: 32 bytes, 16-byte aligned.  Field order is the ABI (optim.py reads it back as 8 words).
struct OoState {
    float scale;        // the loss scale the gradients in g carry
    int step;           // applied updates so far (skipped steps do not count); the bias corrections use step + 1
    int good_steps;     // applied updates since the scale last changed
    int skipped_last;   // 1 when the last step found a non-finite gradient and changed nothing
    int n_skipped;      // skipped steps so far
    float grad_norm;    // global norm of the unscaled gradient at the last applied step
    float clip_coef;    // min(1, max_norm / (grad_norm + 1e-6)) at the last applied step (1 with clipping off)
    int reserved;
};
static_assert(sizeof(OoState) == 32, "the record is 32 bytes");

struct OoGeom {
    long long n;
    int u;              // chunks per thread per iteration: OO_U, or the lab override (1, 2, 4)
};

__host__ __device__ inline long long oo_chunks(const OoGeom& G) { return G.n / 4; }
__host__ __device__ inline int oo_blocks(const OoGeom& G) {
    const long long per = (long long)OO_THREADS * G.u, b = (oo_chunks(G) + per - 1) / per;
    return (int)(b < OO_MAX_BLOCKS ? b : OO_MAX_BLOCKS);
}
// iterations of the grid-stride loop: the same for every block (a block past the ragged tail finds no chunk in range there)
__host__ __device__ inline int oo_iters(const OoGeom& G) {
    const long long per = (long long)oo_blocks(G) * OO_THREADS * G.u;
    return (int)((oo_chunks(G) + per - 1) / per);
}
// chunk of (block, tid) in iteration `it`, slot `s` < u: a wave's 64 lanes take 64 consecutive chunks (1 KiB)
__host__ __device__ inline long long oo_chunk(const OoGeom& G, int block, int tid, int it, int s) {
    return (((long long)it * oo_blocks(G) + block) * G.u + s) * OO_THREADS + tid;
}
__host__ __device__ inline long long oo_off(long long chunk) { return chunk * 4; }
// the most elements one thread accumulates into its sum of squares (the k of the norm's error bound)
__host__ __device__ inline long long oo_thread_elems(const OoGeom& G) { return (long long)oo_iters(G) * G.u * 4; }

// The update's arithmetic is pinned (fp32, one rounding per operation, nothing contracted into an FMA).  With the record's
// scale s, inv = 1 / s, and per step (every block computes the same bits):
//   sum   = partials[0] + partials[1] + ... in double, in index order;   norm = float(sqrt(sum))
//   coef  = max_norm > 0 ? min(1, max_norm / (norm + 1e-6f)) : 1
//   t = step + 1;  bc1 = 1 - beta1^t, bc2 = 1 - beta2^t in double;  a = float(lr / bc1),  r = float(sqrt(bc2))
//   decay = 1 - lr * wd,  c1 = 1 - beta1,  c2 = 1 - beta2
// and per element:
//   x  = g * inv                      (launch 1 accumulates acc = acc + x * x, the product rounded on its own)
//   gh = x * coef
//   p1 = p * decay
//   m' = m + (gh - m) * c1
//   v' = beta2 * v + c2 * (gh * gh)
//   p' = p1 - a * (m' / (sqrt(v') / r + eps))
// Division and square root are the correctly rounded ones.

struct OoHyper {
    float lr, beta1, beta2, eps, weight_decay, max_norm, growth_factor, backoff_factor;
    int growth_interval, dynamic;
};

// ---- host side: oweight_optim.hip
hipError_t oweight_grad_stats_launch(const void* g, const OoGeom& G, const void* state_in, void* partials, hipStream_t st);
hipError_t oweight_adamw_launch(void* p, const void* g, void* m, void* v, const OoGeom& G, const void* state_in, void* state_out,
                                const void* partials, const OoHyper& H, bool nontemporal_g, hipStream_t st);
long long oweight_optim_count_out_of_range(const OoGeom& G);

}  // namespace qeft
