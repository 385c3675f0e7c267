// Single-token attention of the decode harness (rotary + KV append + flash-decoding split): the kernel of decode_aux.hip, with its
// BODY as a device function (the round-4 lab kernel tools/attn_oproj_lab_kernel.h -- attention and o_proj in one launch, measured
// and rejected: profiles/r04_attn_oproj_fused.txt -- runs the same body).
#pragma once
#include "qeft_common.h"

namespace qeft {

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// maximum over the 64 lanes of a wave, every lane gets it: 4 DPP steps inside each row of 16, then two cross-row swaps
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp_mov<0xB1>(v));    // quad_perm [1,0,3,2]
    v = fmaxf(v, dpp_mov<0x4E>(v));    // quad_perm [2,3,0,1]
    v = fmaxf(v, dpp_mov<0x141>(v));   // row_half_mirror
    v = fmaxf(v, dpp_mov<0x140>(v));   // row_mirror
    v = fmaxf(v, __shfl_xor(v, 16));
    v = fmaxf(v, __shfl_xor(v, 32));
    return v;
}

__device__ __forceinline__ void st_agent(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float ld_agent(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

constexpr int kAttnRec = 132;   // floats per (head, split) record of the workspace: acc[128], max, sum, pad
// The arrival counters sit IN FRONT of the records, at an offset that does not depend on S: one workspace sized for the largest
// split then serves every smaller one in any order (the decode engine goes 8 -> 4 -> 1 when a long sequence is followed by a new
// one).  Behind the records they landed, for a smaller S, inside the records a larger S had left: a ticket read from there never
// equals S - 1 and no block merges the head.
__host__ __device__ constexpr size_t attn_ctr_floats(int n_heads) { return ((size_t)n_heads + 3) / 4 * 4; }

// Single-token attention for one sequence.  grid = n_heads * S, block = 256 (4 waves), head_dim = 128.
//   q,k,v  : this token's projections [n_heads*128], [n_kv*128], [n_kv*128] (fp16)
//   cos/sin: fp32 rotary values; ROW != 0: [64], the row of THIS position, selected by the caller (the engine's form);
//            ROW == 0: the whole table [>= max_seq][64], row *pos_ptr is used.  The launcher picks the instantiation (tab_rows == 1)
//   kc, vc : caches [n_kv][max_seq][128] fp16;  *pos_ptr = index of this token (0-based)
//   out    : [n_heads*128] fp16, element i stored at out_pos[i] when out_pos is given
//   ws     : S > 1 only: [attn_ctr_floats(n_heads)] uint32 arrival counters (zero before first use), then [n_heads*S][kAttnRec] floats
// 32 blocks pulling a whole head's K and V each are bound by what ONE CU can load (~100 KB took ~4 us), so a head is
// split over S blocks and the kernel is organised around latency:
//   * requests go out in the order in which their consumers run, because a wave's vector loads retire in order through one
//     counter: q/k/v and the rotary values first (ROW != 0: before `pos` is back), the output map, then the K quarter-rows and
//     V pieces of the first PRE runs of each wave.  The first EARLY of those runs do not wait for `pos` either (ROW != 0): their
//     addresses come from the preloaded arguments alone -- the run's rows if it lies inside the cache, else run 0 -- and `pos`,
//     a scalar round trip behind the kernel arguments, arrives while they go out; what they fetch at or beyond `pos` is masked
//     by the selects that already mask the tail of the last run.  Runs EARLY .. PRE - 1 (and all of them in the whole-table
//     form, whose rotary row needs `pos` first) fetch rows inside the context only; a run past it re-reads row 0, so the count
//     is fixed.  The rotary waits for what is older than that prefetch (vmcnt(PRE * (4 + 4 / DH))), run i's scores
//     for the K loads up to run i's, P.V for the V loads; rotary, scores and P.V of the prefetched runs are straight-line
//     code (values and addresses selected, nothing branched on), so that no wait covers a load its consumer does not read;
//   * positions are dealt in runs of 16 to the 4*S waves of a head (run r belongs to wave r % (4*S)); each wave
//     computes its scores, its own maximum, exp and P.V partials with wave-level operations only (flash-decoding
//     split), the block merges its 4 waves once through LDS;
//   * S > 1: every block publishes its (acc, max, sum) record with write-through stores and takes a ticket from the
//     head's counter; the block that draws the last ticket merges the S records in split order (deterministic) and
//     re-arms the counter.  Nobody waits for anybody (MI355X_MICROARCH.md, inter-workgroup visibility, table row 1).
// DH = 2 (one block per head only): the head's 128 output dims are dealt over DH blocks.  Both compute the scores (K is
// fetched twice), each fetches half of every V row and does half of P.V; their outputs are disjoint, so there is nothing
// to merge.  Per block 3/4 of the bytes (the bound at these sizes is what ONE CU can pull) and half of the P.V math.
// KFT: the key cache has the reference's FasterTransformer layout [n_kv][128/8][max_seq][8] (ft_attention.cpp:131-133,
// ftllama_modeling.py:62-65) instead of [n_kv][max_seq][128]; only the address of a 16-byte (position, 8-dim chunk)
// piece changes -- consecutive positions of one chunk are then contiguous.
template <bool KFT>
__device__ __forceinline__ size_t kcache_off(int p, int chunk, int max_seq) {
    return KFT ? ((size_t)chunk * max_seq + p) * 8 : (size_t)p * 128 + chunk * 8;
}

// Parameter order: what the loads in front of `pos` need comes first -- the leading 14 dwords of the kernel-argument segment
// (all that 16 user SGPRs leave behind the segment's own address) are preloaded into SGPRs at wave launch (build flag
// -amdgpu-kernarg-preload-count): q, k, v, cs, out_pos, kc, the geometry word and n_heads.  The geometry word (rope_attn_geom,
// below) carries heads per kv head, its shift when a power of two, log2 S and max_seq / 16: the cache stride of a head and the
// clamp of the early runs need no scalar load, and no division stands ahead of the first load.  vc is the first argument behind
// them: its scalar load returns while the K requests go out.  ROW: 0 = cs / sn are whole tables; 1 = this position's rows;
// 2 = this position's rows with sn == cs + 64 (the engine's buffer), which takes both from the preloaded cs.
// DBG (lab only, tools/attn_timeline.py): per-wave phase stamps.
// The kernel's BODY is a device function so that the lab's fused attention + o_proj launch can run it too:
// `bid` = the block's index among the attention blocks, `smem_raw` = its dynamic LDS, and -- S == 1 only -- `pub` != NULL sends
// every output element to pub[opos] by an agent-scope (write-through) store instead of a plain store to out[opos]: readers on
// other XCDs of the SAME launch can then be released by a flag (lab only; the product passes NULL).
template <int PRE, int DH = 1, bool KFT = false, bool DBG = false, bool ALIBI = false, int ROW = 1, int EARLY_ = 0>
__device__ __forceinline__ void rope_attn_decode_body(uint8_t* smem_raw, const int bid, const f16* __restrict__ q,
                                                      const f16* __restrict__ k, const f16* __restrict__ v,
                                                      const float* __restrict__ cs, const int* __restrict__ out_pos,
                                                      f16* __restrict__ kc, uint32_t geom, int n_heads, f16* __restrict__ vc,
                                                      const float* __restrict__ sn, const int* __restrict__ pos_ptr,
                                                      f16* __restrict__ out, float* __restrict__ ws,
                                                      unsigned long long* dbg_ptr, const float* __restrict__ alibi,
                                                      f16* __restrict__ pub = nullptr) {
    constexpr int HD = 128;
    // prefetched runs requested before `pos` is known; none in the whole-table form, whose rotary row needs `pos` and is requested first
    constexpr int EARLY = ROW == 0 ? 0 : EARLY_ < PRE ? EARLY_ : PRE;
    const int grp = (int)(geom & 0xfffu), gsh = (int)((geom >> 12) & 0xfu);
    const int lgS = DH > 1 ? 0 : (int)((geom >> 16) & 3u), S = 1 << lgS;      // DH > 1 is launched with one split only
    const int max_seq = (int)((geom >> 18) & 0xfffu) * 16;
    unsigned long long* const dbg = DBG ? dbg_ptr : nullptr;
    unsigned long long stamp[10];
    auto mark = [&](int i) {
        if (dbg) { __builtin_amdgcn_sched_barrier(0); stamp[i] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); }
    };
    unsigned long long rt0 = dbg ? __builtin_amdgcn_s_memrealtime() : 0;
    mark(0);
    float* prob = (float*)smem_raw;          // [max_seq + 16] raw scores
    float* part = prob + max_seq + 16;       // [16*DH][128/DH] P.V partials: (wave, position class) x dims of this block
    float* psum = part + 16 * HD;            // [16*DH] exp sums
    float* wm = psum + 64;                   // [4] wave maxima
    f16* knew = (f16*)(wm + 4);              // [128]
    f16* vnew = knew + HD;                   // [128]
    f16* qs = vnew + HD;                     // [128] rotated, pre-scaled q (fp16 like the reference's rotated q)
    __shared__ int last_ticket;

    constexpr int HDB = HD / DH;             // output dims of this block
    constexpr int NDG = 16 / DH;             // 8-dim groups of this block
    constexpr int NPC = 64 / NDG;            // position classes of a 16-position run
    constexpr int PPC = 16 / NPC;            // positions per class
    // No division stands in front of the first load: DH is a power of two, S = 1 << lgS, and the launcher sends the shift of a
    // power-of-two group size (gsh - 1; gsh = 0: any other size, divided here).
    const int dhi = (int)((unsigned)bid % DH);
    const int hs_idx = (int)((unsigned)bid / DH);
    const int h = hs_idx >> lgS, sp = hs_idx & (S - 1), t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int gw = sp * 4 + w, NW = 4 * S;   // this wave among the head's waves
    const int hk = gsh ? h >> (gsh - 1) : h / grp;
    f16* kch = kc + (size_t)hk * max_seq * HD;
    const bool appender = (sp == 0) && (dhi == 0) && (h == hk * grp);
    // ALIBI (the reference's single_query_attention boundary only): the head's linear position bias, slope * (key - query position)
    // added to the scaled score (decoder_masked_multihead_attention_template.hpp:1335-1345, no padding tokens)
    const float slope = ALIBI ? alibi[h] : 0.f;

    // ---- loads that do not depend on pos.  The per-thread ones are unconditional (addresses selected, never branched
    // on) and nothing is converted here: a conversion or a divergent branch makes the compiler wait for the load on the
    // spot, which serialises one memory round trip per load group at the top of the kernel.
    const int ti = dhi * HDB + (t & (HDB - 1));                        // output element of this thread (within the head)
    const f16* src = (t < 64) ? q + h * HD + t : (t < 128) ? k + hk * HD + (t - 64) : v + hk * HD + (t - 128);
    const f16 raw_a = src[0];
    const f16 raw_b = src[(t < 128) ? 64 : 0];
    // The rotary values are requested by every thread, without a branch and AHEAD of the K/V prefetch in both forms: the
    // counter of outstanding vector loads retires in order, so the rotary's wait for them then leaves the whole prefetch
    // in flight.  (Loaded behind the prefetch in one form only, they made the compiler drain it -- vmcnt(0) -- in both.)
    float rc, rsn;
    if constexpr (ROW != 0) {                 // the caller already selected this position's rotary row: no wait for pos
        rc = cs[t & 63];
        rsn = ROW == 2 ? cs[64 + (t & 63)] : sn[t & 63];     // 2: the sine row stands behind the cosine row (the engine's buffer)
    }
    // The output map is the one load taken under a (kernel-uniform, scalar) branch, and it stands HERE on purpose: loads
    // whose values are used only behind the `pos` check below are otherwise sunk behind that check -- issued one scalar
    // round trip late -- and a load is not sunk past a join of two paths.
    int opos_raw = 0;
    if (out_pos) opos_raw = out_pos[h * HD + ti];
    // ---- K/V of the first PRE runs of this wave: PRE * (4 + 4 / DH) loads whatever the context, so that the compiler's vmcnt
    // bookkeeping is exact: the rotary waits for q/k/v and the table values only, run i's scores for the K loads up to run i's,
    // and P.V for the V loads -- all of it straight-line code, so no wait covers a load its consumer does not read.
    // score role: position pj of the run, dims qd*8 + 32*j .. +8 (j = 0..3): the 4 lanes of a position read 64
    // contiguous bytes per load instruction
    const int qd = lane & 3, pj = lane >> 2;
    // P.V role: dims dhi*HDB + dg*8 .., positions pc*PPC .. of the run
    const int dg = lane & (NDG - 1), pc = lane / NDG;
    const int dim0 = dhi * HDB + dg * 8;
    h8 kpre[PRE][4], vpre[PRE][PPC];
    // Run i of this wave starts at row r0 = (i * NW + gw) * 16 (max_seq % 16 == 0: a run never straddles the cache end).  The
    // first EARLY runs are requested WITHOUT `pos`: rows r0 .. r0 + 15 if the run lies inside the cache (r0 < max_seq), else run
    // 0 -- every such row is inside the allocation whatever `pos` is, and what lies at or beyond `pos` is masked by the selects
    // of score_run / pv_run below (the tests poison those rows).  Runs EARLY .. PRE - 1 wait for `pos` and fetch rows inside the
    // context only (a run past it re-reads row 0, an L1 hit).
    auto k_run = [&](int i, int krow) {
#pragma unroll
        for (int j = 0; j < 4; ++j) kpre[i][j] = *(const h8*)(kch + kcache_off<KFT>(krow, qd + 4 * j, max_seq));
    };
    f16* vch;
    auto v_run = [&](int i, int vrow) {
        const h8* row = (const h8*)(vch + (size_t)vrow * HD + dim0);
#pragma unroll
        for (int j = 0; j < PPC; ++j) vpre[i][j] = row[j * (HD / 8)];
    };
    auto early_r0 = [&](int i) {
        const int r0 = (i * NW + gw) * 16;
        return r0 < max_seq ? r0 : 0;
    };
#pragma unroll
    for (int i = 0; i < EARLY; ++i) k_run(i, early_r0(i) + pj);
    // vc is the first kernel argument behind the preloaded ones.  Its first use is pinned HERE: behind the early K requests, and
    // in front of the `pos` check -- left to the compiler, its scalar load is either awaited in front of those requests or sunk
    // behind the check, where it is one more round trip in series with pos_ptr and `pos` ahead of the rest of the prefetch.
    if constexpr (EARLY > 0) __builtin_amdgcn_sched_barrier(0);
    vch = vc + (size_t)hk * max_seq * HD;
    if constexpr (EARLY > 0) asm volatile("" ::"s"(vch));
    if constexpr (EARLY == PRE) {             // the whole prefetch is out before `pos` is looked at
#pragma unroll
        for (int i = 0; i < EARLY; ++i) v_run(i, early_r0(i) + pc * PPC);
    }
    // `pos` is a scalar load: it arrives while the vector loads above are in flight, and nothing above waits for it.  With an
    // early prefetch it is taken under a kernel-uniform branch for the reason given at the output map: the prefetch's values are
    // used behind the `pos` check only, and without a join between the two the compiler sinks all its loads behind that check.
    mark(1);
    int pos_raw = -1;
    if (EARLY == 0 || pos_ptr) pos_raw = *pos_ptr;
    const int pos = pos_raw, L = pos + 1;
    if (pos < 0 || pos >= max_seq) return;   // never index the cache / rotary table out of range (grid-uniform)
    if (dbg) { asm volatile("" :: "s"(pos)); }
    if constexpr (ROW == 0) {                 // the whole table: row pos, requested ahead of the prefetch (EARLY is 0 in this form)
        rc = cs[(size_t)pos * 64 + (t & 63)];
        rsn = sn[(size_t)pos * 64 + (t & 63)];
    }
    mark(2);
#pragma unroll
    for (int i = EARLY; i < PRE; ++i) {
        const int r0 = (i * NW + gw) * 16;
        k_run(i, r0 < L ? r0 + pj : 0);
    }
    if constexpr (EARLY < PRE) {
#pragma unroll
        for (int i = 0; i < EARLY; ++i) v_run(i, early_r0(i) + pc * PPC);
    }
#pragma unroll
    for (int i = EARLY; i < PRE; ++i) {
        const int r0 = (i * NW + gw) * 16;
        v_run(i, r0 < L ? r0 + pc * PPC : 0);
    }
    const int opos = out_pos ? opos_raw : h * HD + ti;
    // ---- rotary and staging, one straight line for the four waves: every thread rotates (the v threads' result is not used)
    // and writes two LDS halves whose VALUE and ADDRESS are selected by its role.  A value used under a role branch only
    // is sunk into that branch by the compiler, load and all -- behind the prefetch, where waiting for it drains the prefetch.
    const float ra = (float)raw_a, rb = (float)raw_b;
    const int i = t & 63;
    const float c = rc, sv = rsn;
    float r0 = ra * c - rb * sv, r1 = rb * c + ra * sv;
    // the rotated pair exists in fp32 once, for q and k alike: k is the fp16 rounding OF that fp32 value (without this the
    // compiler folds the rounding into a second, fused evaluation for k, which rounds once and differs in the last bit)
    asm("" : "+v"(r0), "+v"(r1));
    const float scale = 0.08838834764831845f;  // 1/sqrt(128)
    const f16 q0 = (f16)(r0 * scale), q1 = (f16)(r1 * scale);
    const f16 k0 = (f16)r0, k1 = (f16)r1;
    const f16 vv = (f16)ra;
    {
        // qs + i | knew + i | vnew + (t - 128), as one offset into knew | vnew | qs (contiguous, above): plain integer selects
        f16* const d0 = knew + t + ((t < 64) ? 2 * HD : (t < 128) ? -64 : 0);
        d0[0] = (t < 64) ? q0 : (t < 128) ? k0 : vv;
        d0[(t < 128) ? 64 : 0] = (t < 64) ? q1 : (t < 128) ? k1 : vv;      // the v threads write their one element twice
    }
    if (appender) {                           // block-uniform; stores only, of values the LDS writes above already needed
        if (t >= 128) {
            vch[(size_t)pos * HD + (t - 128)] = vv;
        } else if (t >= 64) {
            kch[kcache_off<KFT>(pos, i >> 3, max_seq) + (i & 7)] = k0;
            kch[kcache_off<KFT>(pos, (i >> 3) + 8, max_seq) + (i & 7)] = k1;
        }
    }
    // workgroup barrier for LDS only: __syncthreads() would also drain the K/V prefetch that is still in flight (the append
    // stores above count in vmcnt as well; they are the youngest entries and nothing below waits for them)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    mark(3);

    // ---- scores of this wave's runs: raw score -> prob[], running maximum
    h2 qreg[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) qreg[j] = *(const h2*)(qs + (j >> 2) * 32 + qd * 8 + 2 * (j & 3));
    // The new token's own score comes from LDS (its cache row may not have landed, and the tests poison it): every lane
    // runs that chain once per wave, and the lanes of position `pos` take it by a select.  Nothing in a run is branched on,
    // so the PRE prefetched runs are one basic block with one vmcnt wait per K load (this hipcc keeps the runs' dot2 chains in
    // program order and interleaves only the own-score chain with run 0's); a run past the context (the wave-uniform !live)
    // computes on row 0 and sends its masked scores to the 16 spare floats behind prob[max_seq].
    float snew = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) snew = dot2(qreg[j], *(const h2*)(knew + (j >> 2) * 32 + qd * 8 + 2 * (j & 3)), snew);
    float lmax = -3.0e38f;
    auto score_run = [&](int i, const h8* kr, bool live) {
        const int p = (i * NW + gw) * 16 + pj;
        float sdot = 0.f;
        // v_dot2_f32_f16: two products per instruction, fp32 accumulation, no conversions
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const u32x4 kw = __builtin_bit_cast(u32x4, kr[j]);
#pragma unroll
            for (int e = 0; e < 4; ++e) sdot = dot2(qreg[j * 4 + e], as_h2(kw[e]), sdot);
        }
        sdot = (p == pos) ? snew : sdot;
        sdot += dpp_mov<0xB1>(sdot);
        sdot += dpp_mov<0x4E>(sdot);
        if constexpr (ALIBI) sdot += slope * (float)(p - pos);
        sdot = (p >= L) ? -3.0e38f : sdot;   // fetched but outside the context (possibly uninitialised cache rows)
        if (qd == 0) prob[live ? p : max_seq + pj] = sdot;
        lmax = fmaxf(lmax, sdot);
    };
#pragma unroll
    for (int i = 0; i < PRE; ++i) score_run(i, kpre[i], (i * NW + gw) * 16 < L);
    for (int i = PRE; (i * NW + gw) * 16 < L; ++i) {
        h8 kr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) kr[j] = *(const h8*)(kch + kcache_off<KFT>((i * NW + gw) * 16 + pj, qd + 4 * j, max_seq));
        score_run(i, kr, true);
    }
    const float mw = wave_max(lmax);
    mark(4);
    __builtin_amdgcn_wave_barrier();         // prob[] of this wave's runs is written and read by this wave only

    // ---- P.V partials of this wave's runs
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.f;
    float lsum = 0.f;
    // Selects again, no branches: a position outside the context gets the weight 0 by a select (never 0 x cache, which may
    // hold NaN there) and, like the token's own position, the token's v from LDS as its finite operand; adding 0 x that
    // leaves every sum as it was, bit for bit.
    const h8 vn = *(const h8*)(vnew + dim0);
    auto pv_run = [&](int i, const h8* vr, bool live) {
        const int p0 = (i * NW + gw) * 16 + pc * PPC;
        const int s0 = live ? p0 : max_seq + pc * PPC;
        float sraw[PPC];
#pragma unroll
        for (int j = 0; j < PPC; ++j) sraw[j] = prob[s0 + j];
#pragma unroll
        for (int j = 0; j < PPC; ++j) {
            const int p = p0 + j;
            const float ex = __expf(sraw[j] - mw);
            const float e = (p < L) ? ex : 0.f;
            const h8 vv = (p < pos) ? vr[j] : vn;
            lsum += e;
#pragma unroll
            for (int d = 0; d < 8; ++d) o[d] += e * (float)vv[d];
        }
    };
#pragma unroll
    for (int i = 0; i < PRE; ++i) pv_run(i, vpre[i], (i * NW + gw) * 16 < L);
    for (int i = PRE; (i * NW + gw) * 16 < L; ++i) {
        h8 vr[PPC];
#pragma unroll
        for (int j = 0; j < PPC; ++j)
            vr[j] = *(const h8*)(vch + (size_t)((i * NW + gw) * 16 + pc * PPC + j) * HD + dim0);
        pv_run(i, vr, true);
    }
    {
        float* dst = part + (w * NPC + pc) * HDB + dg * 8;
        *(f32x4*)dst = f32x4{o[0], o[1], o[2], o[3]};
        *(f32x4*)(dst + 4) = f32x4{o[4], o[5], o[6], o[7]};
        if (dg == 0) psum[w * NPC + pc] = lsum;
        if (lane == 0) wm[w] = mw;
    }
    mark(5);
    __syncthreads();
    mark(6);
    // ---- merge the block's 4 waves (a wave without positions has max -3e38: factor 0)
    const float M = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
    float acc = 0.f, den = 0.f;
    if (t < HDB) {
#pragma unroll
        for (int g = 0; g < 4 * NPC; ++g) {
            const float f = __expf(wm[g / NPC] - M);
            acc += f * part[g * HDB + t];
            den += f * psum[g];
        }
    }
    if (S == 1) {
        if (t < HDB) {
            const f16 ov = (f16)(acc / den);
            if (pub) __hip_atomic_store((uint16_t*)pub + opos, __builtin_bit_cast(uint16_t, ov), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else out[opos] = ov;
        }
        if (dbg && lane == 0) {
            mark(7);
            unsigned long long* d = dbg + ((size_t)bid * 4 + w) * 12;
            d[0] = rt0; d[1] = __builtin_amdgcn_s_memrealtime();
            for (int i = 0; i < 8; ++i) d[2 + i] = stamp[i];
            d[10] = d[11] = 0;
        }
        return;
    }
    // ---- publish this split's record, take a ticket; the last arriver merges the head
    float* rec = ws + attn_ctr_floats(n_heads) + (size_t)(h * S + sp) * kAttnRec;
    if (t < HD) st_agent(rec + t, acc);
    if (t == 0) {
        st_agent(rec + HD, M);
        st_agent(rec + HD + 1, den);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    mark(7);
    unsigned* ctr = (unsigned*)ws + h;
    if (t == 0) {
        const unsigned ticket = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_ticket = (ticket == (unsigned)(S - 1));
        if (ticket == (unsigned)(S - 1)) __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    mark(8);
    if (dbg && lane == 0 && !last_ticket) {
        unsigned long long* d = dbg + ((size_t)bid * 4 + w) * 12;
        d[0] = rt0; d[1] = __builtin_amdgcn_s_memrealtime();
        for (int i = 0; i < 9; ++i) d[2 + i] = stamp[i];
        d[11] = 0;
    }
    if (!last_ticket) return;
    if (t < HD) {
        const float* r0 = ws + attn_ctr_floats(n_heads) + (size_t)h * S * kAttnRec;
        float Mh = -3.0e38f;
        for (int j = 0; j < S; ++j) Mh = fmaxf(Mh, ld_agent(r0 + j * kAttnRec + HD));
        float a2 = 0.f, d2 = 0.f;
        for (int j = 0; j < S; ++j) {
            const float f = __expf(ld_agent(r0 + j * kAttnRec + HD) - Mh);   // a split without positions: factor 0
            a2 += f * ld_agent(r0 + j * kAttnRec + t);
            d2 += f * ld_agent(r0 + j * kAttnRec + HD + 1);
        }
        out[opos] = (f16)(a2 / d2);
    }
    if (dbg && lane == 0) {
        mark(9);
        unsigned long long* d = dbg + ((size_t)bid * 4 + w) * 12;
        d[0] = rt0; d[1] = __builtin_amdgcn_s_memrealtime();
        for (int i = 0; i < 9; ++i) d[2 + i] = stamp[i];
        d[11] = stamp[9];
    }
}

template <int PRE, int DH = 1, bool KFT = false, bool DBG = false, bool ALIBI = false, int ROW = 1, int EARLY = 0>
__global__ __launch_bounds__(256) void rope_attn_decode_kernel(const f16* __restrict__ q, const f16* __restrict__ k,
                                                               const f16* __restrict__ v, const float* __restrict__ cs,
                                                               const int* __restrict__ out_pos, f16* __restrict__ kc, uint32_t geom,
                                                               int n_heads, f16* __restrict__ vc, const float* __restrict__ sn,
                                                               const int* __restrict__ pos_ptr, f16* __restrict__ out,
                                                               float* __restrict__ ws, unsigned long long* dbg_ptr,
                                                               const float* __restrict__ alibi) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
    rope_attn_decode_body<PRE, DH, KFT, DBG, ALIBI, ROW, EARLY>(smem_raw, (int)blockIdx.x, q, k, v, cs, out_pos, kc, geom, n_heads, vc, sn,
                                                                pos_ptr, out, ws, dbg_ptr, alibi);
}

// The geometry word of the kernel (host side: the launcher).  0 where a field does not fit.
inline uint32_t rope_attn_geom(int n_heads, int n_kv, int S, int max_seq) {
    const int grp = n_kv > 0 ? n_heads / n_kv : 0;
    if (grp < 1 || grp > 4095 || (S != 1 && S != 2 && S != 4 && S != 8) || max_seq < 16 || max_seq % 16 || max_seq > 32768) return 0;
    uint32_t gsh = 0, lgS = 0;
    if ((grp & (grp - 1)) == 0)
        while ((1 << gsh++) != grp) {}
    while ((1 << lgS) != S) ++lgS;
    return (uint32_t)grp | (gsh << 12) | (lgS << 16) | ((uint32_t)(max_seq / 16) << 18);
}

// LDS bytes of the body for a cache of max_seq positions
__host__ __device__ inline size_t rope_attn_smem_bytes(int max_seq) { return (size_t)(max_seq + 16) * 4 + 16 * 128 * 4 + 64 * 4 + 4 * 4 + 3 * 128 * 2; }

}  // namespace qeft
