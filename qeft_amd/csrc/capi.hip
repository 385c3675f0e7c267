// extern "C" entry points declared in include/qeft_hip.h: argument validation + dispatch.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <stdint.h>

#include "../../include/qeft_hip.h"
#include "qeft_common.h"
#include "host_launch.h"
#include "gemm_w4.h"
#include "gemv_w4.h"
#include "gemv_v3.h"
#include "decode_rows.h"
#include "decode_kv8.h"
#include "prefill_attn.h"
#include "attn_train.h"
#include "train_glue.h"
#include "oweight_optim.h"
#include "calib.h"

static thread_local int g_last_hip_error = 0;
thread_local const char* qeft::g_last_variant = "";
// Few rows: the GEMM entry streams the weights once per 16 rows through the MFMA GEMV instead of 128-row GEMM tiles.
// Measured crossover (tools/bench_gemm.py): one 16-row slice costs ~13 us per 2^24 weights, the
// GEMM at M <= 128 is latency-bound at ~54 us per 4096 of K whatever N is -> the GEMV route wins while
// slices * N <= 16384 (always for one slice).
// With a split-K workspace (qeft_gemm_w4_ws) the GEMM itself is no longer latency-bound at these sizes (M = 128:
// 24 / 31 / 46 us on the three Llama-2-7B shapes) and wins from the second slice on.
static bool small_m_route(int m, int n, bool have_workspace = false) {
    if (m <= 16) return true;
    if (have_workspace) return false;
    const int slices = (m + 15) / 16;
    return m <= 64 && (long long)slices * n <= 16384;
}

static int finish(hipError_t e) {
    if (e == hipSuccess) return QEFT_OK;
    g_last_hip_error = (int)e;
    return QEFT_ERR_LAUNCH;
}

// QEFT_GEMV_V3=0: the reference's gemv entries keep the round-1 kernels (A/B timing, and the parity tests of those kernels)
static bool v3_route_enabled() {
    static const int on = [] { const char* e = getenv("QEFT_GEMV_V3"); return e ? atoi(e) : 1; }();
    return on != 0;
}

// QEFT_GEMM_WS=0: 17 .. 64 rows keep the round-3 routes (split-K GEMM tiles / the round-1 small-M GEMV) (A/B timing)
static bool ws_route_enabled() {
    static const int on = [] { const char* e = getenv("QEFT_GEMM_WS"); return e ? atoi(e) : 1; }();
    return on != 0;
}

// QEFT_GEMV_XG=0: batch rows whose x does not fit the LDS go as several launches / to the split-K GEMM tier (A/B timing)
static int xg_route_mode() {      // 0: never, 1: where the x rows do not fit the LDS, 2 (lab): every batch-row launch without a gather
    static const int on = [] { const char* e = getenv("QEFT_GEMV_XG"); return e ? atoi(e) : 1; }();
    return on;
}
static bool xg_route_enabled() { return xg_route_mode() != 0; }

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static int check_common(int n, int k, int g, int n_out) {
    if (n <= 0 || k <= 0 || n % 4 != 0 || k % 64 != 0) return QEFT_ERR_SHAPE;
    if (g <= 0 || g % 32 != 0 || k % g != 0) return QEFT_ERR_GROUP;
    if (n_out < 0 || n_out % 32 != 0 || n_out >= k) return QEFT_ERR_SHAPE;
    if (n_out > 0 && n % 8 != 0) return QEFT_ERR_SHAPE;
    return QEFT_OK;
}

extern "C" {

int qeft_abi_version(void) { return 1; }

int qeft_last_hip_error(void) { return g_last_hip_error; }

const char* qeft_last_variant(void) { return qeft::g_last_variant; }

const char* qeft_error_string(int code) {
    switch (code) {
        case QEFT_OK: return "ok";
        case QEFT_ERR_BATCH: return "Unsupported batch size for gemv kernel.";
        case QEFT_ERR_SHAPE: return "unsupported shape (need N % 4 == 0 (8 with outliers), K % 64 == 0, n_out % 32 == 0, n_out < K)";
        case QEFT_ERR_GROUP: return "unsupported group size (need a multiple of 32 that divides K)";
        case QEFT_ERR_NULL: return "required pointer is NULL";
        case QEFT_ERR_LAUNCH: return "HIP kernel launch failed (see qeft_last_hip_error)";
        case QEFT_ERR_ALIGN: return "pointer is not 16-byte aligned";
        default: return "unknown error";
    }
}

// ---- v3 decode GEMV (gemv_v3.h).  v3_geom is the only code that fills a V3Geom, v3_args the only code that starts a V3Args.
static int v3_geom(qeft::V3Geom& G, int n, int k, int group_size, int n_out, int mode) {
    if (mode != qeft::V3_MODE_PLAIN && mode != qeft::V3_MODE_PAIR) return QEFT_ERR_SHAPE;
    if (n <= 0 || n % 16 != 0) return QEFT_ERR_SHAPE;
    if (k <= 0 || group_size <= 0 || k % group_size != 0) return QEFT_ERR_GROUP;
    if (!qeft::gemv_v3_ok(k, group_size, n_out)) return QEFT_ERR_SHAPE;
    G.K = k;
    G.n_out = n_out;
    G.nsteps = k / 128;
    G.nfull = (k - n_out) / 128;
    G.ngroups = group_size == k ? 1 : k / 128;
    G.nsets = n / 16;
    return QEFT_OK;
}

// The pack of a v3 launch: the geometry, and the operands every launch names.  The rest stays zero; what a caller adds (the
// checkpoint-layout operands, the epilogue, xn_gamma, bits, m) it sets by name.
static int v3_args(qeft::V3Args& a, const void* x, const void* qweight, const void* sz_packed, const void* oweight, const void* bias,
                   void* y, int n, int k, int group_size, int n_out, int mode) {
    a = qeft::V3Args{};
    if (int e = v3_geom(a.g, n, k, group_size, n_out, mode)) return e;
    a.x = (const qeft::f16*)x;
    a.qw = (const uint8_t*)qweight;
    a.szp = (const uint8_t*)sz_packed;
    a.ow = (const uint8_t*)oweight;
    a.bias = (const qeft::f16*)bias;
    a.y = (qeft::f16*)y;
    return QEFT_OK;
}

// m batch rows (1..16 per launch) through the v3 decode GEMV on the operands as the CHECKPOINT holds them (gemv_v3.h): the
// scales staged raw and packed in LDS (or the sz_packed shadow when the caller has one), the outlier slab from
// oweight_interleaved (the gemv entries) or the plain oweight [n, r] (the GEMM entries), the o_proj gather inside the
// launch, the batch rows as A rows of the same MFMAs.  A batch whose x rows do not fit the block's LDS goes in several
// launches, split evenly; more than `max_launches` of them: not taken (V3_NOT_TAKEN), like a shape the kernel does not serve.
constexpr int V3_NOT_TAKEN = -1000;
// launches v3_rows would make for m rows of this shape on checkpoint-layout operands (0: the kernel does not serve it)
static int v3_rows_launches(int m, int n, int k, int group_size, int n_out) {
    qeft::V3Args v;      // (the geometry alone: v3_lds sizes the checkpoint-layout launch by szp == NULL)
    if (m < 1 || !v3_route_enabled() ||
        v3_args(v, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n, k, group_size, n_out, qeft::V3_MODE_PLAIN) != QEFT_OK)
        return 0;
    int mmax = qeft::gemv_v3_max_rows(v, m);
    if (mmax < m && m > 1 && xg_route_enabled()) {
        v.xg = true;
        if (qeft::gemv_v3_max_rows(v, m) >= m) mmax = m;
    }
    return mmax < 1 ? 0 : (m + mmax - 1) / mmax;
}
constexpr int kGemmRowsOnGemvLaunches = 2;      // the GEMM entries put up to 16 rows on the decode GEMV if that takes two launches at most
static int v3_rows(const void* x, const void* qweight, const void* scales, const void* scaled_zeros, const void* oweight_plain,
                   const void* oweight_il, const void* bias, const int* reorder_ids, const void* sz_packed, void* y, int m, int n,
                   int k, int group_size, int n_out, qeft_stream_t stream, int max_launches) {
    qeft::V3Args v;      // (x and y: per launch, below)
    if (!v3_route_enabled() ||
        v3_args(v, nullptr, qweight, sz_packed, oweight_plain, bias, nullptr, n, k, group_size, n_out, qeft::V3_MODE_PLAIN) != QEFT_OK ||
        !aligned16(scales) || !aligned16(scaled_zeros) || (reorder_ids && !aligned16(reorder_ids)))
        return V3_NOT_TAKEN;
    v.scales = (const qeft::f16*)scales;
    v.zeros = (const qeft::f16*)scaled_zeros;
    v.ow_il = (const uint8_t*)oweight_il;
    v.ids = reorder_ids;
    int mmax = qeft::gemv_v3_max_rows(v, m);
    if ((mmax < m || xg_route_mode() == 2) && m > 1 && !reorder_ids && xg_route_enabled()) {
        // the x rows do not fit the block's LDS: the lanes read their fragments from global memory instead (one launch, any K)
        v.xg = true;
        const int mx = qeft::gemv_v3_max_rows(v, m);
        if (mx >= m) mmax = mx; else v.xg = false;
    }
    if (mmax < 1) return V3_NOT_TAKEN;
    const int nlaunch = (m + mmax - 1) / mmax, per = (m + nlaunch - 1) / nlaunch;      // 7 rows as 4 + 3, not 6 + 1
    if (nlaunch > max_launches) return V3_NOT_TAKEN;
    for (int m0 = 0; m0 < m; m0 += per) {
        v.m = m - m0 < per ? m - m0 : per;
        v.x = (const qeft::f16*)x + (size_t)m0 * k;
        v.y = (qeft::f16*)y + (size_t)m0 * n;
        if (const hipError_t e = qeft::gemv_v3_launch(v, qeft::V3_MODE_PLAIN, (hipStream_t)stream)) return finish(e);
    }
    return QEFT_OK;
}

// The pack of the round-1 GEMV kernels (gemv_w4.hip): value-initialised, then the operands every site names.
// What differs between the sites -- where x comes from, the outlier slice as ow_il or ow_plain, ids, residual, xt_aux,
// sz_blk -- each sets by name (profiles/capi_builders_refactor.log lists every field per site).
// gshift: log2 of a power-of-two group, 31 for one group per row.  0 for any other group: only gemm_impl's small-M branch
// gets here with one, the GEMV entries have answered QEFT_ERR_GROUP before they build the pack.
static qeft::GemvArgs gemv_args(const void* x, const void* qweight, const void* scales, const void* scaled_zeros, const void* bias,
                                void* y, int n, int k, int group_size, int n_out) {
    qeft::GemvArgs a{};
    a.x = (const qeft::f16*)x;
    a.qw = (const uint8_t*)qweight;
    a.scales = (const qeft::f16*)scales;
    a.zeros = (const qeft::f16*)scaled_zeros;
    a.bias = (const qeft::f16*)bias;
    a.y = (qeft::f16*)y;
    a.N = n;
    a.K = k;
    a.G = group_size;
    a.n_out = n_out;
    a.gshift = group_size == k ? 31 : (group_size & (group_size - 1)) == 0 ? __builtin_ctz(group_size) : 0;
    a.m_rt = 1;
    return a;
}

static int gemv_fused_impl(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                           const void* oweight_il, const void* bias, const int* reorder_ids, const void* residual,
                           const void* sz_packed, void* y, int m, int n, int k, int group_size, int n_out,
                           qeft_stream_t stream, int bits = 4) {
    if (m < 1 || (bits == 4 && m > 7)) return QEFT_ERR_BATCH;
    if (int e = check_common(n, k, group_size, n_out)) return e;
    if (!x || !qweight || !scales || !scaled_zeros || !y || (n_out > 0 && !oweight_il)) return QEFT_ERR_NULL;
    if (!aligned16(x) || !aligned16(qweight) || (n_out > 0 && !aligned16(oweight_il))) return QEFT_ERR_ALIGN;
    if (sz_packed && !aligned16(sz_packed)) return QEFT_ERR_ALIGN;
    if (bits == 4 && !residual) {
        const int r = v3_rows(x, qweight, scales, scaled_zeros, nullptr, oweight_il, bias, reorder_ids, sz_packed, y, m, n, k, group_size,
                              n_out, stream, 1 << 30);
        if (r != V3_NOT_TAKEN) return r;
    }
    if (group_size != k && (group_size & (group_size - 1)) != 0) return QEFT_ERR_GROUP;  // GEMV: power of two or == K
    qeft::GemvArgs a = gemv_args(x, qweight, scales, scaled_zeros, bias, y, n, k, group_size, n_out);
    a.ow_il = (const qeft::f16*)oweight_il;
    a.ids = reorder_ids;
    a.residual = (const qeft::f16*)residual;
    a.sz_blk = (const uint32_t*)sz_packed;
    if (bits == 3 && reorder_ids) return QEFT_ERR_SHAPE;   // the gather is the caller's (qlinear.py:275) for w3
    return finish(qeft::gemv_w4_launch(qeft::kGemvRows, bits, a, m, (hipStream_t)stream));
}

int qeft_gemv_w4_fused(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                       const void* oweight_il, const void* bias, const int* reorder_ids, const void* residual,
                       const void* sz_packed, void* y, int m, int n, int k, int group_size, int n_out,
                       qeft_stream_t stream) {
    return gemv_fused_impl(x, qweight, scales, scaled_zeros, oweight_il, bias, reorder_ids, residual, sz_packed, y, m, n,
                           k, group_size, n_out, stream);
}

int qeft_gemv_w4(const void* x, const void* qweight, const void* scales, const void* scaled_zeros, void* y, int m,
                 int n, int k, int group_size, qeft_stream_t stream) {
    return gemv_fused_impl(x, qweight, scales, scaled_zeros, nullptr, nullptr, nullptr, nullptr, nullptr, y, m, n, k,
                           group_size, 0, stream);
}

int qeft_gemv_w4_qeft(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                      const void* oweight_il, void* y, int m, int n, int k, int group_size, int n_out,
                      qeft_stream_t stream) {
    return gemv_fused_impl(x, qweight, scales, scaled_zeros, oweight_il, nullptr, nullptr, nullptr, nullptr, y, m, n, k,
                           group_size, n_out, stream);
}

static int gemm_impl(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                     const void* oweight, const void* bias, void* y, int m, int n, int k, int group_size, int n_out,
                     qeft_stream_t stream, void* workspace, size_t workspace_bytes, const void* silu_gate = nullptr,
                     bool* fused_epilogue = nullptr) {
    if (fused_epilogue) *fused_epilogue = false;
    if (m < 1) return QEFT_ERR_SHAPE;
    if (!oweight) n_out = 0;
    if (int e = check_common(n, k, group_size, n_out)) return e;
    if (!x || !qweight || !scales || !scaled_zeros || !y) return QEFT_ERR_NULL;
    if (!aligned16(x) || !aligned16(qweight) || (n_out > 0 && !aligned16(oweight))) return QEFT_ERR_ALIGN;
    if (m <= qeft::V3_MAX_M && (n_out > 0) == (oweight != nullptr)) {
        // up to 16 rows: the batch rows ride as A rows of the decode GEMV's MFMAs -- one weight stream (two launches at most where
        // the caller brought the split-K workspace: a long x whose rows do not fit the LDS then falls to the split-K GEMM tier
        // below rather than stream the weights three times; without a workspace three streams still beat an unsplit 128-row tile)
        const int r = v3_rows(x, qweight, scales, scaled_zeros, oweight, nullptr, bias, nullptr, nullptr, y, m, n, k, group_size, n_out,
                              stream, workspace != nullptr && workspace_bytes > 0 && (group_size & (group_size - 1)) == 0
                                          ? kGemmRowsOnGemvLaunches : (1 << 30));      // (per-channel scales: no split-K tier to fall to)
        if (r != V3_NOT_TAKEN) return r;
    }
    if (ws_route_enabled() && (n_out > 0) == (oweight != nullptr) && aligned16(scales) && aligned16(scaled_zeros) &&
        qeft::gemm_ws_supported(m, n, k, group_size, n_out)) {
        // 17 .. 64 rows: the weight-stationary tier (gemm_ws.hip) -- one launch, one pass over the packed weights, no workspace
        return finish(qeft::gemm_ws_launch(x, qweight, scales, scaled_zeros, oweight, bias, y, m, n, k, n_out, (hipStream_t)stream));
    }
    if (small_m_route(m, n, workspace != nullptr && workspace_bytes > 0) && (n_out > 0) == (oweight != nullptr) &&
        !(m <= qeft::V3_MAX_M && v3_route_enabled() && n % 16 == 0 && qeft::gemv_v3_ok(k, group_size, n_out))) {
        // few rows: stream the weights once per 16 rows through the MFMA GEMV instead of 128-row GEMM tiles.
        // (gemm_4bit semantics with oweight == NULL and a non-zero slice -- dead nibbles -- stays on the GEMM kernel.)
        qeft::GemvArgs a = gemv_args(x, qweight, scales, scaled_zeros, bias, y, n, k, group_size, n_out);
        a.ow_plain = (const qeft::f16*)oweight;      // (any group that is a multiple of 32 gets here: gshift 0 for one that is no power of two)
        const hipError_t e = qeft::gemv_w4_launch(qeft::kGemvSmallM, 4, a, m, (hipStream_t)stream);
        if (e == hipSuccess) return QEFT_OK;
        if (e != hipErrorNotSupported) return finish(e);
    }
    return finish(qeft::gemm_w4_launch(x, qweight, scales, scaled_zeros, oweight, bias, y, m, n, k, group_size, n_out,
                                       (hipStream_t)stream, workspace, workspace_bytes, silu_gate, fused_epilogue));
}

int qeft_gemm_w4(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                 const void* oweight, const void* bias, void* y, int m, int n, int k, int group_size, int n_out,
                 qeft_stream_t stream) {
    return gemm_impl(x, qweight, scales, scaled_zeros, oweight, bias, y, m, n, k, group_size, n_out, stream, nullptr, 0);
}

int qeft_gemm_w4_silu_mul(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                          const void* oweight, const void* bias, const void* gate, void* y, int m, int n, int k,
                          int group_size, int n_out, qeft_stream_t stream) {
    if (!gate) return QEFT_ERR_NULL;
    if (n % 8 != 0 || (long long)m * n > 0x7fffffffLL) return QEFT_ERR_SHAPE;
    if (!aligned16(gate) || !aligned16(y)) return QEFT_ERR_ALIGN;
    bool fused = false;       // reported by the launch itself (the variant string is diagnostic only)
    const int e = gemm_impl(x, qweight, scales, scaled_zeros, oweight, bias, y, m, n, k, group_size, n_out, stream, nullptr, 0,
                            gate, &fused);
    if (e != QEFT_OK || fused) return e;
    // a tier without the fused epilogue: the product is in y, finish in place
    return finish(qeft::silu_mul_launch(gate, y, y, m * n, (hipStream_t)stream));
}

int qeft_gemm_w4_gateup_supported(int m, int n2, int k, int group_size, int n_out) {
    if (m < 1 || check_common(n2, k, group_size, n_out) != QEFT_OK || (long long)m * n2 > 0x7fffffffLL) return 0;
    return qeft::gemm_w4_pair64_ok(m, n2, k, group_size, n_out) ? 1 : 0;
}

int qeft_gemm_w4_gateup(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                        const void* oweight, const void* bias, void* y, int m, int n2, int k, int group_size, int n_out,
                        qeft_stream_t stream) {
    if (!oweight) n_out = 0;
    if (!qeft_gemm_w4_gateup_supported(m, n2, k, group_size, n_out)) return QEFT_ERR_SHAPE;
    if (!x || !qweight || !scales || !scaled_zeros || !y) return QEFT_ERR_NULL;
    if (!aligned16(x) || !aligned16(qweight) || !aligned16(y) || (n_out > 0 && !aligned16(oweight))) return QEFT_ERR_ALIGN;
    return finish(qeft::gemm_w4_launch(x, qweight, scales, scaled_zeros, oweight, bias, y, m, n2, k, group_size, n_out,
                                       (hipStream_t)stream, nullptr, 0, qeft::kSiluPair64));
}

/* ---- 3-bit extension: GEMM forward / dX on the 3-bit stream itself (the loader-wave tiers), no expansion pass */
int qeft_gemm_w3_supported(int m, int n, int k, int group_size, int n_out) {
    if (m < 1 || n < 16 || k < 128 || group_size < 1 || n_out < 0) return 0;
    return qeft::gemm_w3_native_tile(m, n, k, group_size, n_out) != 0;
}

int qeft_gemm_w3(const void* x, const void* qweight3, const void* scales, const void* scaled_zeros, const void* oweight,
                 const void* bias, void* y, int m, int n, int k, int group_size, int n_out, qeft_stream_t stream) {
    if (!oweight) n_out = 0;
    if (!qeft_gemm_w3_supported(m, n, k, group_size, n_out)) return QEFT_ERR_SHAPE;
    if (!x || !qweight3 || !scales || !scaled_zeros || !y) return QEFT_ERR_NULL;
    if (!aligned16(x) || !aligned16(qweight3) || !aligned16(y) || (n_out > 0 && !aligned16(oweight))) return QEFT_ERR_ALIGN;
    return finish(qeft::gemm_w4_launch(x, qweight3, scales, scaled_zeros, oweight, bias, y, m, n, k, group_size, n_out,
                                       (hipStream_t)stream, nullptr, 0, nullptr, nullptr, 3));
}

int qeft_gemm_w3_dx_supported(int m, int n, int k, int group_size, int n_out) {
    if (m < 1 || n < 16 || k < 128 || group_size < 1 || n_out < 0) return 0;
    return qeft::gemm_w3_dx_native(m, n, k, group_size, n_out) ? 1 : 0;
}

int qeft_gemm_w3_dx(const void* dy, const void* qweight3, const void* scales, const void* scaled_zeros, const void* oweight,
                    void* dx, int m, int n, int k, int group_size, int n_out, qeft_stream_t stream) {
    if (!oweight) n_out = 0;
    if (!qeft_gemm_w3_dx_supported(m, n, k, group_size, n_out)) return QEFT_ERR_SHAPE;
    if (!dy || !qweight3 || !scales || !scaled_zeros || !dx) return QEFT_ERR_NULL;
    if (!aligned16(dy) || (reinterpret_cast<uintptr_t>(qweight3) & 3u) || !aligned16(dx) || (n_out > 0 && !aligned16(oweight))) return QEFT_ERR_ALIGN;
    return finish(qeft::gemm_w4_dx_launch(dy, qweight3, scales, scaled_zeros, oweight, dx, m, n, k, group_size, n_out,
                                          (hipStream_t)stream, nullptr, 0, 3));
}

long long qeft_gemm_w4_workspace_bytes(int m, int n, int k, int n_out) {
    if (m < 1 || n < 1 || k < 1 || n_out < 0 || n_out >= k) return 0;
    if (m <= qeft::V3_MAX_M && k % 128 == 0 && n % 16 == 0 && (n_out == 0 || n_out == 128)) {
        // up to 16 rows of a shape the decode GEMV serves (group size 128 assumed: the larger LDS plan): no workspace if gemm_impl
        // will put them there, the split-K tier's otherwise (three weight streams would cost more than its partial sums)
        const int l = v3_rows_launches(m, n, k, 128, n_out);
        if (l >= 1 && l <= kGemmRowsOnGemvLaunches) return 0;
    } else if (ws_route_enabled() && qeft::gemm_ws_supported(m, n, k, 128, n_out)) {
        return 0;       // (group size 128 assumed, as above: the weight-stationary tier needs no workspace)
    } else if (small_m_route(m, n, true)) {
        return 0;
    }
    int s = qeft::gemm_w4_split(m, n, k, n_out);
    const int s3 = qeft::gemm_v3_split(m, n, k, n_out);       // the loader-wave tier's split (whichever tier the launch takes, it fits)
    if (s3 > s) s = s3;
    return s > 1 ? (long long)s * m * n * 4 : 0;
}

int qeft_gemm_w4_ws(const void* x, const void* qweight, const void* scales, const void* scaled_zeros,
                    const void* oweight, const void* bias, void* y, void* workspace, long long workspace_bytes, int m,
                    int n, int k, int group_size, int n_out, qeft_stream_t stream) {
    if (workspace && !aligned16(workspace)) return QEFT_ERR_ALIGN;
    return gemm_impl(x, qweight, scales, scaled_zeros, oweight, bias, y, m, n, k, group_size, n_out, stream, workspace,
                     workspace && workspace_bytes > 0 ? (size_t)workspace_bytes : 0);
}

static int gemm_dx_impl(const void* dy, const void* qweight, const void* scales, const void* scaled_zeros,
                        const void* oweight, void* dx, int m, int n, int k, int group_size, int n_out,
                        qeft_stream_t stream, void* workspace, size_t workspace_bytes) {
    if (m < 1) return QEFT_ERR_SHAPE;
    if (!oweight) n_out = 0;
    if (int e = check_common(n, k, group_size, n_out)) return e;
    if (n % 8 != 0) return QEFT_ERR_SHAPE;  // dy rows are read 16 bytes at a time
    if (!dy || !qweight || !scales || !scaled_zeros || !dx) return QEFT_ERR_NULL;
    if (!aligned16(dy) || !aligned16(qweight) || !aligned16(dx) || (n_out > 0 && !aligned16(oweight)))
        return QEFT_ERR_ALIGN;
    return finish(qeft::gemm_w4_dx_launch(dy, qweight, scales, scaled_zeros, oweight, dx, m, n, k, group_size, n_out,
                                          (hipStream_t)stream, workspace, workspace_bytes));
}

int qeft_gemm_w4_dx(const void* dy, const void* qweight, const void* scales, const void* scaled_zeros,
                    const void* oweight, void* dx, int m, int n, int k, int group_size, int n_out,
                    qeft_stream_t stream) {
    return gemm_dx_impl(dy, qweight, scales, scaled_zeros, oweight, dx, m, n, k, group_size, n_out, stream, nullptr, 0);
}

long long qeft_gemm_w4_dx_workspace_bytes(int m, int n, int k) {
    if (m < 1 || n < 1 || k < 64 || k % 4 != 0) return 0;
    if (qeft::gemm_dx128_takes(m, k)) return 0;       // the 128-wide tile: no split
    const int s = qeft::gemm_w4_dx_split(m, n, k);
    return s > 1 ? (long long)s * m * k * 4 : 0;
}

int qeft_gemm_w4_dx_ws(const void* dy, const void* qweight, const void* scales, const void* scaled_zeros,
                       const void* oweight, void* dx, void* workspace, long long workspace_bytes, int m, int n, int k,
                       int group_size, int n_out, qeft_stream_t stream) {
    if (workspace && !aligned16(workspace)) return QEFT_ERR_ALIGN;
    return gemm_dx_impl(dy, qweight, scales, scaled_zeros, oweight, dx, m, n, k, group_size, n_out, stream, workspace,
                        workspace && workspace_bytes > 0 ? (size_t)workspace_bytes : 0);
}

int qeft_grad_oweight(const void* dy, const void* x, void* d_oweight_f32, int m, int n, int k, int n_out,
                      qeft_stream_t stream) {
    if (m < 1 || n <= 0 || k <= 0 || n_out <= 0 || n_out > k) return QEFT_ERR_SHAPE;
    if (!dy || !x || !d_oweight_f32) return QEFT_ERR_NULL;
    return finish(qeft::grad_oweight_launch(dy, x, d_oweight_f32, m, n, k, n_out, (hipStream_t)stream));
}

/* ---- the launchers' plans as integers: no HIP call, no GPU needed (tests/test_gemm_plan.py) */
static qeft::GemmOverrides overrides_from(const int* v) {
    if (!v) return qeft::gemm_overrides();
    qeft::GemmOverrides o;
    o.v3 = v[0], o.v3m = v[1], o.v3s = v[2], o.nwv = v[3], o.dx_v3 = v[4], o.dow_bn = v[5], o.abl = v[6], o.v1 = v[7] != 0;
    return o;
}
static int plan_out(const qeft::GemmPlan& p, int* out) {
    const int v[QEFT_GEMM_PLAN_INTS] = {p.tier, (int)p.gx, (int)p.gy, (int)p.gz, p.threads, p.lds, p.S, p.reduce(), p.fused, p.supported()};
    memcpy(out, v, sizeof(v));
    return QEFT_OK;
}
// (the plans divide by tile counts: at least one row, one column and one 64-wide k-tile)
static int plan_args(int m, int n, int k, int g, int n_out, const int* out) {
    return !out ? QEFT_ERR_NULL : (m < 1 || n < 1 || k < 64 || g < 1 || n_out < 0) ? QEFT_ERR_SHAPE : QEFT_OK;
}

int qeft_gemm_w4_plan(int m, int n, int k, int group_size, int n_out, int bits, int gate, long long workspace_bytes,
                      const int* overrides, int* out) {
    if (int e = plan_args(m, n, k, group_size, n_out, out)) return e;
    if (gate < 0 || gate > 2) return QEFT_ERR_SHAPE;
    return plan_out(qeft::gemm_w4_plan(m, n, k, group_size, n_out, bits, gate, workspace_bytes > 0 ? (size_t)workspace_bytes : 0,
                                       overrides_from(overrides)), out);
}

int qeft_gemm_w4_dx_plan(int m, int n, int k, int group_size, int n_out, int bits, long long workspace_bytes, const int* overrides,
                         int* out) {
    if (int e = plan_args(m, n, k, group_size, n_out, out)) return e;
    return plan_out(qeft::gemm_w4_dx_plan(m, n, k, group_size, n_out, bits, workspace_bytes > 0 ? (size_t)workspace_bytes : 0,
                                          overrides_from(overrides)), out);
}

int qeft_grad_oweight_plan(int n, int k, int n_out, const int* overrides, int* out) {
    return out ? plan_out(qeft::grad_oweight_plan(n, k, n_out, overrides_from(overrides)), out) : QEFT_ERR_NULL;
}

const char* qeft_gemm_tier_name(int tier) { return qeft::gemm_tier_variant(tier); }

int qeft_gemv_w4_plan(int kind, int bits, int m, int nparts, const int* n_parts, int k, int group_size, int n_out, int flags,
                      const int* overrides, int* out) {
    if (!n_parts || !out) return QEFT_ERR_NULL;
    if (kind < qeft::kGemvRows || kind > qeft::kGemvSilu || (bits != 4 && bits != 3) || m < 0 || nparts < 1 ||
        nparts > (kind == qeft::kGemvGroup ? 3 : 1) || k < 64 || k % 64 != 0 || group_size < 1 || k % group_size != 0 || n_out < 0 ||
        (bits == 4 && n_out >= k))
        return QEFT_ERR_SHAPE;
    for (int p = 0; p < nparts; ++p)
        if (n_parts[p] < 4 || n_parts[p] % 4 != 0) return QEFT_ERR_SHAPE;
    if (overrides && overrides[1] != 0 && overrides[1] != 4 && overrides[1] != 6) return QEFT_ERR_SHAPE;      // depths that have instances
    const qeft::GemvOverrides ov = overrides ? qeft::GemvOverrides{overrides[0], overrides[1]} : qeft::gemv_w4_overrides();
    const qeft::GemvPlan p = qeft::gemv_w4_plan(kind, bits, m, nparts, n_parts, k, group_size, n_out, (flags & 1) != 0, (flags & 2) != 0, ov);
    const qeft::GemvLaunch &b = p.body, &t = p.tail;
    const int v[QEFT_GEMV_W4_PLAN_INTS] = {(int)p.rc, p.variant, p.mfma, p.rc ? 0 : p.bits, p.D, p.rgi, p.outl, p.xg, p.xt, p.threads,
                                           p.blk_end[0], p.blk_end[1], p.blk_end[2], b.count, b.rows, b.M, b.grid, b.lds, b.rs_cap,
                                           t.count, t.rows, t.M, t.grid, t.lds, t.rs_cap};
    memcpy(out, v, sizeof(v));
    return QEFT_OK;
}

const char* qeft_gemv_w4_variant_name(int variant) { return qeft::gemv_w4_variant(variant); }

int qeft_dequant_w4(const void* qweight, const void* scales, const void* scaled_zeros, const void* oweight,
                    void* w_out, int n, int k, int group_size, int n_out, qeft_stream_t stream) {
    if (!oweight) n_out = 0;
    if (int e = check_common(n, k, group_size, n_out)) return e;
    if (!qweight || !scales || !scaled_zeros || !w_out) return QEFT_ERR_NULL;
    if (!aligned16(qweight) || !aligned16(w_out) || (n_out > 0 && !aligned16(oweight))) return QEFT_ERR_ALIGN;
    return finish(qeft::dequant_w4_launch(qweight, scales, scaled_zeros, oweight, w_out, n, k, group_size, n_out,
                                          (hipStream_t)stream));
}

int qeft_pack_scales(const void* scales, const void* scaled_zeros, void* sz_packed, int n, int k, int group_size,
                     qeft_stream_t stream) {
    if (n <= 0 || n % 16 != 0 || k <= 0 || group_size <= 0 || k % group_size != 0) return QEFT_ERR_SHAPE;
    if (group_size != 128 && group_size != k) return QEFT_ERR_GROUP;   // what the MFMA decode GEMV consumes
    if (!scales || !scaled_zeros || !sz_packed) return QEFT_ERR_NULL;
    if (!aligned16(sz_packed)) return QEFT_ERR_ALIGN;
    return finish(qeft::pack_scales_launch(scales, scaled_zeros, sz_packed, n, k / group_size, (hipStream_t)stream));
}

int qeft_pack_oweight(const void* oweight, void* oweight_il, int n, int n_out, qeft_stream_t stream) {
    if (n <= 0 || n % 8 != 0 || n_out <= 0 || n_out % 32 != 0) return QEFT_ERR_SHAPE;
    if (!oweight || !oweight_il) return QEFT_ERR_NULL;
    return finish(qeft::pack_oweight_launch(oweight, oweight_il, n, n_out, (hipStream_t)stream));
}

static int gemv_group_impl(const void* x, const void* norm_gamma, float norm_eps, int nparts,
                           const void* const* qweight, const void* const* scales, const void* const* scaled_zeros,
                           const void* const* oweight_il, const void* const* bias, const void* const* sz_packed,
                           void* const* y, const int* n, int k, int group_size, int n_out, qeft_stream_t stream, int bits) {
    if (nparts < 1 || nparts > 3) return QEFT_ERR_SHAPE;
    if (!x || !qweight || !scales || !scaled_zeros || !y || !n) return QEFT_ERR_NULL;
    if (group_size != k && (group_size & (group_size - 1)) != 0) return QEFT_ERR_GROUP;
    qeft::GemvGroupArgs g{};
    g.x = (const qeft::f16*)x;
    for (int p = 0; p < nparts; ++p) {
        if (int e = check_common(n[p], k, group_size, n_out)) return e;
        if (!qweight[p] || !scales[p] || !scaled_zeros[p] || !y[p] || (n_out > 0 && (!oweight_il || !oweight_il[p])))
            return QEFT_ERR_NULL;
        if (!aligned16(qweight[p]) || (n_out > 0 && !aligned16(oweight_il[p]))) return QEFT_ERR_ALIGN;
        g.qw[p] = (const uint8_t*)qweight[p];
        g.scales[p] = (const qeft::f16*)scales[p];
        g.zeros[p] = (const qeft::f16*)scaled_zeros[p];
        g.ow_il[p] = n_out > 0 ? (const qeft::f16*)oweight_il[p] : nullptr;
        g.bias[p] = bias ? (const qeft::f16*)bias[p] : nullptr;
        g.sz_blk[p] = sz_packed ? (const uint32_t*)sz_packed[p] : nullptr;
        if (g.sz_blk[p] && !aligned16(g.sz_blk[p])) return QEFT_ERR_ALIGN;
        g.y[p] = (qeft::f16*)y[p];
        g.N[p] = n[p];
    }
    if (!aligned16(x)) return QEFT_ERR_ALIGN;
    g.K = k;
    g.G = group_size;
    g.n_out = n_out;
    g.gshift = (group_size == k) ? 31 : __builtin_ctz(group_size);
    if (norm_gamma && !aligned16(norm_gamma)) return QEFT_ERR_ALIGN;
    g.xt_aux = (const qeft::f16*)norm_gamma;
    g.xt_eps = norm_eps;
    return finish(qeft::gemv_w4_group_launch(bits, g, nparts, (hipStream_t)stream));
}

int qeft_gemv_w4_group(const void* x, const void* norm_gamma, float norm_eps, int nparts,
                       const void* const* qweight, const void* const* scales, const void* const* scaled_zeros,
                       const void* const* oweight_il, const void* const* bias, const void* const* sz_packed,
                       void* const* y, const int* n, int k, int group_size, int n_out, qeft_stream_t stream) {
    return gemv_group_impl(x, norm_gamma, norm_eps, nparts, qweight, scales, scaled_zeros, oweight_il, bias, sz_packed, y,
                           n, k, group_size, n_out, stream, 4);
}

int qeft_gemv_w3_group(const void* x, const void* norm_gamma, float norm_eps, int nparts,
                       const void* const* qweight3, const void* const* scales, const void* const* scaled_zeros,
                       const void* const* oweight_il, const void* const* bias, const void* const* sz_packed,
                       void* const* y, const int* n, int k, int group_size, int n_out, qeft_stream_t stream) {
    return gemv_group_impl(x, norm_gamma, norm_eps, nparts, qweight3, scales, scaled_zeros, oweight_il, bias, sz_packed,
                           y, n, k, group_size, n_out, stream, 3);
}

static int gemv_silu_impl(const void* gate, const void* up, const void* qweight, const void* scales,
                          const void* scaled_zeros, const void* oweight_il, const void* bias, const void* residual,
                          const void* sz_packed, void* y, int n, int k, int group_size, int n_out, qeft_stream_t stream,
                          int bits) {
    if (int e = check_common(n, k, group_size, n_out)) return e;
    if (sz_packed && !aligned16(sz_packed)) return QEFT_ERR_ALIGN;
    if (!gate || !up || !qweight || !scales || !scaled_zeros || !y || (n_out > 0 && !oweight_il)) return QEFT_ERR_NULL;
    if (!aligned16(gate) || !aligned16(up) || !aligned16(qweight) || (n_out > 0 && !aligned16(oweight_il)))
        return QEFT_ERR_ALIGN;
    if (group_size != k && (group_size & (group_size - 1)) != 0) return QEFT_ERR_GROUP;
    qeft::GemvArgs a = gemv_args(gate, qweight, scales, scaled_zeros, bias, y, n, k, group_size, n_out);
    a.xt_aux = (const qeft::f16*)up;
    a.ow_il = (const qeft::f16*)oweight_il;
    a.residual = (const qeft::f16*)residual;
    a.sz_blk = (const uint32_t*)sz_packed;
    return finish(qeft::gemv_w4_launch(qeft::kGemvSilu, bits, a, 1, (hipStream_t)stream));
}

int qeft_gemv_w4_silu(const void* gate, const void* up, const void* qweight, const void* scales,
                      const void* scaled_zeros, const void* oweight_il, const void* bias, const void* residual,
                      const void* sz_packed, void* y, int n, int k, int group_size, int n_out, qeft_stream_t stream) {
    return gemv_silu_impl(gate, up, qweight, scales, scaled_zeros, oweight_il, bias, residual, sz_packed, y, n, k,
                          group_size, n_out, stream, 4);
}

int qeft_gemv_w3_silu(const void* gate, const void* up, const void* qweight3, const void* scales,
                      const void* scaled_zeros, const void* oweight_il, const void* bias, const void* residual,
                      const void* sz_packed, void* y, int n, int k, int group_size, int n_out, qeft_stream_t stream) {
    return gemv_silu_impl(gate, up, qweight3, scales, scaled_zeros, oweight_il, bias, residual, sz_packed, y, n, k,
                          group_size, n_out, stream, 3);
}

int qeft_gemv_w3(const void* x, const void* qweight3, const void* scales, const void* scaled_zeros,
                 const void* oweight_il, const void* bias, const void* residual, const void* sz_packed, void* y, int m,
                 int n, int k, int group_size, int n_out, qeft_stream_t stream) {
    return gemv_fused_impl(x, qweight3, scales, scaled_zeros, oweight_il, bias, nullptr, residual, sz_packed, y, m, n, k,
                           group_size, n_out, stream, 3);
}

int qeft_expand_w3(const void* qweight3, void* qweight4, int n, int k, int n_out, qeft_stream_t stream) {
    if (n <= 0 || k <= 0 || n % 16 != 0 || k % 128 != 0 || n_out < 0 || n_out % 128 != 0 || n_out >= k) return QEFT_ERR_SHAPE;
    if (!qweight3 || !qweight4) return QEFT_ERR_NULL;
    if (!aligned16(qweight4) || (reinterpret_cast<uintptr_t>(qweight3) & 3u)) return QEFT_ERR_ALIGN;
    return finish(qeft::expand_w3_launch(qweight3, qweight4, n, k, n_out, (hipStream_t)stream));
}

int qeft_rmsnorm(const void* x, const void* add, const void* gamma, void* res_out, void* y, int m, int hidden,
                 float eps, qeft_stream_t stream) {
    if (m < 1 || hidden < 8 || hidden % 8 != 0) return QEFT_ERR_SHAPE;
    if (!x || !gamma || !y) return QEFT_ERR_NULL;
    if (!aligned16(x) || !aligned16(y) || !aligned16(gamma) || (add && !aligned16(add)) || (res_out && !aligned16(res_out)))
        return QEFT_ERR_ALIGN;
    return finish(qeft::rmsnorm_launch(x, add, gamma, res_out, y, m, hidden, eps, (hipStream_t)stream));
}

int qeft_rmsnorm_f32(const void* x32, const void* gamma, void* y, int m, int hidden, float eps, qeft_stream_t stream) {
    if (m < 1 || hidden < 8 || hidden % 8 != 0) return QEFT_ERR_SHAPE;
    if (!x32 || !gamma || !y) return QEFT_ERR_NULL;
    if (!aligned16(x32) || !aligned16(y) || !aligned16(gamma)) return QEFT_ERR_ALIGN;
    return finish(qeft::rmsnorm_f32_launch(x32, gamma, y, m, hidden, eps, (hipStream_t)stream));
}

int qeft_rope_rows(void* x, const void* cos_tab, const void* sin_tab, int t, int n_heads, int row_stride,
                   qeft_stream_t stream) {
    if (t < 1 || n_heads < 1 || row_stride < n_heads * 128) return QEFT_ERR_SHAPE;
    if (!x || !cos_tab || !sin_tab) return QEFT_ERR_NULL;
    return finish(qeft::rope_rows_launch(x, cos_tab, sin_tab, t, n_heads, row_stride, (hipStream_t)stream));
}

int qeft_lm_head_f16(const void* h32, const void* gamma, const void* weight, void* logits, int hidden, int vocab, float eps,
                     qeft_stream_t stream) {
    if (vocab < 1 || hidden < 512 || hidden % 512 != 0) return QEFT_ERR_SHAPE;
    if (!h32 || !gamma || !weight || !logits) return QEFT_ERR_NULL;
    if (!aligned16(h32) || !aligned16(gamma) || !aligned16(weight)) return QEFT_ERR_ALIGN;
    hipError_t e = qeft::lm_head_f16_launch(h32, gamma, weight, logits, hidden, vocab, eps, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) return QEFT_ERR_SHAPE;
    return finish(e);
}

int qeft_silu_mul(const void* gate, const void* up, void* out, int n, qeft_stream_t stream) {
    if (n < 8 || n % 8 != 0) return QEFT_ERR_SHAPE;
    if (!gate || !up || !out) return QEFT_ERR_NULL;
    if (!aligned16(gate) || !aligned16(up) || !aligned16(out)) return QEFT_ERR_ALIGN;
    return finish(qeft::silu_mul_launch(gate, up, out, n, (hipStream_t)stream));
}

void qeft_debug_attn_stamps(void* p) { qeft::g_attn_dbg = (unsigned long long*)p; }

int qeft_attn_workspace_bytes(int n_heads, int n_split) {
    if (n_heads < 1 || n_heads > 4096 || n_split < 1 || n_split > 8) return 0;
    return (int)qeft::attn_workspace_bytes(n_heads, n_split);
}

int qeft_rope_attn_decode(const void* q, const void* k, const void* v, const void* cos_tab, const void* sin_tab,
                          int tab_rows, void* k_cache, void* v_cache, const int* pos, const int* out_pos, void* out,
                          void* workspace, int n_split, int n_heads, int n_kv_heads, int max_seq, qeft_stream_t stream) {
    if (tab_rows != 1 && tab_rows < max_seq) return QEFT_ERR_SHAPE;
    if (n_heads < 1 || n_kv_heads < 1 || n_heads % n_kv_heads != 0 || max_seq < 16 || max_seq % 16 != 0 || max_seq > 32768)
        return QEFT_ERR_SHAPE;
    if (n_split != 1 && n_split != 2 && n_split != 4 && n_split != 8) return QEFT_ERR_SHAPE;
    if (!q || !k || !v || !cos_tab || !sin_tab || !k_cache || !v_cache || !pos || !out) return QEFT_ERR_NULL;
    if (n_split > 1 && !workspace) return QEFT_ERR_NULL;
    if (!aligned16(k_cache) || !aligned16(v_cache) || !aligned16(workspace)) return QEFT_ERR_ALIGN;
    return finish(qeft::rope_attn_decode_launch(q, k, v, cos_tab, sin_tab, k_cache, v_cache, pos, out_pos, out, workspace,
                                                n_heads, n_kv_heads, max_seq, n_split, tab_rows, (hipStream_t)stream));
}

static int sqa_impl(const void* q, const void* k, const void* v, const void* cos_tab, const void* sin_tab, int tab_rows, void* k_cache_ft,
                    void* v_cache, const int* pos, void* out, int n_heads, int n_kv_heads, int max_seq, const float* alibi_slopes,
                    qeft_stream_t stream) {
    if (tab_rows != 1 && tab_rows < max_seq) return QEFT_ERR_SHAPE;
    if (n_heads < 1 || n_kv_heads < 1 || n_heads % n_kv_heads != 0 || max_seq < 16 || max_seq % 16 != 0 || max_seq > 32768)
        return QEFT_ERR_SHAPE;
    if (!q || !k || !v || !cos_tab || !sin_tab || !k_cache_ft || !v_cache || !pos || !out) return QEFT_ERR_NULL;
    if (!aligned16(k_cache_ft) || !aligned16(v_cache)) return QEFT_ERR_ALIGN;
    return finish(qeft::rope_attn_decode_launch(q, k, v, cos_tab, sin_tab, k_cache_ft, v_cache, pos, nullptr, out, nullptr,
                                                n_heads, n_kv_heads, max_seq, 1, tab_rows, (hipStream_t)stream, true, alibi_slopes));
}

int qeft_single_query_attention(const void* q, const void* k, const void* v, const void* cos_tab, const void* sin_tab,
                                int tab_rows, void* k_cache_ft, void* v_cache, const int* pos, void* out, int n_heads,
                                int n_kv_heads, int max_seq, qeft_stream_t stream) {
    return sqa_impl(q, k, v, cos_tab, sin_tab, tab_rows, k_cache_ft, v_cache, pos, out, n_heads, n_kv_heads, max_seq, nullptr, stream);
}

int qeft_single_query_attention_generic(const void* q, const void* k, const void* v, void* k_cache_ft, void* v_cache, const int* pos,
                                        void* out, int n_heads, int n_kv_heads, int max_seq, int head_dim, const float* alibi_slopes,
                                        qeft_stream_t stream) {
    if (!q || !k || !v || !k_cache_ft || !v_cache || !pos || !out) return QEFT_ERR_NULL;
    if (n_heads < 1 || n_kv_heads < 1 || n_heads % n_kv_heads != 0 || head_dim < 8 || head_dim > 256 || head_dim % 8 != 0 ||
        max_seq < 1 || max_seq > 32768)
        return QEFT_ERR_SHAPE;
    if (!aligned16(k_cache_ft) || !aligned16(v_cache)) return QEFT_ERR_ALIGN;
    qeft::g_last_variant = "sqa_generic";
    return finish(qeft::sqa_generic_launch(q, k, v, k_cache_ft, v_cache, pos, alibi_slopes, out, n_heads, n_kv_heads, max_seq, head_dim,
                                           (hipStream_t)stream));
}

int qeft_single_query_attention_alibi(const void* q, const void* k, const void* v, const void* cos_tab, const void* sin_tab,
                                      int tab_rows, void* k_cache_ft, void* v_cache, const int* pos, void* out, int n_heads,
                                      int n_kv_heads, int max_seq, const float* alibi_slopes, qeft_stream_t stream) {
    if (!alibi_slopes) return QEFT_ERR_NULL;
    return sqa_impl(q, k, v, cos_tab, sin_tab, tab_rows, k_cache_ft, v_cache, pos, out, n_heads, n_kv_heads, max_seq, alibi_slopes, stream);
}

// ---- v3 decode linear (gemv_v3.h)
int qeft_decode_linear_blocks(int n_rows) {
    if (n_rows <= 0 || n_rows % 16 != 0) return 0;
    return qeft::gemv_v3_blocks(n_rows / 16);
}

// What the four qeft_decode_linear* entries ask of the operands they share, in the order of their return codes.  qweight_align:
// 16, or 4 for the 3-bit stream (qeft_decode_linear_w3: 12-byte records).
static int decode_linear_operands(const void* x, const void* qweight, uintptr_t qweight_align, const void* sz_packed, const void* oweight,
                                  const void* y, int n_out) {
    if (!x || !qweight || !sz_packed || !y || (n_out > 0 && !oweight)) return QEFT_ERR_NULL;
    if (!aligned16(x) || ((uintptr_t)qweight & (qweight_align - 1)) != 0 || !aligned16(sz_packed) || (n_out > 0 && !aligned16(oweight)))
        return QEFT_ERR_ALIGN;
    return QEFT_OK;
}

// The fused epilogue of qeft_decode_linear, _w3 and _m: the fp32 residual (y is fp32 then), the next norm's producer form
// (gamma_out, y_norm, ssq_out) and the sums of squares x was derived from.  Checked after the geometry.
static int decode_linear_epilogue(qeft::V3Args& a, int mode, void* y, const void* residual, const float* ssq_in, int n_ssq_in, float eps,
                                  const void* gamma_out, void* y_norm, float* ssq_out) {
    if ((residual || gamma_out) && mode != qeft::V3_MODE_PLAIN) return QEFT_ERR_SHAPE;
    if (gamma_out && (!residual || !y_norm || !ssq_out)) return QEFT_ERR_NULL;
    if ((residual && !aligned16(residual)) || (gamma_out && !aligned16(gamma_out))) return QEFT_ERR_ALIGN;
    if (ssq_in && (n_ssq_in < 1 || n_ssq_in > qeft::V3_MAX_SSQ)) return QEFT_ERR_SHAPE;
    a.residual = (const float*)residual;
    a.y = residual ? nullptr : (qeft::f16*)y;
    a.y32 = residual ? (float*)y : nullptr;
    a.ssq_in = ssq_in;
    a.n_ssq_in = ssq_in ? n_ssq_in : 0;
    a.eps = eps;
    a.gamma_out = (const qeft::f16*)gamma_out;
    a.ynorm = (qeft::f16*)y_norm;
    a.ssq_out = ssq_out;
    return QEFT_OK;
}

// (the differences between the four entries, and which of them a kernel needs: DESIGN.md section 9)
int qeft_decode_linear(const void* x, const void* qweight, const void* sz_packed, const void* oweight, const void* bias,
                       void* y, int n, int k, int group_size, int n_out, int mode, const void* residual,
                       const float* ssq_in, int n_ssq_in, float eps, const void* gamma_out, void* y_norm, float* ssq_out,
                       qeft_stream_t stream) {
    if (int e = decode_linear_operands(x, qweight, 16, sz_packed, oweight, y, n_out)) return e;
    qeft::V3Args a;
    if (int e = v3_args(a, x, qweight, sz_packed, oweight, bias, y, n, k, group_size, n_out, mode)) return e;
    if (int e = decode_linear_epilogue(a, mode, y, residual, ssq_in, n_ssq_in, eps, gamma_out, y_norm, ssq_out)) return e;
    if (ssq_in && !aligned16(ssq_in)) return QEFT_ERR_SHAPE;
    return finish(qeft::gemv_v3_launch(a, mode, (hipStream_t)stream));
}

int qeft_decode_linear_w3(const void* x, const void* qweight3, const void* sz_packed, const void* oweight, const void* bias,
                       void* y, int n, int k, int group_size, int n_out, int mode, const void* residual,
                       const float* ssq_in, int n_ssq_in, float eps, const void* gamma_out, void* y_norm, float* ssq_out,
                       qeft_stream_t stream) {
    if (int e = decode_linear_operands(x, qweight3, 4, sz_packed, oweight, y, n_out)) return e;
    qeft::V3Args a;
    if (int e = v3_args(a, x, qweight3, sz_packed, oweight, bias, y, n, k, group_size, n_out, mode)) return e;
    if (int e = decode_linear_epilogue(a, mode, y, residual, ssq_in, n_ssq_in, eps, gamma_out, y_norm, ssq_out)) return e;
    if (ssq_in && !aligned16(ssq_in)) return QEFT_ERR_SHAPE;
    a.bits = 3;
    return finish(qeft::gemv_v3_launch(a, mode, (hipStream_t)stream));
}

int qeft_decode_linear_hnorm(const void* h32, const void* gamma_x, const void* qweight, const void* sz_packed, const void* oweight,
                             const void* bias, void* y, int n, int k, int group_size, int n_out, int mode, float eps,
                             qeft_stream_t stream) {
    if (!gamma_x) return QEFT_ERR_NULL;
    if (int e = decode_linear_operands(h32, qweight, 16, sz_packed, oweight, y, n_out)) return e;
    if (!aligned16(gamma_x)) return QEFT_ERR_ALIGN;
    qeft::V3Args a;
    if (int e = v3_args(a, h32, qweight, sz_packed, oweight, bias, y, n, k, group_size, n_out, mode)) return e;
    a.xn_gamma = (const qeft::f16*)gamma_x;      // x is fp32 [k]: the kernel reads it as such when xn_gamma is set
    a.eps = eps;
    return finish(qeft::gemv_v3_launch(a, mode, (hipStream_t)stream));
}

long long qeft_gemv_v3_check_extents(int n, int k, int group_size, int n_out, int n_ssq_in, int shrink_rows) {
    qeft::V3Geom G{};
    if (v3_geom(G, n, k, group_size, n_out, qeft::V3_MODE_PLAIN) != QEFT_OK) return -1;
    if (n_ssq_in < 0 || n_ssq_in > qeft::V3_MAX_SSQ) return -1;
    return qeft::gemv_v3_count_out_of_range(G, n - shrink_rows, n_ssq_in, n_ssq_in == 0, 4) +
           (G.nfull > 0 ? qeft::gemv_v3_count_out_of_range(G, n - shrink_rows, n_ssq_in, false, 3) : 0);
}

long long qeft_gemv_v3_check_extents_ckpt(int n, int k, int group_size, int n_out, int m, int gather, int shrink_rows) {
    qeft::V3Geom G{};
    if (v3_geom(G, n, k, group_size, n_out, qeft::V3_MODE_PLAIN) != QEFT_OK || m < 1 || m > qeft::V3_MAX_M) return -1;
    return qeft::gemv_v3_count_out_of_range_ckpt(G, n - shrink_rows, m, gather != 0);
}

// ---- the v3 launcher's plan as integers: what it would run (no HIP call, no GPU needed), what it last ran
static_assert(QEFT_V3_F_PERCH == qeft::V3_F_PERCH && QEFT_V3_F_XN == qeft::V3_F_XN && QEFT_V3_F_SZN == qeft::V3_F_SZN &&
              QEFT_V3_F_OWIL == qeft::V3_F_OWIL && QEFT_V3_F_GATHER == qeft::V3_F_GATHER && QEFT_V3_F_XG == qeft::V3_PLAN_XG &&
              QEFT_V3_F_ENGINE_M == qeft::V3_PLAN_ENGINE_M,
              "the header's flag values are the kernel's");
static void v3_plan_out(const qeft::V3Plan& p, int* out) {
    const int v[QEFT_GEMV_V3_PLAN_INTS] = {p.nblk, p.rs_cap, p.sets_q, p.sets_r, p.nw, p.D, p.outl, p.mode, p.bits, p.fl, p.mb, p.xg, (int)p.smem};
    memcpy(out, v, sizeof(v));
}

int qeft_gemv_v3_plan(int n, int k, int group_size, int n_out, int m, int mode, int bits, int flags, int* out) {
    qeft::V3Geom G{};
    if (!out) return QEFT_ERR_NULL;
    if (v3_geom(G, n, k, group_size, n_out, mode) != QEFT_OK || m < 1 || (bits != 4 && bits != 3)) return -1;
    const uint32_t known = QEFT_V3_F_PERCH | QEFT_V3_F_XN | QEFT_V3_F_SZN | QEFT_V3_F_OWIL | QEFT_V3_F_GATHER | QEFT_V3_F_XG |
                           QEFT_V3_F_ENGINE_M;
    if (((uint32_t)flags & ~known) != 0) return -1;
    // (flags that contradict the shape: per-channel without group_size == k, an interleaved outlier slice without outliers)
    if ((((uint32_t)flags & QEFT_V3_F_PERCH) && !(G.ngroups == 1 && k > 128)) || (((uint32_t)flags & QEFT_V3_F_OWIL) && n_out == 0)) return -1;
    const qeft::V3Plan p = qeft::gemv_v3_plan(G, m, mode, bits, (uint32_t)flags);
    if (!p.ok) return -1;
    v3_plan_out(p, out);
    return QEFT_OK;
}

int qeft_gemv_v3_last_plan(int* out) {
    if (!out) return QEFT_ERR_NULL;
    v3_plan_out(qeft::gemv_v3_last_plan(), out);
    return QEFT_OK;
}

int qeft_gemv_v3_plan_kct(int n, int k, int group_size, int n_out, int m, int mode, int bits, int flags) {
    int out[QEFT_GEMV_V3_PLAN_INTS];
    if (qeft_gemv_v3_plan(n, k, group_size, n_out, m, mode, bits, flags, out) != QEFT_OK) return -1;
    qeft::V3Geom G{};
    v3_geom(G, n, k, group_size, n_out, mode);
    return qeft::gemv_v3_plan(G, m, mode, bits, (uint32_t)flags).kct;
}

int qeft_gemv_v3_last_kct(void) { return qeft::gemv_v3_last_plan().kct; }

int qeft_token_begin_norm_blocks(int hidden) { return hidden >= 8 ? qeft::token_begin_norm_blocks(hidden) : 0; }

int qeft_token_begin_norm(const void* embed, const void* tok, const void* rope_tab, const int* pos, void* h, void* rope_row,
                          const void* gamma, void* h_norm, float* ssq_out, int hidden, int vocab, int max_seq,
                          qeft_stream_t stream) {
    if (hidden < 8 || hidden % 8 != 0 || vocab < 1 || max_seq < 1) return QEFT_ERR_SHAPE;
    if (!embed || !tok || !h || !gamma || !h_norm || !ssq_out || (rope_row && (!rope_tab || !pos))) return QEFT_ERR_NULL;
    if (!aligned16(embed) || !aligned16(h) || !aligned16(gamma) || !aligned16(h_norm)) return QEFT_ERR_ALIGN;
    return finish(qeft::token_begin_norm_launch(embed, tok, rope_tab, pos, h, rope_row, gamma, h_norm, ssq_out, hidden, vocab,
                                                max_seq, (hipStream_t)stream));
}

int qeft_residual_norm(const void* h, const void* add, const void* gamma, void* h_out, void* h_norm, float* ssq_out,
                       int hidden, qeft_stream_t stream) {
    if (hidden < 8 || hidden % 8 != 0) return QEFT_ERR_SHAPE;
    if (!h || !h_out) return QEFT_ERR_NULL;
    if (gamma && (!h_norm || !ssq_out)) return QEFT_ERR_NULL;
    if (!aligned16(h) || !aligned16(h_out) || (add && !aligned16(add)) || (gamma && (!aligned16(gamma) || !aligned16(h_norm))))
        return QEFT_ERR_ALIGN;
    return finish(qeft::residual_norm_launch(h, add, gamma, h_out, h_norm, ssq_out, hidden, (hipStream_t)stream));
}

int qeft_token_begin(const void* embed, const void* tok, const void* rope_tab, const int* pos, void* h, void* rope_row,
                     int hidden, int vocab, int max_seq, qeft_stream_t stream) {
    if (hidden < 8 || hidden % 8 != 0 || vocab < 1 || max_seq < 1) return QEFT_ERR_SHAPE;
    if (!embed || !tok || !h || (rope_row && (!rope_tab || !pos))) return QEFT_ERR_NULL;
    if (!aligned16(embed) || !aligned16(h)) return QEFT_ERR_ALIGN;
    return finish(qeft::token_begin_launch(embed, tok, rope_tab, pos, h, rope_row, hidden, vocab, max_seq, (hipStream_t)stream));
}

int qeft_token_end(const void* logits, void* tok, int* pos, int vocab, int greedy, qeft_stream_t stream) {
    if (vocab < 1) return QEFT_ERR_SHAPE;
    if (!pos || (greedy && (!logits || !tok))) return QEFT_ERR_NULL;
    if (greedy && !aligned16(logits)) return QEFT_ERR_ALIGN;
    return finish(qeft::token_end_launch(logits, tok, pos, vocab, greedy, (hipStream_t)stream));
}

// ---- verify pass (m = 1..8 rows of one sequence): gemv_v3_multi.hip, decode_verify.hip
static bool verify_m_ok(int m) { return m >= 1 && m <= 8; }

int qeft_decode_linear_m(const void* x, const void* qweight, const void* sz_packed, const void* oweight, const void* bias,
                         void* y, int n, int k, int group_size, int n_out, int mode, const void* residual,
                         const float* ssq_in, int n_ssq_in, float eps, const void* gamma_out, void* y_norm, float* ssq_out,
                         int m, qeft_stream_t stream) {
    if (!verify_m_ok(m)) return QEFT_ERR_BATCH;
    if (m == 1)
        return qeft_decode_linear(x, qweight, sz_packed, oweight, bias, y, n, k, group_size, n_out, mode, residual, ssq_in, n_ssq_in,
                                  eps, gamma_out, y_norm, ssq_out, stream);
    if (int e = decode_linear_operands(x, qweight, 16, sz_packed, oweight, y, n_out)) return e;
    qeft::V3Args a;
    if (int e = v3_args(a, x, qweight, sz_packed, oweight, bias, y, n, k, group_size, n_out, mode)) return e;
    if (a.g.ngroups == 1 && k > 128) return QEFT_ERR_GROUP;            // per-channel scales: not an engine operand
    if (int e = decode_linear_epilogue(a, mode, y, residual, ssq_in, n_ssq_in, eps, gamma_out, y_norm, ssq_out)) return e;
    a.m = m;                                                           // (ssq_in [m][n_ssq_in]: no alignment asked)
    hipError_t e = qeft::gemv_v3_multi_launch(a, mode, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) return QEFT_ERR_SHAPE;
    return finish(e);
}

long long qeft_gemv_v3_check_extents_m(int n, int k, int group_size, int n_out, int m, int mode, int n_ssq_in, int shrink_rows) {
    qeft::V3Geom G{};
    if (!verify_m_ok(m) || v3_geom(G, n, k, group_size, n_out, mode) != QEFT_OK) return -1;
    if (G.ngroups == 1 && k > 128) return -1;
    if (n_ssq_in < 0 || n_ssq_in > qeft::V3_MAX_SSQ || shrink_rows < 0 || shrink_rows % 16 != 0 || shrink_rows >= n) return -1;
    // the one-row launch's accesses (weights, scales, outliers: the same for every m) + the m-row ones
    return qeft::gemv_v3_count_out_of_range(G, n - shrink_rows, 0, false, 4) +
           qeft::gemv_v3_count_out_of_range_multi(G, n - shrink_rows, m, mode, n_ssq_in);
}

int qeft_token_begin_norm_m(const void* embed, const void* tokens, const void* rope_tab, const int* pos, void* h, void* rope_rows,
                            const void* gamma, void* h_norm, float* ssq_out, int hidden, int vocab, int max_seq, int m,
                            qeft_stream_t stream) {
    if (!verify_m_ok(m)) return QEFT_ERR_BATCH;
    if (hidden < 8 || hidden % 8 != 0 || vocab < 1 || max_seq < 1) return QEFT_ERR_SHAPE;
    if (!embed || !tokens || !rope_tab || !pos || !h || !rope_rows || !gamma || !h_norm || !ssq_out) return QEFT_ERR_NULL;
    if (!aligned16(embed) || !aligned16(h) || !aligned16(gamma) || !aligned16(h_norm)) return QEFT_ERR_ALIGN;
    return finish(qeft::token_begin_norm_m_launch(embed, tokens, rope_tab, pos, h, rope_rows, gamma, h_norm, ssq_out, hidden, vocab,
                                                  max_seq, m, (hipStream_t)stream));
}

// ---- row-wise attention (m rows of one sequence: decode_verify.hip, decode_verify_kv8.hip; one row each of m sequences:
// decode_batch.hip, decode_attn_kv8.hip).  The entries name their operands in an AttnRowsArgs (decode_rows.h), attn_rows_check
// holds what they all ask of them, in the order of their return codes.  slots: rows of different sequences (slot_tab,
// n_slots); scales: an e4m3 cache (ks, vs: fp32, 4-byte aligned).
static int attn_rows_check(const qeft::AttnRowsArgs& a, bool slots, bool scales) {
    if (!verify_m_ok(a.m)) return QEFT_ERR_BATCH;
    if (a.n_heads < 1 || a.n_kv < 1 || a.n_heads % a.n_kv != 0 || a.n_heads > 4096 || a.max_seq < 16 || a.max_seq % 16 != 0 ||
        a.max_seq > 32768 || (slots && (a.n_slots < 1 || a.n_slots > 4096)))
        return QEFT_ERR_SHAPE;
    if (a.tab_rows != a.m && a.tab_rows < a.max_seq) return QEFT_ERR_SHAPE;
    if (a.tab_stride < 64 || a.qkv_stride < 1 || a.out_stride < 1 || (!a.out_pos && a.out_stride < a.n_heads * 128)) return QEFT_ERR_SHAPE;
    if (a.S != 1 && a.S != 2 && a.S != 4 && a.S != 8) return QEFT_ERR_SHAPE;
    if (!a.q || !a.k || !a.v || !a.cs || !a.sn || !a.kc || !a.vc || (scales && (!a.ks || !a.vs)) || (slots && !a.slot_tab) || !a.pos ||
        !a.out)
        return QEFT_ERR_NULL;
    if (a.S > 1 && !a.ws) return QEFT_ERR_NULL;
    if (!aligned16(a.kc) || !aligned16(a.vc) || !aligned16(a.ws) || (scales && (((uintptr_t)a.ks & 3) || ((uintptr_t)a.vs & 3))))
        return QEFT_ERR_ALIGN;
    return QEFT_OK;
}

// the guard of the four workspace queries: 0 for what the launch entries refuse
static int attn_rows_workspace(size_t (*bytes)(int, int, int), int n_heads, int n_split, int m) {
    if (n_heads < 1 || n_heads > 4096 || n_split < 1 || n_split > 8 || !verify_m_ok(m)) return 0;
    return (int)bytes(n_heads, n_split, m);
}

int qeft_attn_m_workspace_bytes(int n_heads, int n_split, int m) {
    return attn_rows_workspace(qeft::attn_m_workspace_bytes, n_heads, n_split, m);
}

int qeft_rope_attn_decode_m(const void* q, const void* k, const void* v, int qkv_stride, const void* cos_tab, const void* sin_tab,
                            int tab_stride, int tab_rows, void* k_cache, void* v_cache, const int* pos, const int* out_pos,
                            void* out, int out_stride, void* workspace, int n_split, int n_heads, int n_kv_heads, int max_seq,
                            int m, qeft_stream_t stream) {
    qeft::AttnRowsArgs a{};
    a.q = q, a.k = k, a.v = v, a.qkv_stride = qkv_stride;
    a.cs = cos_tab, a.sn = sin_tab, a.tab_stride = tab_stride, a.tab_rows = tab_rows;
    a.kc = k_cache, a.vc = v_cache;
    a.pos = pos, a.out_pos = out_pos, a.out = out, a.out_stride = out_stride, a.ws = workspace;
    a.S = n_split, a.n_heads = n_heads, a.n_kv = n_kv_heads, a.max_seq = max_seq, a.m = m;
    if (int e = attn_rows_check(a, false, false)) return e;
    return finish(qeft::rope_attn_m_launch(a, (hipStream_t)stream));
}

int qeft_lm_head_f16_m(const void* h32, const void* gamma, const void* weight, void* logits, int hidden, int vocab, float eps,
                       int m, qeft_stream_t stream) {
    if (!verify_m_ok(m)) return QEFT_ERR_BATCH;
    if (vocab < 1 || hidden < 512 || hidden % 512 != 0) return QEFT_ERR_SHAPE;
    if (!h32 || !gamma || !weight || !logits) return QEFT_ERR_NULL;
    if (!aligned16(h32) || !aligned16(gamma) || !aligned16(weight)) return QEFT_ERR_ALIGN;
    hipError_t e = qeft::lm_head_m_launch(h32, gamma, weight, logits, hidden, vocab, eps, m, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) return QEFT_ERR_SHAPE;
    return finish(e);
}

int qeft_verify_greedy(const void* logits, const void* tokens, int m, int vocab, int greedy, void* out_tokens, int* n_accepted,
                       void* tok, int* pos, qeft_stream_t stream) {
    if (!verify_m_ok(m)) return QEFT_ERR_BATCH;
    if (vocab < 1) return QEFT_ERR_SHAPE;
    if (!pos || (greedy && (!logits || !tokens || !out_tokens || !n_accepted || !tok))) return QEFT_ERR_NULL;
    if (greedy && !aligned16(logits)) return QEFT_ERR_ALIGN;
    return finish(qeft::verify_greedy_launch(logits, tokens, m, vocab, greedy, out_tokens, n_accepted, tok, pos, (hipStream_t)stream));
}

// ---- batched decoding (m = 1..8 rows of m different sequences, row r in cache slot slots[r]): decode_batch.hip
int qeft_token_begin_norm_batch(const void* embed, const void* tokens, const void* rope_tab, const int* slots, const int* pos, void* h,
                                void* rope_rows, const void* gamma, void* h_norm, float* ssq_out, int hidden, int vocab, int max_seq,
                                int n_slots, int m, qeft_stream_t stream) {
    if (!verify_m_ok(m)) return QEFT_ERR_BATCH;
    if (hidden < 8 || hidden % 8 != 0 || vocab < 1 || max_seq < 1 || n_slots < 1) return QEFT_ERR_SHAPE;
    if (!embed || !tokens || !rope_tab || !slots || !pos || !h || !rope_rows || !gamma || !h_norm || !ssq_out) return QEFT_ERR_NULL;
    if (!aligned16(embed) || !aligned16(h) || !aligned16(gamma) || !aligned16(h_norm)) return QEFT_ERR_ALIGN;
    return finish(qeft::token_begin_norm_b_launch(embed, tokens, rope_tab, slots, pos, h, rope_rows, gamma, h_norm, ssq_out, hidden,
                                                  vocab, max_seq, n_slots, m, (hipStream_t)stream));
}

int qeft_attn_batch_workspace_bytes(int n_heads, int n_split, int m) {
    return attn_rows_workspace(qeft::attn_b_workspace_bytes, n_heads, n_split, m);
}

int qeft_rope_attn_decode_batch(const void* q, const void* k, const void* v, int qkv_stride, const void* cos_tab, const void* sin_tab,
                                int tab_stride, int tab_rows, void* k_cache, void* v_cache, const int* slots, const int* pos,
                                const int* done, const int* out_pos, void* out, int out_stride, void* workspace, int n_split,
                                int n_slots, int n_heads, int n_kv_heads, int max_seq, int m, qeft_stream_t stream) {
    qeft::AttnRowsArgs a{};
    a.q = q, a.k = k, a.v = v, a.qkv_stride = qkv_stride;
    a.cs = cos_tab, a.sn = sin_tab, a.tab_stride = tab_stride, a.tab_rows = tab_rows;
    a.kc = k_cache, a.vc = v_cache;
    a.slot_tab = slots, a.pos = pos, a.done = done, a.n_slots = n_slots;
    a.out_pos = out_pos, a.out = out, a.out_stride = out_stride, a.ws = workspace;
    a.S = n_split, a.n_heads = n_heads, a.n_kv = n_kv_heads, a.max_seq = max_seq, a.m = m;
    if (int e = attn_rows_check(a, true, false)) return e;
    return finish(qeft::rope_attn_b_launch(a, (hipStream_t)stream));
}

int qeft_token_end_batch(const void* logits, const int* slots, void* tokens, int* pos, const int* limit, const int* eos, int* done,
                         void* out, int* counter, int vocab, int out_cap, int n_slots, int m, qeft_stream_t stream) {
    if (!verify_m_ok(m)) return QEFT_ERR_BATCH;
    if (vocab < 1 || out_cap < 1 || n_slots < 1) return QEFT_ERR_SHAPE;
    if (!logits || !slots || !tokens || !pos || !limit || !eos || !done || !out || !counter) return QEFT_ERR_NULL;
    if (!aligned16(logits)) return QEFT_ERR_ALIGN;
    return finish(qeft::token_end_b_launch(logits, slots, tokens, pos, limit, eos, done, out, counter, vocab, out_cap, n_slots, m,
                                           (hipStream_t)stream));
}

// ---- e4m3 KV cache (decode_attn_kv8.hip)
int qeft_attn_kv8_workspace_bytes(int n_heads, int n_split, int m) {
    return attn_rows_workspace(qeft::attn_kv8_workspace_bytes, n_heads, n_split, m);
}

int qeft_rope_attn_decode_kv8(const void* q, const void* k, const void* v, int qkv_stride, const void* cos_tab, const void* sin_tab,
                              int tab_stride, int tab_rows, void* k_codes, void* v_codes, void* k_scales, void* v_scales,
                              const int* slots, const int* pos, const int* done, const int* out_pos, void* out, int out_stride,
                              void* workspace, int n_split, int n_slots, int n_heads, int n_kv_heads, int max_seq, int m,
                              qeft_stream_t stream) {
    qeft::AttnRowsArgs a{};
    a.q = q, a.k = k, a.v = v, a.qkv_stride = qkv_stride;
    a.cs = cos_tab, a.sn = sin_tab, a.tab_stride = tab_stride, a.tab_rows = tab_rows;
    a.kc = k_codes, a.vc = v_codes, a.ks = k_scales, a.vs = v_scales;
    a.slot_tab = slots, a.pos = pos, a.done = done, a.n_slots = n_slots;
    a.out_pos = out_pos, a.out = out, a.out_stride = out_stride, a.ws = workspace;
    a.S = n_split, a.n_heads = n_heads, a.n_kv = n_kv_heads, a.max_seq = max_seq, a.m = m;
    if (int e = attn_rows_check(a, true, true)) return e;
    return finish(qeft::rope_attn_kv8_launch(a, (hipStream_t)stream));
}

int qeft_kv8_store_rows(const void* k_rows, const void* v_rows, int row_stride, void* k_codes, void* v_codes, void* k_scales,
                        void* v_scales, int n_kv_heads, int max_seq, int p0, int n_rows, qeft_stream_t stream) {
    if (n_kv_heads < 1 || n_kv_heads > 4096 || max_seq < 16 || max_seq % 16 != 0 || max_seq > 32768) return QEFT_ERR_SHAPE;
    if (n_rows < 1 || p0 < 0 || p0 > max_seq || n_rows > max_seq - p0 || row_stride < n_kv_heads * 128) return QEFT_ERR_SHAPE;
    if (!k_rows || !v_rows || !k_codes || !v_codes || !k_scales || !v_scales) return QEFT_ERR_NULL;
    if (((uintptr_t)k_rows & 1) || ((uintptr_t)v_rows & 1) || ((uintptr_t)k_scales & 3) || ((uintptr_t)v_scales & 3)) return QEFT_ERR_ALIGN;
    return finish(qeft::kv8_store_rows_launch(k_rows, v_rows, row_stride, k_codes, v_codes, k_scales, v_scales, n_kv_heads, max_seq, p0,
                                              n_rows, (hipStream_t)stream));
}

// ---- the verify pass over an e4m3 KV cache (decode_verify_kv8.hip)
int qeft_attn_m_kv8_workspace_bytes(int n_heads, int n_split, int m) {
    return attn_rows_workspace(qeft::attn_m_workspace_bytes, n_heads, n_split, m);      // one layout of counters and records with the fp16 kernel
}

int qeft_rope_attn_decode_m_kv8(const void* q, const void* k, const void* v, int qkv_stride, const void* cos_tab, const void* sin_tab,
                                int tab_stride, int tab_rows, void* k_codes, void* v_codes, void* k_scales, void* v_scales,
                                const int* pos, const int* out_pos, void* out, int out_stride, void* workspace, int n_split,
                                int n_heads, int n_kv_heads, int max_seq, int m, qeft_stream_t stream) {
    qeft::AttnRowsArgs a{};
    a.q = q, a.k = k, a.v = v, a.qkv_stride = qkv_stride;
    a.cs = cos_tab, a.sn = sin_tab, a.tab_stride = tab_stride, a.tab_rows = tab_rows;
    a.kc = k_codes, a.vc = v_codes, a.ks = k_scales, a.vs = v_scales;
    a.pos = pos, a.out_pos = out_pos, a.out = out, a.out_stride = out_stride, a.ws = workspace;
    a.S = n_split, a.n_heads = n_heads, a.n_kv = n_kv_heads, a.max_seq = max_seq, a.m = m;
    if (int e = attn_rows_check(a, false, true)) return e;
    return finish(qeft::rope_attn_m_kv8_launch(a, (hipStream_t)stream));
}

// ---- prompt attention over the cache (prefill_attn.hip)
static int prefill_geom(qeft::PaGeom& G, int q_stride, int kv_rows, int out_stride, int start, int t, int n_heads, int n_kv_heads) {
    if (t < 1 || start < 0 || kv_rows < 1 || start > kv_rows || t > kv_rows - start) return QEFT_ERR_SHAPE;
    if (n_heads < 1 || n_kv_heads < 1 || n_heads > 4096 || n_heads % n_kv_heads != 0) return QEFT_ERR_SHAPE;
    if (q_stride % 8 != 0 || q_stride < n_heads * 128 || out_stride % 8 != 0 || out_stride < n_heads * 128) return QEFT_ERR_SHAPE;
    if (kv_rows > (1 << 24) || (long long)t * q_stride > (1ll << 40)) return QEFT_ERR_SHAPE;
    G = qeft::PaGeom{q_stride, kv_rows, out_stride, start, t, n_heads, n_kv_heads};
    return QEFT_OK;
}

int qeft_attn_prefill(const void* q, int q_stride, const void* k_cache, const void* v_cache, int kv_rows, void* out, int out_stride,
                      int start, int t, int n_heads, int n_kv_heads, qeft_stream_t stream) {
    qeft::PaGeom G{};
    if (int e = prefill_geom(G, q_stride, kv_rows, out_stride, start, t, n_heads, n_kv_heads)) return e;
    if (!q || !k_cache || !v_cache || !out) return QEFT_ERR_NULL;
    if (!aligned16(q) || !aligned16(k_cache) || !aligned16(v_cache) || !aligned16(out)) return QEFT_ERR_ALIGN;
    return finish(qeft::prefill_attn_launch(q, k_cache, v_cache, out, G, (hipStream_t)stream));
}

long long qeft_attn_prefill_check_extents(int q_stride, int kv_rows, int out_stride, int start, int t, int n_heads, int n_kv_heads) {
    qeft::PaGeom G{};
    if (prefill_geom(G, q_stride, kv_rows, out_stride, start, t, n_heads, n_kv_heads) != QEFT_OK) return -1;
    return qeft::prefill_attn_count_out_of_range(G);
}

// ---- prompt attention with the past in an e4m3 cache (prefill_attn_kv8.hip)
static int prefill_kv8_geom(qeft::Pa8Geom& G8, int q_stride, int kv_rows, int new_stride, int out_stride, int start, int t, int n_heads,
                            int n_kv_heads) {
    if (int e = prefill_geom(G8.g, q_stride, kv_rows, out_stride, start, t, n_heads, n_kv_heads)) return e;
    if (new_stride % 8 != 0 || new_stride < n_kv_heads * 128 || (long long)t * new_stride > (1ll << 40)) return QEFT_ERR_SHAPE;
    G8.new_stride = new_stride;
    return QEFT_OK;
}

int qeft_attn_prefill_kv8(const void* q, int q_stride, const void* k_codes, const void* v_codes, const void* k_scales,
                          const void* v_scales, int kv_rows, const void* k_new, const void* v_new, int new_stride, void* out,
                          int out_stride, int start, int t, int n_heads, int n_kv_heads, qeft_stream_t stream) {
    qeft::Pa8Geom G8{};
    if (int e = prefill_kv8_geom(G8, q_stride, kv_rows, new_stride, out_stride, start, t, n_heads, n_kv_heads)) return e;
    if (!q || !k_codes || !v_codes || !k_scales || !v_scales || !k_new || !v_new || !out) return QEFT_ERR_NULL;
    if (!aligned16(q) || !aligned16(k_codes) || !aligned16(v_codes) || !aligned16(k_new) || !aligned16(v_new) || !aligned16(out) ||
        ((uintptr_t)k_scales & 3) || ((uintptr_t)v_scales & 3))
        return QEFT_ERR_ALIGN;
    return finish(qeft::prefill_attn_kv8_launch(q, k_codes, v_codes, k_scales, v_scales, k_new, v_new, out, G8, (hipStream_t)stream));
}

long long qeft_attn_prefill_kv8_check_extents(int q_stride, int kv_rows, int new_stride, int out_stride, int start, int t, int n_heads,
                                              int n_kv_heads) {
    qeft::Pa8Geom G8{};
    if (prefill_kv8_geom(G8, q_stride, kv_rows, new_stride, out_stride, start, t, n_heads, n_kv_heads) != QEFT_OK) return -1;
    return qeft::prefill_attn_kv8_count_out_of_range(G8);
}

// ---- training attention (attn_train.hip)
static bool attn_train_stride_ok(int stride, int width) { return stride % 8 == 0 && stride >= width && stride <= (1 << 24); }

static int attn_train_geom(qeft::AtGeom& A, int q_stride, int kv_stride, int out_stride, int n_seq, int t, int n_heads, int n_kv_heads) {
    if (t < 1 || n_seq < 1 || (long long)n_seq * t > (1ll << 20)) return QEFT_ERR_SHAPE;
    if (n_heads < 1 || n_kv_heads < 1 || n_heads > 4096 || n_heads % n_kv_heads != 0) return QEFT_ERR_SHAPE;
    if (!attn_train_stride_ok(q_stride, n_heads * 128) || !attn_train_stride_ok(out_stride, n_heads * 128) ||
        !attn_train_stride_ok(kv_stride, n_kv_heads * 128))
        return QEFT_ERR_SHAPE;
    A = qeft::AtGeom{};
    A.f.g = qeft::PaGeom{q_stride, t, out_stride, 0, t, n_heads, n_kv_heads};
    A.f.new_stride = kv_stride;
    A.dout_stride = A.dq_stride = n_heads * 128;
    A.dkv_stride = n_kv_heads * 128;
    A.n_seq = n_seq;
    if (qeft::at_q_blocks(A) >= (1ll << 31) || qeft::at_delta_blocks(A) >= (1ll << 31)) return QEFT_ERR_SHAPE;      // the grids
    return QEFT_OK;
}

static int attn_train_bwd_geom(qeft::AtGeom& A, int q_stride, int kv_stride, int out_stride, int dout_stride, int dq_stride,
                               int dkv_stride, int n_seq, int t, int n_heads, int n_kv_heads) {
    if (int e = attn_train_geom(A, q_stride, kv_stride, out_stride, n_seq, t, n_heads, n_kv_heads)) return e;
    if (!attn_train_stride_ok(dout_stride, n_heads * 128) || !attn_train_stride_ok(dq_stride, n_heads * 128) ||
        !attn_train_stride_ok(dkv_stride, n_kv_heads * 128))
        return QEFT_ERR_SHAPE;
    A.dout_stride = dout_stride;
    A.dq_stride = dq_stride;
    A.dkv_stride = dkv_stride;
    return QEFT_OK;
}

int qeft_attn_train_fwd(const void* q, int q_stride, const void* k, const void* v, int kv_stride, void* out, int out_stride, float* lse,
                        int n_seq, int t, int n_heads, int n_kv_heads, qeft_stream_t stream) {
    qeft::AtGeom A{};
    if (int e = attn_train_geom(A, q_stride, kv_stride, out_stride, n_seq, t, n_heads, n_kv_heads)) return e;
    if (!q || !k || !v || !out || !lse) return QEFT_ERR_NULL;
    if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(out) || ((uintptr_t)lse & 3)) return QEFT_ERR_ALIGN;
    return finish(qeft::attn_train_fwd_launch(q, k, v, out, lse, A, (hipStream_t)stream));
}

long long qeft_attn_train_check_extents(int q_stride, int kv_stride, int out_stride, int n_seq, int t, int n_heads, int n_kv_heads) {
    qeft::AtGeom A{};
    if (attn_train_geom(A, q_stride, kv_stride, out_stride, n_seq, t, n_heads, n_kv_heads) != QEFT_OK) return -1;
    return qeft::attn_train_fwd_count_out_of_range(A);
}

long long qeft_attn_train_bwd_workspace_bytes(int n_seq, int t, int n_heads, int n_kv_heads) {
    qeft::AtGeom A{};
    if (n_heads < 1 || n_kv_heads < 1 || n_heads > 4096) return 0;
    if (attn_train_geom(A, n_heads * 128, n_kv_heads * 128, n_heads * 128, n_seq, t, n_heads, n_kv_heads) != QEFT_OK) return 0;
    return 4ll * n_seq * t * n_heads;                                  // delta, fp32 [n_seq t][n_heads]
}

static int attn_train_bwd_entry(const void* q, int q_stride, const void* k, const void* v, int kv_stride, const void* out,
                                int out_stride, const void* dout, int dout_stride, const float* lse, void* dq, int dq_stride, void* dk,
                                void* dv, int dkv_stride, void* workspace, long long workspace_bytes, int n_seq, int t, int n_heads,
                                int n_kv_heads, int parts, qeft_stream_t stream) {
    qeft::AtGeom A{};
    if (int e = attn_train_bwd_geom(A, q_stride, kv_stride, out_stride, dout_stride, dq_stride, dkv_stride, n_seq, t, n_heads,
                                    n_kv_heads))
        return e;
    if (workspace_bytes < 4ll * n_seq * t * n_heads) return QEFT_ERR_SHAPE;
    if (!q || !k || !v || !out || !dout || !lse || !dq || !dk || !dv || !workspace) return QEFT_ERR_NULL;
    if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(out) || !aligned16(dout) || !aligned16(dq) || !aligned16(dk) ||
        !aligned16(dv) || !aligned16(workspace) || ((uintptr_t)lse & 3))
        return QEFT_ERR_ALIGN;
    return finish(qeft::attn_train_bwd_launch(q, k, v, out, dout, lse, dq, dk, dv, (float*)workspace, A, parts, (hipStream_t)stream));
}

int qeft_attn_train_bwd(const void* q, int q_stride, const void* k, const void* v, int kv_stride, const void* out, int out_stride,
                        const void* dout, int dout_stride, const float* lse, void* dq, int dq_stride, void* dk, void* dv,
                        int dkv_stride, void* workspace, long long workspace_bytes, int n_seq, int t, int n_heads, int n_kv_heads,
                        qeft_stream_t stream) {
    return attn_train_bwd_entry(q, q_stride, k, v, kv_stride, out, out_stride, dout, dout_stride, lse, dq, dq_stride, dk, dv, dkv_stride,
                                workspace, workspace_bytes, n_seq, t, n_heads, n_kv_heads, 7, stream);
}

int qeft_attn_train_bwd_part(const void* q, int q_stride, const void* k, const void* v, int kv_stride, const void* out, int out_stride,
                             const void* dout, int dout_stride, const float* lse, void* dq, int dq_stride, void* dk, void* dv,
                             int dkv_stride, void* workspace, long long workspace_bytes, int n_seq, int t, int n_heads, int n_kv_heads,
                             int part, qeft_stream_t stream) {
    if (part < 0 || part > 2) return QEFT_ERR_SHAPE;
    return attn_train_bwd_entry(q, q_stride, k, v, kv_stride, out, out_stride, dout, dout_stride, lse, dq, dq_stride, dk, dv, dkv_stride,
                                workspace, workspace_bytes, n_seq, t, n_heads, n_kv_heads, 1 << part, stream);
}

long long qeft_attn_train_bwd_check_extents(int q_stride, int kv_stride, int out_stride, int dout_stride, int dq_stride, int dkv_stride,
                                            int n_seq, int t, int n_heads, int n_kv_heads) {
    qeft::AtGeom A{};
    if (attn_train_bwd_geom(A, q_stride, kv_stride, out_stride, dout_stride, dq_stride, dkv_stride, n_seq, t, n_heads, n_kv_heads) !=
        QEFT_OK)
        return -1;
    return qeft::attn_train_bwd_count_out_of_range(A);
}

// ---- training attention over packed sequences (attn_train.hip, the varlen launches).  seq_rows is a HOST array, the n_seq + 1
// prefix of the lengths; it is copied into the launch's arguments here, so what is validated is what the kernels read.
// Order: the scalars (QEFT_ERR_SHAPE), seq_rows itself (QEFT_ERR_NULL), its contents (QEFT_ERR_SHAPE); the entries go on with
// the workspace size, then NULL, then alignment of the device operands.
static int attn_train_varlen_geom(qeft::AtVarGeom& V, int q_stride, int kv_stride, int out_stride, int dout_stride, int dq_stride,
                                  int dkv_stride, const int* seq_rows, int n_seq, int n_heads, int n_kv_heads) {
    if (n_seq < 1 || n_seq > qeft::AT_MAX_SEQ) return QEFT_ERR_SHAPE;
    V = qeft::AtVarGeom{};
    if (int e = attn_train_bwd_geom(V.a, q_stride, kv_stride, out_stride, dout_stride, dq_stride, dkv_stride, 1, 1, n_heads, n_kv_heads))
        return e;
    if (!seq_rows) return QEFT_ERR_NULL;
    if (seq_rows[0] != 0) return QEFT_ERR_SHAPE;
    int longest = 0;
    for (int i = 0; i < n_seq; ++i) {
        if (seq_rows[i + 1] <= seq_rows[i] || seq_rows[i + 1] > (1 << 20)) return QEFT_ERR_SHAPE;       // len >= 1, R <= 2^20
        if (seq_rows[i + 1] - seq_rows[i] > longest) longest = seq_rows[i + 1] - seq_rows[i];
    }
    for (int i = 0; i <= n_seq; ++i) V.cu[i] = seq_rows[i];
    V.a.f.g.t = V.a.f.g.kv_rows = longest;
    V.a.n_seq = n_seq;
    return QEFT_OK;
}

static int attn_train_varlen_fwd_geom(qeft::AtVarGeom& V, int q_stride, int kv_stride, int out_stride, const int* seq_rows, int n_seq,
                                      int n_heads, int n_kv_heads) {
    if (n_heads < 1 || n_kv_heads < 1 || n_heads > 4096) return QEFT_ERR_SHAPE;     // before they size the gradients' default strides
    return attn_train_varlen_geom(V, q_stride, kv_stride, out_stride, n_heads * 128, n_heads * 128, n_kv_heads * 128, seq_rows, n_seq,
                                  n_heads, n_kv_heads);
}

int qeft_attn_train_varlen_fwd(const void* q, int q_stride, const void* k, const void* v, int kv_stride, void* out, int out_stride,
                               float* lse, const int* seq_rows, int n_seq, int n_heads, int n_kv_heads, qeft_stream_t stream) {
    qeft::AtVarGeom V;
    if (int e = attn_train_varlen_fwd_geom(V, q_stride, kv_stride, out_stride, seq_rows, n_seq, n_heads, n_kv_heads)) return e;
    if (!q || !k || !v || !out || !lse) return QEFT_ERR_NULL;
    if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(out) || ((uintptr_t)lse & 3)) return QEFT_ERR_ALIGN;
    return finish(qeft::attn_train_varlen_fwd_launch(q, k, v, out, lse, V, (hipStream_t)stream));
}

long long qeft_attn_train_varlen_check_extents(int q_stride, int kv_stride, int out_stride, const int* seq_rows, int n_seq, int n_heads,
                                               int n_kv_heads) {
    qeft::AtVarGeom V;
    if (attn_train_varlen_fwd_geom(V, q_stride, kv_stride, out_stride, seq_rows, n_seq, n_heads, n_kv_heads) != QEFT_OK) return -1;
    return qeft::attn_train_varlen_fwd_count_out_of_range(V);
}

long long qeft_attn_train_varlen_bwd_workspace_bytes(const int* seq_rows, int n_seq, int n_heads, int n_kv_heads) {
    qeft::AtVarGeom V;
    if (n_heads < 1 || n_kv_heads < 1 || n_heads > 4096) return 0;
    if (attn_train_varlen_fwd_geom(V, n_heads * 128, n_kv_heads * 128, n_heads * 128, seq_rows, n_seq, n_heads, n_kv_heads) != QEFT_OK)
        return 0;
    return 4ll * qeft::at_var_rows(V) * n_heads;                       // delta, fp32 [R][n_heads]
}

static int attn_train_varlen_bwd_entry(const void* q, int q_stride, const void* k, const void* v, int kv_stride, const void* out,
                                       int out_stride, const void* dout, int dout_stride, const float* lse, void* dq, int dq_stride,
                                       void* dk, void* dv, int dkv_stride, void* workspace, long long workspace_bytes,
                                       const int* seq_rows, int n_seq, int n_heads, int n_kv_heads, int parts, qeft_stream_t stream) {
    qeft::AtVarGeom V;
    if (int e = attn_train_varlen_geom(V, q_stride, kv_stride, out_stride, dout_stride, dq_stride, dkv_stride, seq_rows, n_seq, n_heads,
                                       n_kv_heads))
        return e;
    if (workspace_bytes < 4ll * qeft::at_var_rows(V) * n_heads) return QEFT_ERR_SHAPE;
    if (!q || !k || !v || !out || !dout || !lse || !dq || !dk || !dv || !workspace) return QEFT_ERR_NULL;
    if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(out) || !aligned16(dout) || !aligned16(dq) || !aligned16(dk) ||
        !aligned16(dv) || !aligned16(workspace) || ((uintptr_t)lse & 3))
        return QEFT_ERR_ALIGN;
    return finish(qeft::attn_train_varlen_bwd_launch(q, k, v, out, dout, lse, dq, dk, dv, (float*)workspace, V, parts,
                                                     (hipStream_t)stream));
}

int qeft_attn_train_varlen_bwd(const void* q, int q_stride, const void* k, const void* v, int kv_stride, const void* out, int out_stride,
                               const void* dout, int dout_stride, const float* lse, void* dq, int dq_stride, void* dk, void* dv,
                               int dkv_stride, void* workspace, long long workspace_bytes, const int* seq_rows, int n_seq, int n_heads,
                               int n_kv_heads, qeft_stream_t stream) {
    return attn_train_varlen_bwd_entry(q, q_stride, k, v, kv_stride, out, out_stride, dout, dout_stride, lse, dq, dq_stride, dk, dv,
                                       dkv_stride, workspace, workspace_bytes, seq_rows, n_seq, n_heads, n_kv_heads, 7, stream);
}

int qeft_attn_train_varlen_bwd_part(const void* q, int q_stride, const void* k, const void* v, int kv_stride, const void* out,
                                    int out_stride, const void* dout, int dout_stride, const float* lse, void* dq, int dq_stride,
                                    void* dk, void* dv, int dkv_stride, void* workspace, long long workspace_bytes, const int* seq_rows,
                                    int n_seq, int n_heads, int n_kv_heads, int part, qeft_stream_t stream) {
    if (part < 0 || part > 2) return QEFT_ERR_SHAPE;
    return attn_train_varlen_bwd_entry(q, q_stride, k, v, kv_stride, out, out_stride, dout, dout_stride, lse, dq, dq_stride, dk, dv,
                                       dkv_stride, workspace, workspace_bytes, seq_rows, n_seq, n_heads, n_kv_heads, 1 << part, stream);
}

long long qeft_attn_train_varlen_bwd_check_extents(int q_stride, int kv_stride, int out_stride, int dout_stride, int dq_stride,
                                                   int dkv_stride, const int* seq_rows, int n_seq, int n_heads, int n_kv_heads) {
    qeft::AtVarGeom V;
    if (attn_train_varlen_geom(V, q_stride, kv_stride, out_stride, dout_stride, dq_stride, dkv_stride, seq_rows, n_seq, n_heads,
                               n_kv_heads) != QEFT_OK)
        return -1;
    return qeft::attn_train_varlen_bwd_count_out_of_range(V);
}

// ---- training glue (train_glue.hip)
static bool tg_stride_ok(int stride, int width) { return stride % 8 == 0 && stride >= width && stride <= (1 << 24); }

static int tg_norm_geom(qeft::TgNorm& G, int m, int hidden) {
    if (m < 1 || m > (1 << 20) || hidden < 8 || hidden % 8 != 0 || hidden > (1 << 24)) return QEFT_ERR_SHAPE;
    G = qeft::TgNorm{m, hidden};
    return QEFT_OK;
}

static int tg_swiglu_geom(qeft::TgSwiglu& G, int m, int n, int gate_stride, int up_stride, int dact_stride, int dgate_stride,
                          int dup_stride) {
    if (m < 1 || m > (1 << 20) || n < 8 || n % 8 != 0 || n > (1 << 24)) return QEFT_ERR_SHAPE;
    if (!tg_stride_ok(gate_stride, n) || !tg_stride_ok(up_stride, n) || !tg_stride_ok(dact_stride, n) || !tg_stride_ok(dgate_stride, n) ||
        !tg_stride_ok(dup_stride, n))
        return QEFT_ERR_SHAPE;
    G = qeft::TgSwiglu{m, n, gate_stride, up_stride, dact_stride, dgate_stride, dup_stride};
    if (qeft::tg_swiglu_blocks(G) >= (1ll << 31)) return QEFT_ERR_SHAPE;                 // the grid
    return QEFT_OK;
}

int qeft_add_rmsnorm_fwd(const void* h, const void* add, const void* gamma, void* sum_out, void* y, int m, int hidden, float eps,
                         qeft_stream_t stream) {
    qeft::TgNorm G{};
    if (int e = tg_norm_geom(G, m, hidden)) return e;
    if (!h || !gamma || !y || (add != nullptr) != (sum_out != nullptr)) return QEFT_ERR_NULL;
    if (!aligned16(h) || !aligned16(add) || !aligned16(gamma) || !aligned16(sum_out) || !aligned16(y)) return QEFT_ERR_ALIGN;
    return finish(qeft::add_rmsnorm_fwd_launch(h, add, gamma, sum_out, y, G, eps, (hipStream_t)stream));
}

int qeft_add_rmsnorm_bwd(const void* s, const void* gamma, const void* dy, const void* dres, void* dsum, int m, int hidden, float eps,
                         qeft_stream_t stream) {
    qeft::TgNorm G{};
    if (int e = tg_norm_geom(G, m, hidden)) return e;
    if (!dy && !dres) return QEFT_ERR_SHAPE;                     // no gradient at all: nothing to compute
    if (!s || !gamma || !dsum) return QEFT_ERR_NULL;
    if (!aligned16(s) || !aligned16(gamma) || !aligned16(dy) || !aligned16(dres) || !aligned16(dsum)) return QEFT_ERR_ALIGN;
    return finish(qeft::add_rmsnorm_bwd_launch(s, gamma, dy, dres, dsum, G, eps, (hipStream_t)stream));
}

int qeft_swiglu_fwd(const void* gate, const void* up, void* out, int m, int n, int gate_stride, int up_stride, qeft_stream_t stream) {
    qeft::TgSwiglu G{};
    if (int e = tg_swiglu_geom(G, m, n, gate_stride, up_stride, n, n, n)) return e;
    if (!gate || !up || !out) return QEFT_ERR_NULL;
    if (!aligned16(gate) || !aligned16(up) || !aligned16(out)) return QEFT_ERR_ALIGN;
    return finish(qeft::swiglu_fwd_launch(gate, up, out, G, (hipStream_t)stream));
}

int qeft_swiglu_bwd(const void* gate, const void* up, const void* dact, void* dgate, void* dup, int m, int n, int gate_stride,
                    int up_stride, int dact_stride, int dgate_stride, int dup_stride, qeft_stream_t stream) {
    qeft::TgSwiglu G{};
    if (int e = tg_swiglu_geom(G, m, n, gate_stride, up_stride, dact_stride, dgate_stride, dup_stride)) return e;
    if (!gate || !up || !dact || !dgate || !dup) return QEFT_ERR_NULL;
    if (!aligned16(gate) || !aligned16(up) || !aligned16(dact) || !aligned16(dgate) || !aligned16(dup)) return QEFT_ERR_ALIGN;
    return finish(qeft::swiglu_bwd_launch(gate, up, dact, dgate, dup, G, (hipStream_t)stream));
}

static int tg_rope_geom(qeft::TgRope& G, int rows, int t_len, int n_heads, int n_kv_heads, int q_stride, int k_stride) {
    if (rows < 1 || rows > (1 << 20) || t_len < 1 || rows % t_len != 0) return QEFT_ERR_SHAPE;
    if (n_heads < 1 || n_heads > 256 || n_kv_heads < 1 || n_kv_heads > 256) return QEFT_ERR_SHAPE;
    if (!tg_stride_ok(q_stride, n_heads * 128) || !tg_stride_ok(k_stride, n_kv_heads * 128)) return QEFT_ERR_SHAPE;
    G = qeft::TgRope{rows, t_len, n_heads, n_kv_heads, q_stride, k_stride};
    return QEFT_OK;
}

int qeft_rope_qk(const void* q, const void* k, const void* cos_tab, const void* sin_tab, void* q_out, void* k_out, int rows, int t_len,
                 int n_heads, int n_kv_heads, int q_stride, int k_stride, int inverse, qeft_stream_t stream) {
    qeft::TgRope G{};
    if (int e = tg_rope_geom(G, rows, t_len, n_heads, n_kv_heads, q_stride, k_stride)) return e;
    if (inverse != 0 && inverse != 1) return QEFT_ERR_SHAPE;
    if (!q || !k || !cos_tab || !sin_tab || !q_out || !k_out) return QEFT_ERR_NULL;
    if (!aligned16(q) || !aligned16(k) || !aligned16(cos_tab) || !aligned16(sin_tab) || !aligned16(q_out) || !aligned16(k_out))
        return QEFT_ERR_ALIGN;
    return finish(qeft::rope_qk_launch(q, k, cos_tab, sin_tab, q_out, k_out, G, inverse == 1, (hipStream_t)stream));
}

long long qeft_rope_qk_check_extents(int rows, int t_len, int n_heads, int n_kv_heads, int q_stride, int k_stride) {
    qeft::TgRope G{};
    if (tg_rope_geom(G, rows, t_len, n_heads, n_kv_heads, q_stride, k_stride) != QEFT_OK) return -1;
    return qeft::train_glue_rope_count_out_of_range(G);
}

long long qeft_train_glue_check_extents(int op, int rows, int width, int stride0, int stride1, int stride2, int stride3, int stride4) {
    switch (op) {
        case QEFT_GLUE_ADD_RMSNORM_FWD:
        case QEFT_GLUE_ADD_RMSNORM_BWD: {
            qeft::TgNorm G{};
            if (tg_norm_geom(G, rows, width) != QEFT_OK) return -1;
            return qeft::train_glue_norm_count_out_of_range(G);
        }
        case QEFT_GLUE_SWIGLU_FWD: {
            qeft::TgSwiglu G{};
            if (tg_swiglu_geom(G, rows, width, stride0, stride1, width, width, width) != QEFT_OK) return -1;
            return qeft::train_glue_swiglu_count_out_of_range(G, false);
        }
        case QEFT_GLUE_SWIGLU_BWD: {
            qeft::TgSwiglu G{};
            if (tg_swiglu_geom(G, rows, width, stride0, stride1, stride2, stride3, stride4) != QEFT_OK) return -1;
            return qeft::train_glue_swiglu_count_out_of_range(G, true);
        }
        default: return -1;
    }
}

// ---- training update (oweight_optim.hip)
// qeft_oweight_optim_lab: the measurement override of the geometry (chunks per thread per iteration, non-temporal loads of g)
static int g_oo_u = 0, g_oo_nt = 0;

static int oo_geom(qeft::OoGeom& G, long long n) {
    if (n <= 0 || n % 64 != 0 || n > qeft::OO_MAX_N) return QEFT_ERR_SHAPE;
    G = qeft::OoGeom{n, g_oo_u ? g_oo_u : qeft::OO_U};
    return QEFT_OK;
}

int qeft_oweight_optim_lab(int u, int nontemporal_g) {
    if ((u != 0 && u != 1 && u != 2 && u != 4) || (nontemporal_g != 0 && nontemporal_g != 1)) return QEFT_ERR_SHAPE;
    g_oo_u = u;
    g_oo_nt = nontemporal_g;
    return QEFT_OK;
}

int qeft_oweight_optim_blocks(long long n) {
    qeft::OoGeom G{};
    return oo_geom(G, n) == QEFT_OK ? qeft::oo_blocks(G) : 0;
}

long long qeft_oweight_optim_thread_elems(long long n) {
    qeft::OoGeom G{};
    return oo_geom(G, n) == QEFT_OK ? qeft::oo_thread_elems(G) : 0;
}

long long qeft_oweight_optim_check_extents(long long n) {
    qeft::OoGeom G{};
    if (oo_geom(G, n) != QEFT_OK) return -1;
    return qeft::oweight_optim_count_out_of_range(G);
}

int qeft_oweight_grad_stats(const void* g, long long n, const void* state_in, void* partials, qeft_stream_t stream) {
    qeft::OoGeom G{};
    if (int e = oo_geom(G, n)) return e;
    if (!g || !state_in || !partials) return QEFT_ERR_NULL;
    if (!aligned16(g) || !aligned16(state_in) || !aligned16(partials)) return QEFT_ERR_ALIGN;
    return finish(qeft::oweight_grad_stats_launch(g, G, state_in, partials, (hipStream_t)stream));
}

int qeft_oweight_adamw(void* p, const void* g, void* m, void* v, long long n, const void* state_in, void* state_out,
                       const void* partials, float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm,
                       float growth_factor, float backoff_factor, int growth_interval, int dynamic, qeft_stream_t stream) {
    qeft::OoGeom G{};
    if (int e = oo_geom(G, n)) return e;
    // written so that a NaN fails every one of them
    if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps > 0.f) || !(growth_factor > 0.f) ||
        !(backoff_factor > 0.f) || !(lr >= 0.f) || !(weight_decay >= 0.f) || !(max_norm >= 0.f) || growth_interval < 1 ||
        (dynamic != 0 && dynamic != 1))
        return QEFT_ERR_SHAPE;
    if (!p || !g || !m || !v || !state_in || !state_out || !partials || state_in == state_out) return QEFT_ERR_NULL;   // two records
    if (!aligned16(p) || !aligned16(g) || !aligned16(m) || !aligned16(v) || !aligned16(state_in) || !aligned16(state_out) ||
        !aligned16(partials))
        return QEFT_ERR_ALIGN;
    const qeft::OoHyper H{lr, beta1, beta2, eps, weight_decay, max_norm, growth_factor, backoff_factor, growth_interval, dynamic};
    return finish(qeft::oweight_adamw_launch(p, g, m, v, G, state_in, state_out, partials, H, g_oo_nt != 0, (hipStream_t)stream));
}

// ---- calibration (calib.hip)
static int ha_geom(qeft::HaGeom& G, int t, int k) {
    if (t < 1 || t > qeft::HA_MAX_T || k < 64 || k % 64 != 0 || k > qeft::HA_MAX_K) return QEFT_ERR_SHAPE;
    G = qeft::HaGeom{t, k};
    return QEFT_OK;
}

int qeft_hessian_accum(const void* x, void* h, int t, int k, float alpha, float beta, qeft_stream_t stream) {
    qeft::HaGeom G{};
    if (int e = ha_geom(G, t, k)) return e;
    if (!x || !h) return QEFT_ERR_NULL;
    if (!aligned16(x) || !aligned16(h)) return QEFT_ERR_ALIGN;
    return finish(qeft::hessian_accum_launch(x, h, G, alpha, beta, (hipStream_t)stream));
}

long long qeft_hessian_accum_check_extents(int t, int k) {
    qeft::HaGeom G{};
    if (ha_geom(G, t, k) != QEFT_OK || k > qeft::HA_MAX_K_ENUM) return -1;
    return qeft::hessian_accum_count_out_of_range(G);
}

int qeft_gptq_block(void* w1, int ld_w, const void* hinv1, int ld_h, const void* scale, const void* zero, void* q1, void* err1, int n,
                    int count, int maxq, qeft_stream_t stream) {
    if (n < 1 || count < 1 || count > qeft::GB_MAX_COUNT || ld_w < count || ld_h < count || (maxq != 7 && maxq != 15))
        return QEFT_ERR_SHAPE;
    if (!w1 || !hinv1 || !scale || !zero || !q1 || !err1) return QEFT_ERR_NULL;
    if (((uintptr_t)w1 | (uintptr_t)hinv1 | (uintptr_t)scale | (uintptr_t)zero | (uintptr_t)q1 | (uintptr_t)err1) & 3) return QEFT_ERR_ALIGN;
    const qeft::GbGeom G{n, count, ld_w, ld_h};
    return finish(qeft::gptq_block_launch(w1, hinv1, scale, zero, q1, err1, G, (float)maxq, (hipStream_t)stream));
}

// ---- fused lm_head + cross-entropy pieces (lm_head_nll.hip)
static bool lm_head_nll_shape_ok(int x_stride, int t, int hidden, int vocab) {
    if (t < 1 || t > (1 << 20) || vocab < 1 || vocab > (1 << 24) || hidden < 64 || hidden % 64 != 0 || hidden > (1 << 16)) return false;
    if (x_stride % 8 != 0 || x_stride < hidden || x_stride > (1 << 24)) return false;
    return ((long long)(t + 63) / 64) * ((vocab + 127) / 128) < (1ll << 31);          // the grid of the 64-row tile
}

long long qeft_lm_head_nll_workspace_bytes(int t, int vocab) {
    if (!lm_head_nll_shape_ok(64, t, 64, vocab)) return 0;
    return (long long)qeft::lm_head_nll_workspace_bytes(t, vocab);
}

int qeft_lm_head_nll(const void* x, int x_stride, const void* weight, const int* targets, float* lse, float* tgt_logit, int* argmax,
                     void* workspace, long long workspace_bytes, int t, int hidden, int vocab, qeft_stream_t stream) {
    if (!lm_head_nll_shape_ok(x_stride, t, hidden, vocab)) return QEFT_ERR_SHAPE;
    if (workspace_bytes < (long long)qeft::lm_head_nll_workspace_bytes(t, vocab)) return QEFT_ERR_SHAPE;
    if (!x || !weight || !lse || !workspace || (targets && !tgt_logit)) return QEFT_ERR_NULL;
    if (!aligned16(x) || !aligned16(weight) || !aligned16(workspace) || ((uintptr_t)targets & 3) || ((uintptr_t)lse & 3) ||
        ((uintptr_t)tgt_logit & 3) || ((uintptr_t)argmax & 3))
        return QEFT_ERR_ALIGN;
    return finish(qeft::lm_head_nll_launch(x, weight, targets, lse, tgt_logit, argmax, workspace, x_stride, t, hidden, vocab,
                                           (hipStream_t)stream));
}

long long qeft_lm_head_nll_check_extents(int x_stride, int t, int hidden, int vocab) {
    if (!lm_head_nll_shape_ok(x_stride, t, hidden, vocab)) return -1;
    return qeft::lm_head_nll_count_out_of_range(x_stride, t, hidden, vocab);
}

// ---- backward of the fused lm_head + cross-entropy (lm_head_nll_grad.hip)
static bool lm_head_nll_grad_shape_ok(int x_stride, int dx_stride, int t, int hidden, int vocab) {
    if (!lm_head_nll_shape_ok(x_stride, t, hidden, vocab)) return false;
    return dx_stride % 8 == 0 && dx_stride >= hidden && dx_stride <= (1 << 24);
}

int qeft_lm_head_nll_grad_chunk_rows(int hidden, int vocab) {
    (void)hidden;
    (void)vocab;
    return qeft::lm_head_nll_grad_chunk_rows();
}

long long qeft_lm_head_nll_grad_workspace_bytes(int t, int hidden, int vocab) {
    if (!lm_head_nll_grad_shape_ok(hidden, hidden, t, hidden, vocab)) return 0;
    return (long long)qeft::lm_head_nll_grad_workspace_bytes(t, vocab);
}

int qeft_lm_head_nll_grad(const void* x, int x_stride, const void* weight, const int* targets, const float* lse,
                          const float* grad_nll, void* dx, int dx_stride, int dx_fp32, void* workspace, long long workspace_bytes,
                          int t, int hidden, int vocab, qeft_stream_t stream) {
    if (!lm_head_nll_grad_shape_ok(x_stride, dx_stride, t, hidden, vocab)) return QEFT_ERR_SHAPE;
    if (workspace_bytes < (long long)qeft::lm_head_nll_grad_workspace_bytes(t, vocab)) return QEFT_ERR_SHAPE;
    if (!x || !weight || !targets || !lse || !grad_nll || !dx || !workspace) return QEFT_ERR_NULL;
    if (!aligned16(x) || !aligned16(weight) || !aligned16(dx) || !aligned16(workspace) || ((uintptr_t)targets & 3) ||
        ((uintptr_t)lse & 3) || ((uintptr_t)grad_nll & 3))
        return QEFT_ERR_ALIGN;
    return finish(qeft::lm_head_nll_grad_launch(x, weight, targets, lse, grad_nll, dx, workspace, x_stride, dx_stride, dx_fp32 != 0, t,
                                                hidden, vocab, (hipStream_t)stream));
}

long long qeft_lm_head_nll_grad_check_extents(int x_stride, int dx_stride, int t, int hidden, int vocab) {
    if (!lm_head_nll_grad_shape_ok(x_stride, dx_stride, t, hidden, vocab)) return -1;
    return qeft::lm_head_nll_grad_count_out_of_range(x_stride, dx_stride, t, hidden, vocab);
}

// ---- sampled token end (decode_sample.hip)
int qeft_sample(const void* logits, int vocab, int m, const int* params, const int* positions, void* tokens_out,
                qeft_stream_t stream) {
    if (m < 1) return QEFT_ERR_BATCH;
    if (vocab < 1) return QEFT_ERR_SHAPE;
    if (!logits || !params || !positions || !tokens_out) return QEFT_ERR_NULL;
    if (!aligned16(logits) || !aligned16(params)) return QEFT_ERR_ALIGN;
    return finish(qeft::sample_launch(logits, vocab, m, params, positions, tokens_out, (hipStream_t)stream));
}

int qeft_token_end_sample(const void* logits, void* tok, int* pos, int vocab, const int* params, qeft_stream_t stream) {
    if (vocab < 1) return QEFT_ERR_SHAPE;
    if (!logits || !tok || !pos || !params) return QEFT_ERR_NULL;
    if (!aligned16(logits) || !aligned16(params)) return QEFT_ERR_ALIGN;
    return finish(qeft::token_end_sample_launch(logits, tok, pos, params, vocab, (hipStream_t)stream));
}

int qeft_token_end_sample_batch(const void* logits, const int* slots, void* tokens, int* pos, const int* limit, const int* eos,
                                int* done, void* out, int* counter, const int* params, int vocab, int out_cap, int n_slots, int m,
                                qeft_stream_t stream) {
    if (!verify_m_ok(m)) return QEFT_ERR_BATCH;
    if (vocab < 1 || out_cap < 1 || n_slots < 1) return QEFT_ERR_SHAPE;
    if (!logits || !slots || !tokens || !pos || !limit || !eos || !done || !out || !counter || !params) return QEFT_ERR_NULL;
    if (!aligned16(logits) || !aligned16(params)) return QEFT_ERR_ALIGN;
    return finish(qeft::token_end_sample_b_launch(logits, slots, tokens, pos, limit, eos, done, out, counter, params, vocab, out_cap,
                                                  n_slots, m, (hipStream_t)stream));
}

int qeft_verify_sample(const void* logits, const void* tokens, int m, int vocab, const int* params, int* work, void* out_tokens,
                       int* n_accepted, void* tok, int* pos, qeft_stream_t stream) {
    if (!verify_m_ok(m)) return QEFT_ERR_BATCH;
    if (vocab < 1) return QEFT_ERR_SHAPE;
    if (!logits || !tokens || !params || !work || !out_tokens || !n_accepted || !tok || !pos) return QEFT_ERR_NULL;
    if (!aligned16(logits) || !aligned16(params)) return QEFT_ERR_ALIGN;
    return finish(qeft::verify_sample_launch(logits, tokens, m, vocab, params, work, out_tokens, n_accepted, tok, pos,
                                             (hipStream_t)stream));
}

}  // extern "C"
