// Records what the C ABI decides on a CPU: for each call its return code, qeft_last_variant() and, for every launch the
// library would make, the kernel's symbol, grid, block, LDS bytes and arguments.  Launches nothing and opens no device: the
// library sources are compiled with tools/capi_record.h in front of them, which replaces the three HIP calls they make.
// Built against two trees and run on the same inputs, the two outputs are compared byte for byte (a refactor of capi.hip
// or of a launcher's host side must leave them identical).  A tool: not run by the test suite, never on a GPU machine.
//
//   for s in <tree>/qeft_amd/csrc/*.hip (all of build.SOURCES but oneshot.hip):
//       hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -mllvm -amdgpu-kernarg-preload-count=16 -w \
//             -include tools/capi_record.h -c $s -o obj/$(basename $s .hip).o          (a full compile, not --cuda-host-only)
//   clang++ -O1 -std=c++17 -I<tree>/include -c tools/capi_record.cpp -o obj/main.o      (plain C++)
//   hipcc --offload-arch=gfx950 --hip-link -rdynamic obj/*.o -ldl -o capi_record
//   ./capi_record [full|reduced] [refusals.jsonl] > record.txt
//       reduced: the shorter list, for runs under QEFT_GEMV_V3=0, QEFT_GEMM_WS=0, QEFT_GEMV_XG=0|2
//       refusals.jsonl: every refused call that made no HIP call, as ["entry", [arguments], code, "single"|"pair"]; an array
//       of pointers is a list of addresses, an array of ints {"ints": [...]}, a missing array null
//       (tests/golden/capi_refusals_parent.json.gz: the parent's rows, every "single" and every third "pair")
//
// Operand i of a call is the made-up address (i + 1) << 24, so a kernel argument prints as A<i>+<offset>.  For each entry:
// a grid of accepted calls, then around some of them every argument wrong alone (NULL, misaligned by 2 / 4 / 8, a list of
// integers) and every two arguments wrong together (which pins the precedence of the checks), then the launcher errors the
// entry maps (hipGetLastError programmed to fail once).
#include <stdint.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "qeft_hip.h"

extern "C" {
FILE* capi_rec_out = nullptr;
int capi_rec_next_error = 0;
int capi_rec_hip_calls = 0;
}

typedef long long ll;
typedef std::vector<ll> Args;

// kinds: p pointer, i int, l long long, f float (in millionths), s stream, A array of pointers [nparts], N array of ints [nparts]
struct Entry {
    const char* name;
    const char* kinds;
    std::function<ll(const Args&)> fn;
    int nparts_at = -1;
};

static FILE* g_refusals = nullptr;
static long g_calls = 0, g_refused_rows = 0;

static ll base_of(int i) { return (ll)(i + 1) << 24; }
static void* P(const Args& a, int i) { return (void*)(uintptr_t)a[i]; }
static int I(const Args& a, int i) { return (int)a[i]; }
static float F(const Args& a, int i) { return (float)a[i] * 1e-6f; }

// array arguments: v == 0: no array; else element p = (v & ~15) + (p << 16), all 2 bytes askew if v & 2, the last one NULL if v & 1
struct PtrArray {
    void* e[3];
    void** get(ll v, int nparts) {
        if (v == 0) return nullptr;
        for (int p = 0; p < 3; ++p) e[p] = (void*)(uintptr_t)((v & ~15ll) + ((ll)p << 16) + ((v & 2) ? 2 : 0));
        if ((v & 1) && nparts >= 1 && nparts <= 3) e[nparts - 1] = nullptr;
        return e;
    }
};
constexpr ll kNoIntArray = -999;
struct IntArray {
    int e[3];
    int* get(ll v) {
        if (v == kNoIntArray) return nullptr;
        e[0] = e[1] = e[2] = (int)v;
        return e;
    }
};

static void print_value(FILE* f, const Entry& en, const Args& a, size_t i, bool json) {
    const char k = en.kinds[i];
    const int nparts = en.nparts_at >= 0 ? (int)a[en.nparts_at] : 0;
    if (k == 'A') {
        PtrArray arr;
        void** e = arr.get(a[i], nparts);
        if (!e) { fprintf(f, json ? "null" : "0"); return; }
        fputc('[', f);
        for (int p = 0; p < 3; ++p) fprintf(f, "%s%llu", p ? "," : "", (unsigned long long)(uintptr_t)e[p]);
        fputc(']', f);
    } else if (k == 'N') {
        if (a[i] == kNoIntArray) { fprintf(f, json ? "null" : "0"); return; }
        fprintf(f, json ? "{\"ints\":[%lld,%lld,%lld]}" : "[%lld,%lld,%lld]", a[i], a[i], a[i]);
    } else if (k == 'f') {
        fprintf(f, "%.9g", (double)F(a, (int)i));
    } else if (k == 'p' && !json) {
        const ll v = a[i], b = base_of((int)i);
        if (v == 0) fprintf(f, "0");
        else if (v == b) fprintf(f, "A%zu", i);
        else fprintf(f, "A%zu+%llx", i, v - b);
    } else {
        fprintf(f, "%lld", a[i]);
    }
}

namespace qeft { extern thread_local const char* g_last_variant; }

static ll record(const Entry& en, const Args& a, const char* tag) {
    static char* buf = nullptr;
    static size_t buf_size = 0;
    FILE* mem = open_memstream(&buf, &buf_size);
    capi_rec_out = mem;
    qeft::g_last_variant = "";
    const int calls0 = capi_rec_hip_calls;
    const ll code = en.fn(a);
    const int hip_calls = capi_rec_hip_calls - calls0;
    fclose(mem);
    ++g_calls;
    printf("%s(", en.name);
    for (size_t i = 0; i < a.size(); ++i) {
        if (i) putchar(' ');
        print_value(stdout, en, a, i, false);
    }
    printf(") = %lld variant '%s'", code, qeft_last_variant());
    if (code == QEFT_ERR_LAUNCH) printf(" hip_error %d", qeft_last_hip_error());
    fwrite(buf, 1, buf_size, stdout);
    putchar('\n');
    capi_rec_next_error = 0;
    if (g_refusals && tag && code != 0 && code != QEFT_ERR_LAUNCH && hip_calls == 0 && strchr(en.kinds, 'p')) {
        fprintf(g_refusals, "[\"%s\",[", en.name);
        for (size_t i = 0; i < a.size(); ++i) {
            if (i) fputc(',', g_refusals);
            print_value(g_refusals, en, a, i, true);
        }
        fprintf(g_refusals, "],%lld,\"%s\"]\n", code, tag);
        ++g_refused_rows;
    }
    return code;
}

// ---- the ways one argument can be wrong
static const ll kIntsSingle[] = {-1, 0, 1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 48, 64, 96, 100, 128, 160, 192, 256, 512, 4096, 4100, 32768, 32784, 65536};
static const ll kIntsPair[] = {-1, 0, 3, 9, 100, 32784};
static const ll kArrayFlags[] = {1, 2};

static std::vector<ll> mutations(const Entry& en, const Args& a, size_t i, bool pair) {
    std::vector<ll> out;
    switch (en.kinds[i]) {
        case 'p':
            if (a[i] != 0) out = {0, a[i] + 2, a[i] + 4, a[i] + 8};
            else out = {base_of((int)i), base_of((int)i) + 2, base_of((int)i) + 4};       // an optional operand that the base call leaves out
            break;
        case 'i':
            if (pair) out.assign(kIntsPair, kIntsPair + sizeof(kIntsPair) / sizeof(ll));
            else out.assign(kIntsSingle, kIntsSingle + sizeof(kIntsSingle) / sizeof(ll));
            break;
        case 'l': out = {-1, 0, 1, 4096, 1ll << 20, 1ll << 33}; break;
        case 'A':
            if (a[i] != 0) { out.push_back(0); for (ll f : kArrayFlags) out.push_back(a[i] | f); }
            else out.push_back(base_of((int)i));
            break;
        case 'N': out = {kNoIntArray, 0, 6, 100}; break;
        default: break;
    }
    return out;
}

static void singles(const Entry& en, const Args& base) {
    for (size_t i = 0; i < base.size(); ++i)
        for (ll v : mutations(en, base, i, false)) {
            if (v == base[i]) continue;
            Args a = base;
            a[i] = v;
            record(en, a, "single");
        }
}

static void pairs(const Entry& en, const Args& base) {
    for (size_t i = 0; i < base.size(); ++i)
        for (ll vi : mutations(en, base, i, true)) {
            if (vi == base[i]) continue;
            for (size_t j = i + 1; j < base.size(); ++j)
                for (ll vj : mutations(en, base, j, true)) {
                    if (vj == base[j]) continue;
                    Args a = base;
                    a[i] = vi;
                    a[j] = vj;
                    record(en, a, "pair");
                }
        }
}

// hipErrorInvalidValue, hipErrorNotSupported and one that no entry maps (hipErrorLaunchFailure), from the first hipGetLastError
static void launcher_errors(const Entry& en, const Args& base) {
    for (int e : {1, 801, 719}) {
        capi_rec_next_error = e;
        record(en, base, nullptr);
    }
}

// all operands present (pointer i at its base, arrays whole); the integers come from the caller
static Args operands(const Entry& en) {
    Args a(strlen(en.kinds), 0);
    for (size_t i = 0; i < a.size(); ++i)
        if (en.kinds[i] == 'p' || en.kinds[i] == 'A') a[i] = base_of((int)i);
    return a;
}

struct Shape { int n, k; };
static const Shape kShapes[] = {            // q|k|v, o, gate|up, down of Llama-2-7B / 13B / 70B (tests/test_gpu_verify_shapes.py) and the smallest
    {12288, 4096}, {4096, 4096}, {22016, 4096}, {4096, 11008}, {11008, 4096},
    {15360, 5120}, {5120, 5120}, {27648, 5120}, {5120, 13824}, {13824, 5120},
    {10240, 8192}, {8192, 8192}, {57344, 8192}, {8192, 28672}, {28672, 8192},
    {16, 128}, {16, 256}, {8, 64}, {64, 192}, {4104, 4160}};
static const Shape kShapesReduced[] = {{4096, 4096}, {22016, 4096}, {4096, 11008}, {5120, 13824}, {16, 256}, {8, 64}, {4104, 4160}};

static bool g_reduced = false;
static std::vector<Shape> shapes() {
    if (g_reduced) return std::vector<Shape>(kShapesReduced, kShapesReduced + sizeof(kShapesReduced) / sizeof(Shape));
    return std::vector<Shape>(kShapes, kShapes + sizeof(kShapes) / sizeof(Shape));
}

// set the integers named in `at` (index, value pairs)
static Args with(Args a, std::initializer_list<std::pair<int, ll>> at) {
    for (auto& p : at) a[p.first] = p.second;
    return a;
}
// every subset of the optional operands `opt` left out
static void optional_subsets(const Entry& en, const Args& base, std::vector<int> opt, const char* tag = nullptr) {
    for (unsigned mask = 0; mask < (1u << opt.size()); ++mask) {
        Args a = base;
        for (size_t b = 0; b < opt.size(); ++b)
            if (mask >> b & 1) a[opt[b]] = 0;
        record(en, a, tag);
    }
}

#define FN [](const Args& a) -> ll

int main(int argc, char** argv) {
    g_reduced = argc > 1 && !strcmp(argv[1], "reduced");
    if (argc > 2) g_refusals = fopen(argv[2], "w");
    const bool full = !g_reduced;
    const std::vector<ll> groups = {128, -1 /* == k */, 64, 32, 256, 96};
    const int ms17[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 24, 33, 64, 65, 128, 200, 2048};

    // ---- the reference's GEMV entries
    {
        const Entry fused{"qeft_gemv_w4_fused", "ppppppppppiiiiis", FN {
            return qeft_gemv_w4_fused(P(a, 0), P(a, 1), P(a, 2), P(a, 3), P(a, 4), P(a, 5), (const int*)P(a, 6), P(a, 7), P(a, 8), P(a, 9), I(a, 10),
                                      I(a, 11), I(a, 12), I(a, 13), I(a, 14), P(a, 15)); }};
        const Entry plain{"qeft_gemv_w4", "pppppiiiis", FN {
            return qeft_gemv_w4(P(a, 0), P(a, 1), P(a, 2), P(a, 3), P(a, 4), I(a, 5), I(a, 6), I(a, 7), I(a, 8), P(a, 9)); }};
        const Entry outl{"qeft_gemv_w4_qeft", "ppppppiiiiis", FN {
            return qeft_gemv_w4_qeft(P(a, 0), P(a, 1), P(a, 2), P(a, 3), P(a, 4), P(a, 5), I(a, 6), I(a, 7), I(a, 8), I(a, 9), I(a, 10), P(a, 11)); }};
        const Entry w3{"qeft_gemv_w3", "pppppppppiiiiis", FN {
            return qeft_gemv_w3(P(a, 0), P(a, 1), P(a, 2), P(a, 3), P(a, 4), P(a, 5), P(a, 6), P(a, 7), P(a, 8), I(a, 9), I(a, 10), I(a, 11), I(a, 12),
                                I(a, 13), P(a, 14)); }};
        for (const Shape& s : shapes())
            for (ll g : groups)
                for (int n_out : {0, 128, 32, 64})
                    for (int m = 1; m <= 8; ++m) {
                        const ll gs = g < 0 ? s.k : g;
                        const Args f = with(operands(fused), {{10, m}, {11, s.n}, {12, s.k}, {13, gs}, {14, n_out}});
                        const bool few = m == 1 || m == 4 || m == 7;
                        if (few && (n_out == 0 || n_out == 128)) optional_subsets(fused, n_out ? f : with(f, {{4, 0}}), {5, 6, 7, 8});
                        else record(fused, n_out ? f : with(f, {{4, 0}}), nullptr);
                        if (n_out == 0) record(plain, with(operands(plain), {{5, m}, {6, s.n}, {7, s.k}, {8, gs}}), nullptr);
                        record(outl, with(operands(outl), {{6, m}, {7, s.n}, {8, s.k}, {9, gs}, {10, n_out}}), nullptr);
                        const Args w = with(operands(w3), {{9, m}, {10, s.n}, {11, s.k}, {12, gs}, {13, n_out}});
                        if (few && n_out != 32) optional_subsets(w3, n_out ? w : with(w, {{4, 0}}), {5, 6, 7});
                        else record(w3, w, nullptr);
                    }
        const Args fb = with(operands(fused), {{10, 3}, {11, 4096}, {12, 4096}, {13, 128}, {14, 128}});
        for (const Args& b : {fb, with(fb, {{7, 0}}), with(fb, {{13, 64}, {14, 64}}), with(fb, {{10, 1}, {11, 8}, {12, 64}, {13, 32}, {14, 0}, {4, 0}})}) {
            singles(fused, b);
            if (full) pairs(fused, b);
            launcher_errors(fused, b);
        }
        const Args pb = with(operands(plain), {{5, 2}, {6, 4096}, {7, 4096}, {8, 128}});
        singles(plain, pb);
        if (full) pairs(plain, pb);
        launcher_errors(plain, pb);
        const Args ob = with(operands(outl), {{6, 2}, {7, 4096}, {8, 4096}, {9, 128}, {10, 128}});
        singles(outl, ob);
        if (full) pairs(outl, ob);
        launcher_errors(outl, ob);
        const Args wb = with(operands(w3), {{9, 2}, {10, 4096}, {11, 4096}, {12, 128}, {13, 128}});
        singles(w3, wb);
        if (full) pairs(w3, wb);
        launcher_errors(w3, wb);
    }
    {
        const Entry silu4{"qeft_gemv_w4_silu", "ppppppppppiiiis", FN {
            return qeft_gemv_w4_silu(P(a, 0), P(a, 1), P(a, 2), P(a, 3), P(a, 4), P(a, 5), P(a, 6), P(a, 7), P(a, 8), P(a, 9), I(a, 10), I(a, 11),
                                     I(a, 12), I(a, 13), P(a, 14)); }};
        const Entry silu3{"qeft_gemv_w3_silu", "ppppppppppiiiis", FN {
            return qeft_gemv_w3_silu(P(a, 0), P(a, 1), P(a, 2), P(a, 3), P(a, 4), P(a, 5), P(a, 6), P(a, 7), P(a, 8), P(a, 9), I(a, 10), I(a, 11),
                                     I(a, 12), I(a, 13), P(a, 14)); }};
        for (const Entry* en : {&silu4, &silu3}) {
            for (const Shape& s : shapes())
                for (ll g : groups)
                    for (int n_out : {0, 128, 32, 64}) {
                        const Args b = with(operands(*en), {{10, s.n}, {11, s.k}, {12, g < 0 ? s.k : g}, {13, n_out}});
                        optional_subsets(*en, n_out ? b : with(b, {{5, 0}}), {6, 7, 8});
                    }
            const Args b = with(operands(*en), {{10, 4096}, {11, 11008}, {12, 128}, {13, 128}});
            singles(*en, b);
            if (full) pairs(*en, b);
            launcher_errors(*en, b);
        }
    }
    {
        Entry g4{"qeft_gemv_w4_group", "ppfiAAAAAAANiiis", FN {
            PtrArray q, s, z, o, b, p, y;
            IntArray n;
            const int np = I(a, 3);
            return qeft_gemv_w4_group(P(a, 0), P(a, 1), F(a, 2), np, q.get(a[4], np), s.get(a[5], np), z.get(a[6], np), o.get(a[7], np),
                                      b.get(a[8], np), p.get(a[9], np), y.get(a[10], np), n.get(a[11]), I(a, 12), I(a, 13), I(a, 14), P(a, 15)); }};
        Entry g3{"qeft_gemv_w3_group", "ppfiAAAAAAANiiis", FN {
            PtrArray q, s, z, o, b, p, y;
            IntArray n;
            const int np = I(a, 3);
            return qeft_gemv_w3_group(P(a, 0), P(a, 1), F(a, 2), np, q.get(a[4], np), s.get(a[5], np), z.get(a[6], np), o.get(a[7], np),
                                      b.get(a[8], np), p.get(a[9], np), y.get(a[10], np), n.get(a[11]), I(a, 12), I(a, 13), I(a, 14), P(a, 15)); }};
        g4.nparts_at = g3.nparts_at = 3;
        for (const Entry* en : {&g4, &g3}) {
            for (const Shape& s : shapes())
                for (ll g : groups)
                    for (int n_out : {0, 128, 64})
                        for (int np = 1; np <= 3; ++np) {
                            const Args b = with(operands(*en), {{2, 10}, {3, np}, {11, s.n}, {12, s.k}, {13, g < 0 ? s.k : g}, {14, n_out}});
                            optional_subsets(*en, n_out ? b : with(b, {{7, 0}}), {1, 8, 9});
                        }
            const Args b = with(operands(*en), {{2, 10}, {3, 3}, {11, 4096}, {12, 4096}, {13, 128}, {14, 128}});
            singles(*en, b);
            if (full) pairs(*en, b);
            launcher_errors(*en, b);
        }
    }

    // ---- the GEMM forward entries
    {
        const Entry gemm{"qeft_gemm_w4", "pppppppiiiiis", FN {
            return qeft_gemm_w4(P(a, 0), P(a, 1), P(a, 2), P(a, 3), P(a, 4), P(a, 5), P(a, 6), I(a, 7), I(a, 8), I(a, 9), I(a, 10), I(a, 11), P(a, 12)); }};
        const Entry gemm3{"qeft_gemm_w3", "pppppppiiiiis", FN {
            return qeft_gemm_w3(P(a, 0), P(a, 1), P(a, 2), P(a, 3), P(a, 4), P(a, 5), P(a, 6), I(a, 7), I(a, 8), I(a, 9), I(a, 10), I(a, 11), P(a, 12)); }};
        const Entry gateup{"qeft_gemm_w4_gateup", "pppppppiiiiis", FN {
            return qeft_gemm_w4_gateup(P(a, 0), P(a, 1), P(a, 2), P(a, 3), P(a, 4), P(a, 5), P(a, 6), I(a, 7), I(a, 8), I(a, 9), I(a, 10), I(a, 11), P(a, 12)); }};
        const Entry silu{"qeft_gemm_w4_silu_mul", "ppppppppiiiiis", FN {
            return qeft_gemm_w4_silu_mul(P(a, 0), P(a, 1), P(a, 2), P(a, 3), P(a, 4), P(a, 5), P(a, 6), P(a, 7), I(a, 8), I(a, 9), I(a, 10), I(a, 11),
                                         I(a, 12), P(a, 13)); }};
        const Entry ws{"qeft_gemm_w4_ws", "ppppppppliiiiis", FN {
            return qeft_gemm_w4_ws(P(a, 0), P(a, 1), P(a, 2), P(a, 3), P(a, 4), P(a, 5), P(a, 6), P(a, 7), a[8], I(a, 9), I(a, 10), I(a, 11), I(a, 12),
                                   I(a, 13), P(a, 14)); }};
        const Entry wsb{"qeft_gemm_w4_workspace_bytes", "iiii", FN { return qeft_gemm_w4_workspace_bytes(I(a, 0), I(a, 1), I(a, 2), I(a, 3)); }};
        for (const Shape& s : shapes())
            for (ll g : groups)
                for (int n_out : {0, 128, 64})
                    for (int m : ms17) {
                        const ll gs = g < 0 ? s.k : g;
                        for (int ow : {1, 0})
                            for (int bias : {1, 0}) {
                                if ((!ow || !bias) && m != 1 && m != 8 && m != 16 && m != 17 && m != 65) continue;
                                Args b = with(operands(gemm), {{7, m}, {8, s.n}, {9, s.k}, {10, gs}, {11, n_out}});
                                if (!ow) b[4] = 0;
                                if (!bias) b[5] = 0;
                                record(gemm, b, nullptr);
                                if (g == 128 || g < 0) record(gemm3, b, nullptr);
                                if (g == 128) record(gateup, b, nullptr);
                                Args sb = with(operands(silu), {{8, m}, {9, s.n}, {10, s.k}, {11, gs}, {12, n_out}});
                                if (!ow) sb[4] = 0;
                                if (!bias) sb[5] = 0;
                                if (g == 128 || g == 96 || m <= 17) record(silu, sb, nullptr);
                                const ll need = qeft_gemm_w4_workspace_bytes(m, s.n, s.k, n_out);
                                for (ll bytes : {need, need - 1, 0ll, 1ll << 32}) {
                                    if (bytes < 0 || (bytes == need - 1 && need == 0)) continue;
                                    Args wa = with(operands(ws), {{8, bytes}, {9, m}, {10, s.n}, {11, s.k}, {12, gs}, {13, n_out}});
                                    if (!ow) wa[4] = 0;
                                    if (!bias) wa[5] = 0;
                                    record(ws, wa, nullptr);
                                    if (bytes == need) record(ws, with(wa, {{7, 0}}), nullptr);
                                }
                            }
                        if (g == 128) record(wsb, {m, s.n, s.k, n_out}, nullptr);
                    }
        const Args gb = with(operands(gemm), {{7, 12}, {8, 4096}, {9, 4096}, {10, 128}, {11, 128}});
        for (const Entry* en : {&gemm, &gemm3, &gateup})
            for (const Args& b : {gb, with(gb, {{7, 40}}), with(gb, {{7, 16}, {8, 4104}, {9, 4160}, {10, 32}, {11, 64}}), with(gb, {{7, 300}})}) {
                singles(*en, b);
                if (full) pairs(*en, b);
                launcher_errors(*en, b);
            }
        const Args sb = with(operands(silu), {{8, 12}, {9, 4096}, {10, 4096}, {11, 128}, {12, 128}});
        for (const Args& b : {sb, with(sb, {{8, 300}})}) {
            singles(silu, b);
            if (full) pairs(silu, b);
            launcher_errors(silu, b);
        }
        const Args wb = with(operands(ws), {{8, 1ll << 30}, {9, 12}, {10, 4096}, {11, 4096}, {12, 128}, {13, 128}});
        for (const Args& b : {wb, with(wb, {{9, 96}}), with(wb, {{9, 16}, {10, 4104}, {11, 4160}, {12, 32}, {13, 64}})}) {
            singles(ws, b);
            if (full) pairs(ws, b);
            launcher_errors(ws, b);
        }
        singles(wsb, {12, 4096, 4096, 128});
    }

    // ---- the decode engine's linears
    {
        const Entry lin{"qeft_decode_linear", "ppppppiiiiippifppps", FN {
            return qeft_decode_linear(P(a, 0), P(a, 1), P(a, 2), P(a, 3), P(a, 4), P(a, 5), I(a, 6), I(a, 7), I(a, 8), I(a, 9), I(a, 10), P(a, 11),
                                      (const float*)P(a, 12), I(a, 13), F(a, 14), P(a, 15), P(a, 16), (float*)P(a, 17), P(a, 18)); }};
        const Entry lin3{"qeft_decode_linear_w3", "ppppppiiiiippifppps", FN {
            return qeft_decode_linear_w3(P(a, 0), P(a, 1), P(a, 2), P(a, 3), P(a, 4), P(a, 5), I(a, 6), I(a, 7), I(a, 8), I(a, 9), I(a, 10), P(a, 11),
                                         (const float*)P(a, 12), I(a, 13), F(a, 14), P(a, 15), P(a, 16), (float*)P(a, 17), P(a, 18)); }};
        const Entry linm{"qeft_decode_linear_m", "ppppppiiiiippifpppis", FN {
            return qeft_decode_linear_m(P(a, 0), P(a, 1), P(a, 2), P(a, 3), P(a, 4), P(a, 5), I(a, 6), I(a, 7), I(a, 8), I(a, 9), I(a, 10), P(a, 11),
                                        (const float*)P(a, 12), I(a, 13), F(a, 14), P(a, 15), P(a, 16), (float*)P(a, 17), I(a, 18), P(a, 19)); }};
        const Entry hn{"qeft_decode_linear_hnorm", "pppppppiiiiifs", FN {
            return qeft_decode_linear_hnorm(P(a, 0), P(a, 1), P(a, 2), P(a, 3), P(a, 4), P(a, 5), P(a, 6), I(a, 7), I(a, 8), I(a, 9), I(a, 10), I(a, 11),
                                            F(a, 12), P(a, 13)); }};
        for (const Shape& s : shapes())
            for (ll g : {128ll, -1ll})
                for (int n_out : {0, 128})
                    for (int mode : {0, 1}) {
                        const ll gs = g < 0 ? s.k : g;
                        for (const Entry* en : {&lin, &lin3, &linm})
                            for (int m = 1; m <= (en == &linm ? 8 : 1); ++m)
                                for (int ssq : {0, 1, 16, 512}) {
                                    Args b = with(operands(*en), {{6, s.n}, {7, s.k}, {8, gs}, {9, n_out}, {10, mode}, {13, ssq}, {14, 10}});
                                    if (en == &linm) b[18] = m;
                                    if (!n_out) b[3] = 0;
                                    if (!ssq) b[12] = 0;
                                    // no epilogue / residual / residual + gamma_out, each with and without the bias
                                    for (int epi = 0; epi < 3; ++epi)
                                        for (int bias : {1, 0}) {
                                            Args c = b;
                                            if (!bias) c[4] = 0;
                                            if (epi == 0) c[11] = c[15] = c[16] = c[17] = 0;
                                            if (epi == 1) c[15] = c[16] = c[17] = 0;
                                            record(*en, c, nullptr);
                                        }
                                }
                        Args h = with(operands(hn), {{7, s.n}, {8, s.k}, {9, gs}, {10, n_out}, {11, mode}, {12, 10}});
                        if (!n_out) h[4] = 0;
                        optional_subsets(hn, h, {5});
                    }
        const Args lb = with(operands(lin), {{6, 4096}, {7, 4096}, {8, 128}, {9, 128}, {10, 0}, {13, 16}, {14, 10}});
        for (const Entry* en : {&lin, &lin3, &linm})
            for (int m : {1, 4}) {
                if (en != &linm && m == 4) continue;
                Args b = lb;
                if (en == &linm) { b.insert(b.begin() + 18, m); b[19] = 0; }
                for (const Args& c : {b, with(b, {{10, 1}, {11, 0}, {15, 0}, {16, 0}, {17, 0}}), with(b, {{11, 0}, {12, 0}, {13, 0}, {15, 0}, {16, 0}, {17, 0}, {3, 0}, {9, 0}})}) {
                    singles(*en, c);
                    if (full) pairs(*en, c);
                    launcher_errors(*en, c);
                }
            }
        const Args hb = with(operands(hn), {{7, 4096}, {8, 4096}, {9, 128}, {10, 128}, {11, 0}, {12, 10}});
        singles(hn, hb);
        if (full) pairs(hn, hb);
        launcher_errors(hn, hb);
    }

    // ---- the row-wise attention entries and their workspace queries
    {
        const Entry am{"qeft_rope_attn_decode_m", "pppippiipppppipiiiiis", FN {
            return qeft_rope_attn_decode_m(P(a, 0), P(a, 1), P(a, 2), I(a, 3), P(a, 4), P(a, 5), I(a, 6), I(a, 7), P(a, 8), P(a, 9), (const int*)P(a, 10),
                                           (const int*)P(a, 11), P(a, 12), I(a, 13), P(a, 14), I(a, 15), I(a, 16), I(a, 17), I(a, 18), I(a, 19), P(a, 20)); }};
        const Entry ab{"qeft_rope_attn_decode_batch", "pppippiipppppppipiiiiiis", FN {
            return qeft_rope_attn_decode_batch(P(a, 0), P(a, 1), P(a, 2), I(a, 3), P(a, 4), P(a, 5), I(a, 6), I(a, 7), P(a, 8), P(a, 9), (const int*)P(a, 10),
                                               (const int*)P(a, 11), (const int*)P(a, 12), (const int*)P(a, 13), P(a, 14), I(a, 15), P(a, 16), I(a, 17),
                                               I(a, 18), I(a, 19), I(a, 20), I(a, 21), I(a, 22), P(a, 23)); }};
        const Entry a8{"qeft_rope_attn_decode_kv8", "pppippiipppppppppipiiiiiis", FN {
            return qeft_rope_attn_decode_kv8(P(a, 0), P(a, 1), P(a, 2), I(a, 3), P(a, 4), P(a, 5), I(a, 6), I(a, 7), P(a, 8), P(a, 9), P(a, 10), P(a, 11),
                                             (const int*)P(a, 12), (const int*)P(a, 13), (const int*)P(a, 14), (const int*)P(a, 15), P(a, 16), I(a, 17),
                                             P(a, 18), I(a, 19), I(a, 20), I(a, 21), I(a, 22), I(a, 23), I(a, 24), P(a, 25)); }};
        const Entry am8{"qeft_rope_attn_decode_m_kv8", "pppippiipppppppipiiiiis", FN {
            return qeft_rope_attn_decode_m_kv8(P(a, 0), P(a, 1), P(a, 2), I(a, 3), P(a, 4), P(a, 5), I(a, 6), I(a, 7), P(a, 8), P(a, 9), P(a, 10), P(a, 11),
                                               (const int*)P(a, 12), (const int*)P(a, 13), P(a, 14), I(a, 15), P(a, 16), I(a, 17), I(a, 18), I(a, 19),
                                               I(a, 20), I(a, 21), P(a, 22)); }};
        struct Lay { int stride, tab_stride, tab_rows, out_pos, out_stride, ws, split, slots, heads, kv, max_seq, m, done; };
        auto call = [&](const Entry& en, const Lay& L) {
            Args a = operands(en);
            const bool slots = &en == &ab || &en == &a8, scales = &en == &a8 || &en == &am8;
            int i = 8 + 2 + (scales ? 2 : 0);                   // behind the caches (and their scales)
            a[3] = L.stride, a[6] = L.tab_stride, a[7] = L.tab_rows;
            if (slots) { i += 2; if (!L.done) a[i] = 0; ++i; } else ++i;      // slots, pos, done | pos
            if (!L.out_pos) a[i] = 0;
            i += 2;                                             // out_pos, out
            a[i++] = L.out_stride;
            if (!L.ws) a[i] = 0;
            ++i;
            a[i++] = L.split;
            if (slots) a[i++] = L.slots;
            a[i++] = L.heads, a[i++] = L.kv, a[i++] = L.max_seq, a[i++] = L.m;
            return a;
        };
        const int gqa[][2] = {{32, 32}, {32, 8}, {64, 8}, {40, 40}, {8, 1}, {1, 1}};
        for (const Entry* en : {&am, &ab, &a8, &am8}) {
            for (auto& hk : gqa)
                for (int split : {1, 2, 4, 8})
                    for (int m = 1; m <= 8; ++m)
                        for (int max_seq : {16, 4096, 32768})
                            for (int whole_table : {0, 1})
                                for (int out_pos : {0, 1})
                                    for (int ws : {1, 0}) {
                                        if (!ws && split > 1 && m > 2) continue;
                                        const int heads = hk[0], kv = hk[1];
                                        const Lay L{(heads + 2 * kv) * 128, 128, whole_table ? max_seq : m, out_pos, heads * 128, ws, split, 8, heads, kv, max_seq,
                                                    m, out_pos};
                                        record(*en, call(*en, L), nullptr);
                                    }
            const Lay L{6144, 128, 4, 0, 4096, 1, 4, 8, 32, 8, 4096, 4, 1};
            Lay L2 = L, L3 = L;
            L2.split = 1, L2.ws = 0, L2.out_pos = 1, L2.tab_rows = 4096, L2.tab_stride = 64, L2.out_stride = 1;
            L3.heads = 64, L3.m = 8, L3.tab_rows = 8, L3.max_seq = 32768, L3.out_stride = 8192, L3.stride = 10240, L3.done = 0;
            for (const Lay& l : {L, L2, L3}) {
                const Args b = call(*en, l);
                singles(*en, b);
                if (full) pairs(*en, b);
                launcher_errors(*en, b);
            }
        }
        const Entry wm{"qeft_attn_m_workspace_bytes", "iii", FN { return qeft_attn_m_workspace_bytes(I(a, 0), I(a, 1), I(a, 2)); }};
        const Entry wb{"qeft_attn_batch_workspace_bytes", "iii", FN { return qeft_attn_batch_workspace_bytes(I(a, 0), I(a, 1), I(a, 2)); }};
        const Entry w8{"qeft_attn_kv8_workspace_bytes", "iii", FN { return qeft_attn_kv8_workspace_bytes(I(a, 0), I(a, 1), I(a, 2)); }};
        const Entry wm8{"qeft_attn_m_kv8_workspace_bytes", "iii", FN { return qeft_attn_m_kv8_workspace_bytes(I(a, 0), I(a, 1), I(a, 2)); }};
        for (const Entry* en : {&wm, &wb, &w8, &wm8})
            for (int heads : {-1, 0, 1, 8, 32, 40, 64, 4096, 4097})
                for (int split = -1; split <= 9; ++split)
                    for (int m = -1; m <= 9; ++m) record(*en, {heads, split, m}, nullptr);
    }
    fprintf(stderr, "%ld calls recorded, %ld refusals written\n", g_calls, g_refused_rows);
    if (g_refusals) fclose(g_refusals);
    return 0;
}
