// Recording stand-ins for the three HIP calls the library's launchers make; the other half of tools/capi_record.cpp.
// Force-included in front of every library source (hipcc ... -include tools/capi_record.h): after this header a
// hipLaunchKernelGGL prints the kernel's symbol, grid, block, LDS bytes and every kernel argument instead of launching,
// hipFuncSetAttribute prints its value and succeeds, hipGetLastError returns what capi_record.cpp programmed (success
// unless told otherwise).  Nothing here opens a device.
//
// Operands of a C ABI call are made-up addresses, argument i at (i + 1) << 24 (capi_record.cpp): a kernel pointer argument
// prints as A<i>+<offset>, scalars as values, the argument structs of the GEMV kernels field by field, any other struct as
// its 32-bit words.
#pragma once
#include <hip/hip_runtime.h>

#include <cxxabi.h>
#include <dlfcn.h>
#include <stdint.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>

extern "C" {
extern FILE* capi_rec_out;        // where the current call's launches go (capi_record.cpp)
extern int capi_rec_next_error;   // what the next hipGetLastError() returns; back to hipSuccess after it
extern int capi_rec_hip_calls;    // HIP calls the library has made so far
}

namespace capi_rec {

inline void ptr(const void* p) {
    const unsigned long long v = (unsigned long long)(uintptr_t)p;
    if (v == 0) fprintf(capi_rec_out, "0");
    else if (v >= (1ull << 24) && v < (65ull << 24) && (v & 0xffffff) == 0) fprintf(capi_rec_out, "A%llu", (v >> 24) - 1);
    else if (v >= (1ull << 24) && v < (65ull << 24)) fprintf(capi_rec_out, "A%llu+%llx", (v >> 24) - 1, v & 0xffffff);
    else fprintf(capi_rec_out, "%#llx", v);
}

template <class T, class = void> struct is_gemv_args : std::false_type {};
template <class T> struct is_gemv_args<T, std::void_t<decltype(std::declval<T>().ow_plain), decltype(std::declval<T>().m_rt)>> : std::true_type {};
template <class T, class = void> struct is_gemv_group_args : std::false_type {};
template <class T> struct is_gemv_group_args<T, std::void_t<decltype(std::declval<T>().blk_end), decltype(std::declval<T>().sz_blk)>> : std::true_type {};
template <class T, class = void> struct is_v3_tail : std::false_type {};
template <class T> struct is_v3_tail<T, std::void_t<decltype(std::declval<T>().ssq_in), decltype(std::declval<T>().nsteps), decltype(std::declval<T>().ynorm)>> : std::true_type {};

template <class T> void arg(const T& v);
template <class T> void field(const char* name, const T& v) {
    fprintf(capi_rec_out, " %s=", name);
    arg(v);
}
template <class T, size_t N> void field(const char* name, const T (&v)[N]) {
    fprintf(capi_rec_out, " %s=[", name);
    for (size_t i = 0; i < N; ++i) {
        if (i) fputc(' ', capi_rec_out);
        arg(v[i]);
    }
    fputc(']', capi_rec_out);
}
#define CAPI_REC_F(name) field(#name, v.name)

template <class T> void arg(const T& v) {
    if constexpr (std::is_pointer_v<T>) ptr((const void*)v);
    else if constexpr (std::is_same_v<T, bool>) fprintf(capi_rec_out, v ? "true" : "false");
    else if constexpr (std::is_floating_point_v<T>) fprintf(capi_rec_out, "%a", (double)v);
    else if constexpr (std::is_integral_v<T> || std::is_enum_v<T>) fprintf(capi_rec_out, "%lld", (long long)v);
    else if constexpr (is_gemv_args<T>::value) {
        fprintf(capi_rec_out, "GemvArgs{");
        CAPI_REC_F(x); CAPI_REC_F(qw); CAPI_REC_F(scales); CAPI_REC_F(zeros); CAPI_REC_F(ow_il); CAPI_REC_F(bias); CAPI_REC_F(ids);
        CAPI_REC_F(residual); CAPI_REC_F(y); CAPI_REC_F(N); CAPI_REC_F(K); CAPI_REC_F(G); CAPI_REC_F(n_out); CAPI_REC_F(gshift);
        CAPI_REC_F(xt_aux); CAPI_REC_F(xt_eps); CAPI_REC_F(sz_blk); CAPI_REC_F(dbg); CAPI_REC_F(dbg2); CAPI_REC_F(ow_plain); CAPI_REC_F(m_rt);
        fprintf(capi_rec_out, " }");
    } else if constexpr (is_gemv_group_args<T>::value) {
        fprintf(capi_rec_out, "GemvGroupArgs{");
        CAPI_REC_F(x); CAPI_REC_F(qw); CAPI_REC_F(scales); CAPI_REC_F(zeros); CAPI_REC_F(ow_il); CAPI_REC_F(bias); CAPI_REC_F(y); CAPI_REC_F(N);
        CAPI_REC_F(blk_end); CAPI_REC_F(K); CAPI_REC_F(G); CAPI_REC_F(n_out); CAPI_REC_F(gshift); CAPI_REC_F(xt_aux); CAPI_REC_F(xt_eps);
        CAPI_REC_F(sz_blk);
        fprintf(capi_rec_out, " }");
    } else if constexpr (is_v3_tail<T>::value) {
        fprintf(capi_rec_out, "V3Tail{");
        CAPI_REC_F(ssq_in); CAPI_REC_F(residual); CAPI_REC_F(gamma_out); CAPI_REC_F(bias); CAPI_REC_F(y); CAPI_REC_F(y32); CAPI_REC_F(ynorm);
        CAPI_REC_F(ssq_out); CAPI_REC_F(dbg); CAPI_REC_F(ids); CAPI_REC_F(n_out); CAPI_REC_F(nsteps); CAPI_REC_F(nsets); CAPI_REC_F(n_ssq_in);
        CAPI_REC_F(eps);
        fprintf(capi_rec_out, " }");
    } else {
        static_assert(std::is_trivially_copyable_v<T> && sizeof(T) % 4 == 0, "a kernel argument the recorder cannot print");
        uint32_t w[sizeof(T) / 4];
        memcpy(w, &v, sizeof(T));
        fprintf(capi_rec_out, "struct%zu{", sizeof(T));
        for (size_t i = 0; i < sizeof(T) / 4; ++i) fprintf(capi_rec_out, " %x", w[i]);
        fprintf(capi_rec_out, " }");
    }
}

inline void kernel_name(const void* host_fn, const char* spelled) {
    Dl_info info;
    if (dladdr(host_fn, &info) && info.dli_sname) {
        int status = 0;
        char* d = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &status);
        fprintf(capi_rec_out, "%s", status == 0 && d ? d : info.dli_sname);
        free(d);
    } else {
        fprintf(capi_rec_out, "?%s", spelled);
    }
}

// every argument is printed as the kernel's own parameter type (what the launch converts it to)
template <class... KA, class... A>
void launch(const char* spelled, void (*kern)(KA...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A&&... a) {
    static_assert(sizeof...(KA) == sizeof...(A), "argument count of a launch");
    ++capi_rec_hip_calls;
    fprintf(capi_rec_out, "\n    launch ");
    kernel_name(reinterpret_cast<const void*>(kern), spelled);
    fprintf(capi_rec_out, " grid %u %u %u block %u %u %u lds %zu stream ", grid.x, grid.y, grid.z, block.x, block.y, block.z, lds);
    ptr(st);
    fprintf(capi_rec_out, " args");
    ((fputc(' ', capi_rec_out), arg<std::decay_t<KA>>(static_cast<KA>(a))), ...);
}

template <class F> hipError_t set_attribute(F fn, int attr, int value) {
    ++capi_rec_hip_calls;
    fprintf(capi_rec_out, "\n    attribute ");
    kernel_name(reinterpret_cast<const void*>(fn), "");
    fprintf(capi_rec_out, " %d = %d", attr, value);
    return hipSuccess;
}

inline hipError_t last_error() {
    ++capi_rec_hip_calls;
    const hipError_t e = (hipError_t)capi_rec_next_error;
    capi_rec_next_error = 0;
    return e;
}

}  // namespace capi_rec

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kern, grid, block, lds, st, ...) capi_rec::launch(#kern, kern, grid, block, lds, st, ##__VA_ARGS__)
#define hipFuncSetAttribute(fn, attr, value) capi_rec::set_attribute(fn, (int)(attr), (int)(value))
#define hipGetLastError() capi_rec::last_error()
