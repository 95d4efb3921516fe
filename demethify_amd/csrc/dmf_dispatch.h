// What the launch wrappers of the kernel translation units share: run-time values to template parameters, a kernel's
// dynamic-LDS limit, and the thresholds an experiment build may move.  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

namespace dmf {

// f(std::integral_constant<int, v>{}) for Lo <= v <= Hi (instantiated for every value of the range, in ascending order),
// hipErrorInvalidValue outside it.  f returns hipError_t.
template <int Lo, int Hi, class F>
hipError_t dispatch_int(int v, F&& f) {
    if constexpr (Lo > Hi) {
        return hipErrorInvalidValue;
    } else {
        if (v == Lo) return f(std::integral_constant<int, Lo>{});
        return dispatch_int<Lo + 1, Hi>(v, f);
    }
}

// f(std::true_type{}) or f(std::false_type{})
template <class F>
hipError_t dispatch_bool(bool b, F&& f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}

// Raises Kernel's limit of dynamic LDS to `bytes` (launches above 48 KB need it).  The record of what each device
// already has is per kernel instantiation, so a launch inside the per-iteration loop pays for one hipGetDevice.
template <auto Kernel>
hipError_t raise_dynamic_lds(size_t bytes) {
    static int raised[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if ((int)bytes <= raised[dev]) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) raised[dev] = (int)bytes;
    return e;
}

// A threshold: a named constant in the product.  Only a -DDMF_EXPERIMENT build (DMF_EXPERIMENT=1 python -m
// demethify_amd._build, what tools/wide_nu_sweep.py and tools/gram_i8_vs_fp64.py use for their before / after columns) lets
// the environment move it.
inline int knob(const char* name, int value) {
#ifdef DMF_EXPERIMENT
    if (const char* v = getenv(name)) return atoi(v);
#else
    (void)name;
#endif
    return value;
}

// workgroups per CU of a persistent kernel: an experiment build's override counts when it is positive
inline int per_cu_knob(const char* name, int per_cu) {
    const int v = knob(name, per_cu);
    return v > 0 ? v : per_cu;
}

}  // namespace dmf
