// Cross-lane moves inside a 16-lane DPP row, and the argmin butterfly built on them.  Shared by the alpha kernels
// (dmf_kernels_alpha.hip) and the Frank-Wolfe lane of the two batched solver families (dmf_batch.h).
#pragma once
#include <hip/hip_runtime.h>

namespace dmf {

template <int CTRL>
__device__ __forceinline__ int row_mov(int x) {  // permutations, or values masked afterwards: no destination to initialise
    return __builtin_amdgcn_mov_dpp(x, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ double row_mov(double x) {
    const int lo = row_mov<CTRL>(__double2loint(x)), hi = row_mov<CTRL>(__double2hiint(x));
    return __hiloint2double(hi, lo);
}

// value of lane (k ^ J) of the 16-lane row, for a double or an int
template <int J, class T>
__device__ __forceinline__ T row_xor(T x, int k) {
    if constexpr (J == 1) return row_mov<0xB1>(x);       // quad_perm [1, 0, 3, 2]
    else if constexpr (J == 2) return row_mov<0x4E>(x);  // quad_perm [2, 3, 0, 1]
    else if constexpr (J == 8) return row_mov<0x128>(x); // row_ror:8
    else {                                               // J == 4: row_shl:4 for the lower half of an octet
        const T from_above = row_mov<0x104>(x), from_below = row_mov<0x114>(x);
        return (k & 4) ? from_below : from_above;
    }
}

// one butterfly step of a row-wide argmin: lowest index first among equal minima (np.argmin)
template <int J>
__device__ __forceinline__ void argmin_step(double& v, int& idx, int k) {
    const double ov = row_xor<J>(v, k);
    const int oi = row_xor<J>(idx, k);
    const bool take = ov < v || (ov == v && oi < idx);
    v = take ? ov : v;
    idx = take ? oi : idx;
}

}  // namespace dmf
