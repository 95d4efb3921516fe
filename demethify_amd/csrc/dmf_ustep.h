// The row-local inner iteration of the u phase (deconvolution.py:81-90) with lane = (row, unknown type): what its kernels
// share -- the momentum table, the cross-lane and clamp helpers, the three lane layouts of the split form.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "dmf_device.h"
#include "dmf_internal.h"

namespace dmf {

// momentum coefficients beta_t of the n_iter2 inner steps (deconvolution.py:83-85), the same for every row: the recurrence
// itself, by ONE thread (the caller picks it)
__device__ __forceinline__ void fill_momentum_table(const SolverState* __restrict__ state, int n_iter2,
                                                    double* __restrict__ beta_tab) {
    double a1 = state->a1, lw_prev = state->l_w_prev;
    const double lw = state->l_w;
    for (int t2 = 0; t2 < n_iter2; ++t2) {
        double beta;
        momentum_step(a1, lw_prev, lw, beta);
        beta_tab[t2] = beta;
        lw_prev = lw;
    }
}

template <int CTRL>
__device__ __forceinline__ double f_dpp_quad(double x) {
    // mov_dpp, not update_dpp(0, ...): a quad permute has a source in every lane, and an "old" value would
    // cost a v_mov per half to initialise the destination (8 extra instructions per inner step at n_u = 4)
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

template <int NU, int L>
__device__ __forceinline__ double f_group_bcast(double x, int lane0) {
    if constexpr (NU == 1) return x;
    else if constexpr (NU == 2) return f_dpp_quad<(L) | (L << 2) | ((2 + L) << 4) | ((2 + L) << 6)>(x);
    else if constexpr (NU == 4) return f_dpp_quad<L | (L << 2) | (L << 4) | (L << 6)>(x);
    else return __shfl(x, lane0 + L, 64);
}

// clip(a * b + c, 0, 1) in one instruction: the VOP3 clamp modifier clamps an FP result to [0, 1]
// (np.clip(x, 0, 1) of deconvolution.py:88; a NaN would come out as 0 instead of NaN)
__device__ __forceinline__ double f_fma_clamp01(double a, double b, double c) {
    double r;
    asm("v_fma_f64 %0, %1, %2, %3 clamp" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// x of the lane R places further round this lane's row group (NU = 2 or 4 lanes, aligned to a quad)
template <int NU, int R>
__device__ __forceinline__ double f_group_rot(double x) {
    static_assert(NU == 2 || NU == 4, "row groups that tile a quad");
    if constexpr (NU == 2) return f_dpp_quad<1 | (0 << 2) | (3 << 4) | (2 << 6)>(x);
    else return f_dpp_quad<((0 + R) & 3) | (((1 + R) & 3) << 2) | (((2 + R) & 3) << 4) | (((3 + R) & 3) << 6)>(x);
}

// g - sum_l x_l * Mrow[l] over the NU lanes of a row group, l ascending
template <int NU, int L = 0>
__device__ __forceinline__ double grad_row(double g, double base, const double (&Mrow)[NU], int lane0) {
    if constexpr (L < NU) {
        g = fma(-f_group_bcast<NU, L>(base, lane0), Mrow[L], g);
        return grad_row<NU, L + 1>(g, base, Mrow, lane0);
    } else {
        return g;
    }
}

// clip(seed + sum_l x_l * Mn[l], 0, 1) over the NU lanes of a row group as one FMA chain whose last link clamps.
// Under contention from the C waves of its SIMD the phase-B wave pays ~10 cycles per instruction issued,
// dependent or not, so the instruction count (NU FMAs here against NU multiplies + NU adds for a balanced tree
// and a separate clamp) matters more than the depth of the chain.
template <int NU, int L = 0>
__device__ __forceinline__ double f_step_chain(double acc, double x, const double (&Mn)[NU], int lane0) {
    if constexpr (L == NU - 1) {
        return f_fma_clamp01(f_group_bcast<NU, L>(x, lane0), Mn[L], acc);
    } else {
        return f_step_chain<NU, L + 1>(fma(f_group_bcast<NU, L>(x, lane0), Mn[L], acc), x, Mn, lane0);
    }
}

// One accelerated projected-gradient step of a row group (deconvolution.py:83-88): (cur, prev) = (u, u_) in,
// prev = the new u out (cur is then u_).  AT_PREV: gradient at the previous iterate (deconvolution.py:163) instead
// of the extrapolated point (:88).  c and M arrive pre-scaled by 1 / l_w (M negated).
// Ms: this lane's row of -M / l_w in ROTATED order -- Ms[r] = -M[j][(j + r) % NU] / l_w -- with the step's own "+ ut"
// folded into Ms[0] at the extrapolated point (deconvolution.py:88; not at :163, where the gradient point differs).
// A wave alone on its SIMD issues an FP64 instruction every 8 cycles and a 32-bit one every 4 (tools/rowpass2_probe:
// 145 cycles per step for 11 FP64 + 10 other instructions, with or without a second workgroup on the CU), so phase B
// costs what it issues: NU - 1 quad rotations (instead of NU broadcasts) and one FMA chain whose last link clamps --
// 6 FP64 + 8 other instructions per step at NU = 4.
template <int NU, bool AT_PREV>
__device__ __forceinline__ void inner_step(double cur, double& prev, double cj, const double (&Ms)[NU], int b_lo, int b_hi,
                                           int t2, int lane0) {
    const double beta = __hiloint2double(__builtin_amdgcn_readlane(b_hi, t2), __builtin_amdgcn_readlane(b_lo, t2));
    const double ut = fma(beta, cur - prev, cur);
    const double x = AT_PREV ? cur : ut;
    if constexpr (NU == 3) {  // (three lanes per row do not tile a quad: shuffles, in the same rotated order)
        const int jb = (threadIdx.x & 63) - lane0;
        double acc = fma(Ms[0], x, AT_PREV ? ut + cj : cj);
        acc = fma(Ms[1], __shfl(x, lane0 + (jb + 1) % 3, 64), acc);
        prev = f_fma_clamp01(Ms[2], __shfl(x, lane0 + (jb + 2) % 3, 64), acc);
    } else if constexpr (NU == 1) {
        prev = f_fma_clamp01(Ms[0], x, AT_PREV ? ut + cj : cj);
    } else {
        double acc = fma(Ms[0], x, AT_PREV ? ut + cj : cj);
#pragma unroll
        for (int r = 1; r < NU - 1; ++r) acc = fma(Ms[r], r == 1 ? f_group_rot<NU, 1>(x) : f_group_rot<NU, 2>(x), acc);
        prev = f_fma_clamp01(Ms[NU - 1], NU == 2 ? f_group_rot<NU, 1>(x) : f_group_rot<NU, 3>(x), acc);
    }
}

// ONE CpG row per 16-lane DPP row (lane j < NU of the row holds unknown j): the gradient needs lane l's value in every lane
// of the row, which v_fmac_f64_dpp row_newbcast:l delivers inside the multiply-add -- NU instructions per step where a
// row group of shuffles pays 2 NU ds_bpermute round trips (NU = 8: 239 -> 145 us at 5e5 rows and 20 steps).
// (a DPP source written by the previous vector instruction needs two wait states: only the first multiply-add of a
// gradient follows the instruction that produced x)
template <int L>
__device__ __forceinline__ void fmac_row16(double& acc, double x, double m) {
    if constexpr (L == 0)
        asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                     : "+v"(acc)
                     : "v"(x), "v"(m), "n"(L));
    else
        asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                     : "+v"(acc)
                     : "v"(x), "v"(m), "n"(L));
}
template <int NU, int L = 0>
__device__ __forceinline__ void grad_row16(double& g, double base, const double (&Mneg)[NU]) {
    if constexpr (L < NU) {
        fmac_row16<L>(g, base, Mneg[L]);
        grad_row16<NU, L + 1>(g, base, Mneg);
    }
}
// Two DPP rows per CpG row: the gradient's first 16 terms broadcast from the half that holds unknowns 0..15, the rest from
// the other -- row_newbcast within each DPP row, as above.
template <int NU, int L = 0>
__device__ __forceinline__ void grad_row32_lo(double& g, double x, const double (&Mneg)[NU]) {
    if constexpr (L < 16) {
        fmac_row16<L>(g, x, Mneg[L]);
        grad_row32_lo<NU, L + 1>(g, x, Mneg);
    }
}
template <int NU, int L = 16>
__device__ __forceinline__ void grad_row32_hi(double& g, double x, const double (&Mneg)[NU]) {
    if constexpr (L < NU) {
        // (the first of these follows the instruction that selected x: fmac_row16<0> carries the wait states)
        if constexpr (L == 16) fmac_row16<0>(g, x, Mneg[L]);
        else fmac_row16<L - 16>(g, x, Mneg[L]);
        grad_row32_hi<NU, L + 1>(g, x, Mneg);
    }
}

// ---- The lane layouts of the split form: how a wave's 64 lanes map to (row, unknown j), how a lane loads its operands
// from a row of cm = [c_i | packed M_i] (NU + NU (NU + 1) / 2 doubles) and how it takes one step.  Which layout a width
// takes: InnerLanes below.  A layout is built from the lane index: row() is the lane's row of the wave, live() whether the
// lane holds an unknown.  load(..) fetches the operands of global row `grow` (ok: the lane is live and grow < N) and returns
// the lane's index into u / u_, which the kernel loads from -- in every lane, or (kDeadLanesLoadZero) 0.0 where not ok.
// step(ut, base) returns the new u_j from the extrapolated point ut and the gradient point base.  Same per-row arithmetic
// order everywhere -- g = c_j - sum_l M_jl x_l, l ascending -- but NOT the same arithmetic: each layout scales and clamps
// its own way.

// 1..4 unknowns: 64 / NU rows per wave, a row's lanes adjacent.  c_j / l_w and -M_jl / l_w: the step is then one
// multiply-add chain whose last link clamps to [0, 1] (VOP3 clamp), the form of the row pass's phase B (15 instead of 18
// vector instructions per step at four unknowns; 1.15 ms either way at the purity mode's 500 steps and 1e6 rows).
template <int NU>
struct QuadGroup {
    static_assert(NU >= 1 && NU <= 4, "row groups of the broadcasts of f_group_bcast");
    static constexpr int kRowsPerWave = 64 / NU;
    static constexpr bool kDeadLanesLoadZero = false;  // u[gi] unconditionally, from the clamped row
    int rl, j, lane0;  // row of the wave, unknown, first lane of the row group
    double cjs, Ms[NU];
    __device__ __forceinline__ explicit QuadGroup(int lane) : rl(lane / NU), j(lane - rl * NU), lane0(lane - j) {}
    __device__ __forceinline__ int row() const { return rl; }
    __device__ __forceinline__ bool live() const { return rl < kRowsPerWave; }
    __device__ __forceinline__ int64_t load(const double* cm, int64_t grow, int64_t N, bool ok, double inv_lw) {
        constexpr int NV = NU + NU * (NU + 1) / 2;
        const int64_t rowc = ok ? grow : 0;
        const double* __restrict__ mine = cm + rowc * NV;
        cjs = mine[j] * inv_lw;
#pragma unroll
        for (int l = 0; l < NU; ++l) Ms[l] = -inv_lw * mine[NU + (l <= j ? tri(l, j) : tri(j, l))];
        return rowc * NU + j;
    }
    __device__ __forceinline__ double step(double ut, double base) const {
        return f_step_chain<NU>(ut + cjs, base, Ms, lane0);  // clip(ut + (c_j - sum_l M_jl x_l) / l_w, 0, 1)
    }
};

// 5..16 unknowns: one row per DPP row, four per wave.  c_j and -M unscaled; dead lanes (j >= NU) load 0 and are never
// broadcast from.  (k_inner_bu, at 1..16, loads the same operands inside its chunk schedule and takes the static step.)
template <int NU>
struct DppRow {
    static_assert(NU >= 1 && NU <= 16, "one row per DPP row");
    static constexpr int kRowsPerWave = 4;
    static constexpr bool kDeadLanesLoadZero = true;
    int lane, j;
    double cj, Mneg[NU], inv_lw;
    __device__ __forceinline__ explicit DppRow(int lane_) : lane(lane_), j(lane & 15) {}
    __device__ __forceinline__ int row() const { return lane >> 4; }
    __device__ __forceinline__ bool live() const { return j < NU; }
    __device__ __forceinline__ int64_t load(const double* cm, int64_t grow, int64_t N, bool ok, double inv_lw_) {
        constexpr int NV = NU + NU * (NU + 1) / 2;
        const int64_t rowc = grow < N ? grow : 0;
        const int jc = j < NU ? j : 0;
        inv_lw = inv_lw_;
        const double* __restrict__ mine = cm + rowc * NV;
        cj = mine[jc];
#pragma unroll
        for (int l = 0; l < NU; ++l) Mneg[l] = -mine[NU + (l <= jc ? tri(l, jc) : tri(jc, l))];
        return rowc * NU + jc;
    }
    __device__ __forceinline__ double step(double ut, double base) const { return step(ut, base, cj, Mneg, inv_lw); }
    static __device__ __forceinline__ double step(double ut, double base, double cj, const double (&Mneg)[NU],
                                                  double inv_lw) {
        double g = cj;
        grad_row16<NU>(g, base, Mneg);
        return fmin(fmax(fma(g, inv_lw, ut), 0.0), 1.0);
    }
};

// 17..32 unknowns: one row per 32 lanes = two DPP rows (lane j < 16 of the first holds unknown j, of the second unknown
// 16 + j).  Each lane keeps its own iterate value and, exchanged once per step, its partner's 16 lanes away.  Dead lanes
// keep a zero row of M and a zero iterate: the partner reads it.
template <int NU>
struct DppRowPair {
    static_assert(NU > 16 && NU <= 32, "one row per two DPP rows");
    static constexpr int kRowsPerWave = 2;
    static constexpr bool kDeadLanesLoadZero = true;
    int lane, j;
    bool upper;  // second DPP row of the CpG row: unknowns 16..31
    double cj, Mneg[NU], inv_lw;
    __device__ __forceinline__ explicit DppRowPair(int lane_) : lane(lane_), j(lane & 31), upper((lane & 16) != 0) {}
    __device__ __forceinline__ int row() const { return lane >> 5; }
    __device__ __forceinline__ bool live() const { return j < NU; }
    __device__ __forceinline__ int64_t load(const double* cm, int64_t grow, int64_t N, bool ok, double inv_lw_) {
        constexpr int NV = NU + NU * (NU + 1) / 2;
        const int64_t rowc = grow < N ? grow : 0;
        const int jc = j < NU ? j : 0;
        inv_lw = inv_lw_;
        const double* __restrict__ mine = cm + rowc * NV;
        cj = mine[jc];
#pragma unroll
        for (int l = 0; l < NU; ++l) Mneg[l] = j < NU ? -mine[NU + (l <= jc ? tri(l, jc) : tri(jc, l))] : 0.0;
        return rowc * NU + jc;
    }
    __device__ __forceinline__ double step(double ut, double base) const {
        const double other = __shfl_xor(base, 16, 64);  // the partner lane's value (lanes >= NU hold 0)
        const double x_lo = upper ? other : base, x_hi = upper ? base : other;
        double g = cj;
        grad_row32_lo<NU>(g, x_lo, Mneg);
        grad_row32_hi<NU>(g, x_hi, Mneg);
        double uu = fmin(fmax(fma(g, inv_lw, ut), 0.0), 1.0);
        if (j >= NU) uu = 0.0;
        return uu;
    }
};

// the width rule of the split form: rows per workgroup of 4 waves are 4 x (64 / n_u), 16 and 8
template <int NU>
using InnerLanes =
    std::conditional_t<(NU <= 4), QuadGroup<NU>, std::conditional_t<(NU <= 16), DppRow<NU>, DppRowPair<NU>>>;

}  // namespace dmf
