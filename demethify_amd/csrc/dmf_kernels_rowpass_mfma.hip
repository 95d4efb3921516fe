// u phase on the FP64 matrix cores (v_mfma_f64_16x16x4_f64), gfx950.
//
// Same Gram form as dmf_kernels_rowpass.hip (c_i, M_i per row, then n_iter2 row-local steps) but the
// three contractions of the row pass run as MFMAs on 16-row x 16-sample tiles held in the
// "row-on-lane" layout  lane = (row = l & 15, q = l >> 4), register r <-> sample s0 + 4q + r:
//     E^T = V^T - alpha_known^T Rt^T        A = -alpha_known^T (m = sample, k = known type), B = Rt^T, C = V^T
//     c^T += alpha_unk (D*E)^T              A = alpha_unk      (m = unknown j, k = sample),  B = (D*E)^T
//     M^T += P D^T                          A = P (m = pair (j,l), k = sample), P = alpha_unk_j * alpha_unk_l
// (the m <-> sample permutation of the first product is folded into its A operand, so one 32-byte
// contiguous load per lane feeds all three).  The alpha-derived A operands are built once per wave and
// reused for every row block; workgroups are persistent over row blocks.
//
// Layout facts used (verified on hardware with tools/mfma_probe.hip):
//   A[i][k]: lane (i = l & 15, k = l >> 4);  B[k][j]: lane (k = l >> 4, j = l & 15);
//   C/D register r of lane l = C[(l >> 4) + 4 r][l & 15].
// `Rt` here is the problem's padded copy of R_trunc: row stride 4 * NKC doubles, zero pad columns.
#include <cstdlib>
#include <type_traits>

#include "dmf_device.h"
#include "dmf_dispatch.h"
#include "dmf_internal.h"
#include "dmf_ustep.h"

namespace dmf {

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

constexpr int kStripsPerWave = 4;  // 16-sample strips owned by one wave (64 samples)
constexpr int kMfmaMaxWaves = 8;   // S <= 512 on this path


// VEC: S % 4 == 0, so a lane's four samples are contiguous, 32-byte aligned and all in range.
// D16T (with VEC): the counts come from the problem's u16 copy (row stride SD) -- 8 instead of 32 bytes per lane and
// strip, and 8 instead of 32 staging registers for the prefetched strips (with 7 or 8 unknowns the f64 form spills).
template <int NKC, int NU, bool VEC, bool D16T>
__global__ __launch_bounds__(512) void k_u_phase_mfma(
    const double* __restrict__ V, const double* __restrict__ D, const unsigned short* __restrict__ D16, int SD,
    const double* __restrict__ Rt,
    const double* __restrict__ alpha, double* __restrict__ u, double* __restrict__ u_prev,
    const SolverState* __restrict__ state, int64_t N, int S, int n_c, int n_iter2, int mode,
    double* __restrict__ cm_out) {
    // cm_out != nullptr: "split" mode for many inner steps -- the per-row c_i / M_i go to cm_out[row][NU + NP]
    // and k_u_inner_rows runs the inner iterations with every lane of the chip busy, instead of one wave per
    // workgroup doing them here while the others wait.
    constexpr int NP = NU * (NU + 1) / 2;
    constexpr int NMT = (NP + 15) / 16;  // 16-row tiles of the pair matrix
    constexpr int NV = NU + NP;
    extern __shared__ double lds_dyn[];  // beta[n_iter2] then red[2][NW][NV][16]
    if (state->done) return;

    const int NW = blockDim.x >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int m16 = lane & 15, q = lane >> 4;
    const double* __restrict__ A2 = alpha + (int64_t)n_c * S;
    double* __restrict__ beta_tab = lds_dyn;
    double* __restrict__ red = lds_dyn + (cm_out ? 0 : ((n_iter2 + 1) & ~1));

    // momentum coefficients of the n_iter2 inner steps (deconvolution.py:83-85): same for every row
    if (threadIdx.x == 0 && cm_out == nullptr) {  // (fill_momentum_table, written out: the call moves this kernel's registers)
        double a1 = state->a1, lw_prev = state->l_w_prev;
        const double lw = state->l_w;
        for (int t2 = 0; t2 < n_iter2; ++t2) {
            double beta;
            momentum_step(a1, lw_prev, lw, beta);
            beta_tab[t2] = beta;
            lw_prev = lw;
        }
    }
    const double inv_lw = 1.0 / state->l_w;  // x / l_w as x * (1 / l_w): <= 1 ulp from the division

    // ---- per-wave constant A operands (zero for samples >= S and types >= n_c / n_u) ----------
    double a1op[kStripsPerWave][NKC > 0 ? NKC : 1];
    double a2op[kStripsPerWave][4];
    double pop[kStripsPerWave][NMT][4];
    int col0[kStripsPerWave];  // first of this lane's four samples in strip t (clamped into range)
#pragma unroll
    for (int t = 0; t < kStripsPerWave; ++t) {
        const int s0 = (wave * kStripsPerWave + t) * 16;
        // first product: m <-> sample s0 + 4 (m & 3) + (m >> 2), k <-> known type 4 kc + q
        const int s_e = s0 + 4 * (m16 & 3) + (m16 >> 2);
        const int s_ec = s_e < S ? s_e : S - 1;
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc) {
            const int kk = kc * 4 + q;
            const double keep = (kk < n_c && s_e < S) ? -1.0 : 0.0;
            a1op[t][kc] = keep * alpha[(int64_t)(kk < n_c ? kk : 0) * S + s_ec];
        }
        int jp[NMT], lp[NMT];
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) {
            const int p = mt * 16 + m16;
            int l = 0;
            while ((l + 1) * (l + 2) / 2 <= p) ++l;
            jp[mt] = p < NP ? p - l * (l + 1) / 2 : 0;
            lp[mt] = p < NP ? l : 0;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int s = s0 + 4 * q + r;  // k-step r: k = q <-> sample s0 + 4 q + r
            const int sc = s < S ? s : S - 1;
            const double keep2 = (m16 < NU && s < S) ? 1.0 : 0.0;
            a2op[t][r] = keep2 * A2[(int64_t)(m16 < NU ? m16 : 0) * S + sc];
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt) {
                const double keepp = (mt * 16 + m16 < NP && s < S) ? 1.0 : 0.0;
                pop[t][mt][r] = keepp * (A2[(int64_t)jp[mt] * S + sc] * A2[(int64_t)lp[mt] * S + sc]);
            }
        }
        const int c = s0 + 4 * q;
        col0[t] = VEC ? (c < S ? c : 0) : c;
    }
    __syncthreads();  // beta_tab visible

    const int64_t nblk = (N + 15) / 16;
    // Loads are unconditional from clamped addresses: out-of-range samples meet zero A operands and
    // out-of-range rows only feed output columns that are never read, so no masking is needed.
    using DStage = std::conditional_t<D16T, unsigned long long, v4d>;  // a strip's four counts as staged for the next block
    auto load_strip = [&](int64_t rowc, int t, v4d& e, DStage& d) {
        const double* __restrict__ vp = V + rowc * S;
        if constexpr (D16T) {
            static_assert(!D16T || VEC, "the u16 path reads four samples with one 8-byte load");
            const v2d v01 = *reinterpret_cast<const v2d*>(vp + col0[t]);
            const v2d v23 = *reinterpret_cast<const v2d*>(vp + col0[t] + 2);
            e = v4d{v01.x, v01.y, v23.x, v23.y};
            d = *reinterpret_cast<const unsigned long long*>(D16 + rowc * SD + col0[t]);
        } else {
            const double* __restrict__ dp = D + rowc * S;
            if constexpr (VEC) {
                const v2d v01 = *reinterpret_cast<const v2d*>(vp + col0[t]);
                const v2d v23 = *reinterpret_cast<const v2d*>(vp + col0[t] + 2);
                const v2d d01 = *reinterpret_cast<const v2d*>(dp + col0[t]);
                const v2d d23 = *reinterpret_cast<const v2d*>(dp + col0[t] + 2);
                e = v4d{v01.x, v01.y, v23.x, v23.y};
                d = v4d{d01.x, d01.y, d23.x, d23.y};
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = col0[t] + r < S ? col0[t] + r : S - 1;
                    e[r] = vp[c];
                    d[r] = dp[c];
                }
            }
        }
    };
    auto counts_of = [&](const DStage& d) -> v4d {
        if constexpr (D16T) {
            const unsigned int lo = (unsigned int)d, hi = (unsigned int)(d >> 32);
            return v4d{(double)(lo & 0xFFFFu), (double)(lo >> 16), (double)(hi & 0xFFFFu), (double)(hi >> 16)};
        } else {
            return d;
        }
    };
    auto row_of = [&](int64_t blk) {
        const int64_t row = blk * 16 + m16;
        return row < N ? row : N - 1;
    };

    v4d nv[kStripsPerWave];
    DStage nd[kStripsPerWave];
    double nrt[NKC > 0 ? NKC : 1];
    {
        const int64_t rowc = row_of(blockIdx.x);
#pragma unroll
        for (int t = 0; t < kStripsPerWave; ++t) load_strip(rowc, t, nv[t], nd[t]);
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc) nrt[kc] = Rt[rowc * (4 * NKC) + kc * 4 + q];
    }

    int it = 0;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x, ++it) {
        const int64_t row0 = blk * 16;
        const int64_t nxt = blk + gridDim.x < nblk ? blk + gridDim.x : blk;
        const int64_t rowc_n = row_of(nxt);

        // the wave that will run this block's inner iterations fetches its u / u_ now (first pass)
        constexpr int RPW = 64 / NU;  // rows per pass of the inner-iteration phase
        const int rl = lane / NU, j = lane - rl * NU;
        const bool my_turn = cm_out == nullptr && wave == it % NW;
        const bool ok0 = rl < RPW && rl < 16 && row0 + rl < N;
        double uu0 = 0.0, up0 = 0.0;
        if (my_turn) {
            const int64_t gi0 = ok0 ? (row0 + rl) * NU + j : 0;
            uu0 = u[gi0];
            up0 = u_prev[gi0];
        }

        double rtop[NKC > 0 ? NKC : 1];
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc) {
            rtop[kc] = nrt[kc];  // B operand of the first product: Rt^T[k = 4 kc + q][n = row]
            nrt[kc] = Rt[rowc_n * (4 * NKC) + kc * 4 + q];
        }
        v4d cacc = {0.0, 0.0, 0.0, 0.0};
        v4d macc[NMT];
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) macc[mt] = cacc;

#pragma unroll
        for (int t = 0; t < kStripsPerWave; ++t) {
            v4d e = nv[t];
            const v4d d = counts_of(nd[t]);
            load_strip(rowc_n, t, nv[t], nd[t]);  // prefetch the next row block's strip t ...
            __builtin_amdgcn_sched_barrier(0);    // ... and keep it in front of this strip's MFMAs
#pragma unroll
            for (int kc = 0; kc < NKC; ++kc)
                e = __builtin_amdgcn_mfma_f64_16x16x4f64(a1op[t][kc], rtop[kc], e, 0, 0, 0);
            const v4d w = d * e;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                cacc = __builtin_amdgcn_mfma_f64_16x16x4f64(a2op[t][r], w[r], cacc, 0, 0, 0);
#pragma unroll
                for (int mt = 0; mt < NMT; ++mt)
                    macc[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(pop[t][mt][r], d[r], macc[mt], 0, 0, 0);
            }
        }

        // ---- partial c / M of this wave's samples -> LDS (register r' of lane <-> m = q + 4 r')
        double* __restrict__ mine = red + ((size_t)((it & 1) * NW + wave) * NV) * 16;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int m = q + 4 * rr;
            if (m < NU) mine[m * 16 + m16] = cacc[rr];
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt) {
                const int p = mt * 16 + m;
                if (p < NP) mine[(NU + p) * 16 + m16] = macc[mt][rr];
            }
        }
        __syncthreads();

        if (cm_out != nullptr) {  // split mode: fixed-order sum over the waves, one (value, row) per thread
            const double* __restrict__ all = red + ((size_t)(it & 1) * NW * NV) * 16;
            for (int e = threadIdx.x; e < NV * 16; e += blockDim.x) {
                const int v = e >> 4, r = e & 15;
                double tot = 0.0;
                for (int w = 0; w < NW; ++w) tot += all[((size_t)w * NV + v) * 16 + r];
                if (row0 + r < N) cm_out[(row0 + r) * NV + v] = tot;
            }
        }
        // ---- row-local inner iterations by one wave (round robin), lane = (row, unknown j)
        if (my_turn) {
            const double* __restrict__ all = red + ((size_t)(it & 1) * NW * NV) * 16;
            const int lane0 = lane - j;
            for (int pass0 = 0; pass0 < 16; pass0 += RPW) {
                const int rloc = pass0 + rl;
                const bool ok = rl < RPW && rloc < 16 && row0 + rloc < N;
                const int rlc = rloc < 16 ? rloc : 15;
                double cj = 0.0, Mrow[NU];
#pragma unroll
                for (int l = 0; l < NU; ++l) Mrow[l] = 0.0;
                for (int w = 0; w < NW; ++w) {
                    const double* __restrict__ part = all + (size_t)w * NV * 16;
                    cj += part[j * 16 + rlc];
#pragma unroll
                    for (int l = 0; l < NU; ++l) {
                        const int p = l <= j ? tri(l, j) : tri(j, l);
                        Mrow[l] += part[(NU + p) * 16 + rlc];
                    }
                }
                const int64_t gi = ok ? (row0 + rloc) * NU + j : 0;
                double uu = pass0 == 0 ? uu0 : u[gi];
                double up = pass0 == 0 ? up0 : u_prev[gi];
                for (int t2 = 0; t2 < n_iter2; ++t2) {
                    const double beta = beta_tab[t2];
                    const double ut = uu + beta * (uu - up);
                    const double base = mode == 1 ? uu : ut;  // deconvolution.py:163 vs :88
                    up = uu;
                    const double g = grad_row<NU>(cj, base, Mrow, lane0);
                    uu = fmin(fmax(fma(g, inv_lw, ut), 0.0), 1.0);
                }
                if (ok) {
                    u[gi] = uu;
                    u_prev[gi] = up;
                }
            }
        }
    }
}

bool u_phase_mfma_supported(int S, int n_c, int n_u) {
    return n_u >= 1 && n_u <= 8 && n_c <= 16 && S <= 16 * kStripsPerWave * kMfmaMaxWaves;
}

UPhaseMfmaPlan u_phase_mfma_plan(int64_t N, int S, int n_c, int n_u, int n_iter2, bool has_d16, int SD, bool split) {
    UPhaseMfmaPlan g;
    if (N < 1 || S < 1 || n_c < 0 || n_c > 16 || n_u < 1 || n_u > 8 || n_iter2 < 0) return g;
    const int nstrips = (S + 15) / 16;
    g.nw = (nstrips + kStripsPerWave - 1) / kStripsPerWave;
    g.nkc = (n_c + 3) / 4, g.nu = n_u;
    g.vec = (S & 3) == 0;
    g.d16 = g.vec && has_d16 && (SD & 3) == 0;
    g.split = split;
    // persistent workgroups: as many as fit two waves per SIMD (the kernel needs ~250 registers) -- 3 per CU at
    // NW = 2 left a quarter of the wave slots empty
    const int per_cu = per_cu_knob("DMF_UMFMA_PER_CU", g.nw >= 8 ? 1 : 8 / g.nw);
    const int64_t nblk = (N + 15) / 16, cap = (int64_t)256 * per_cu;
    g.grid = (int)(nblk < cap ? nblk : cap);
    g.blocks_per_wg = (nblk + g.grid - 1) / g.grid;
    const int nv = n_u + n_u * (n_u + 1) / 2;
    // (split mode keeps no momentum table in LDS)
    g.lds = ((size_t)(split ? 0 : ((n_iter2 + 1) & ~1)) + (size_t)2 * g.nw * nv * 16) * sizeof(double);
    g.raise = g.lds > 48 * 1024;
    g.supported = g.nw <= kMfmaMaxWaves && g.lds <= 150 * 1024;
    return g;
}

// cm_out: null, or where the split mode leaves the per-row c_i / M_i (see the kernel)
hipError_t launch_u_phase_mfma_impl(const ProblemView& p, const IterateView& it, int n_iter2, double* cm_out, hipStream_t st) {
    const UPhaseMfmaPlan g = u_phase_mfma_plan(p.N, p.S, p.n_c, it.n_u, n_iter2, p.D16 != nullptr, p.SD, cm_out != nullptr);
    if (!g.supported) return hipErrorInvalidValue;
    return dispatch_int<0, 4>(g.nkc, [&](auto nkc) {
        return dispatch_int<1, 8>(g.nu, [&](auto nu) {
            constexpr int NKC = decltype(nkc)::value, NU = decltype(nu)::value;
            const auto launch = [&](auto vec_t, auto d16_t) {
                constexpr auto kernel = k_u_phase_mfma<NKC, NU, decltype(vec_t)::value, decltype(d16_t)::value>;
                if (g.raise) {
                    const hipError_t e = raise_dynamic_lds<kernel>(g.lds);
                    if (e != hipSuccess) return e;
                }
                hipLaunchKernelGGL(kernel, dim3((unsigned)g.grid), dim3(g.nw * 64), g.lds, st, p.V, p.D, p.D16, p.SD, p.Rtp,
                                   it.alpha, it.u, it.u_prev, it.state, p.N, p.S, p.n_c, n_iter2, it.mode, cm_out);
                return hipGetLastError();
            };
            if (g.d16) return launch(std::true_type{}, std::true_type{});
            if (g.vec) return launch(std::true_type{}, std::false_type{});
            return launch(std::false_type{}, std::false_type{});
        });
    });
}

hipError_t launch_u_phase_mfma(const ProblemView& p, const IterateView& it, int n_iter2, hipStream_t st) {
    return launch_u_phase_mfma_impl(p, it, n_iter2, nullptr, st);
}

}  // namespace dmf
