// The consumers of the split u phase: a producer (k_u_phase_mfma in split mode, or k_cm_i8) has left c_i / M_i per row in
// HBM -- N x (n_u + n_u (n_u + 1) / 2) doubles, small next to V and D -- and the inner iterations (the CLI default under
// --purity is 500) run from there with lane = (row, unknown) over the whole chip: k_u_inner_rows, one body for the three
// lane layouts of dmf_ustep.h, and k_inner_bu, the same iterations fused with the b_u stream of the integer Gram route.
#include "dmf_device.h"
#include "dmf_dispatch.h"
#include "dmf_internal.h"
#include "dmf_ustep.h"

namespace dmf {

__global__ void k_beta_table(const SolverState* __restrict__ state, int n_iter2, double* __restrict__ beta_out) {
    if (state->done) return;
    fill_momentum_table(state, n_iter2, beta_out);
}

constexpr int kBetaChunk = 6144;  // momentum coefficients held in LDS at a time (48 KB)

template <class Lanes>
__global__ __launch_bounds__(256) void k_u_inner_rows(const double* __restrict__ cm, const double* __restrict__ beta_g,
                                                      double* __restrict__ u, double* __restrict__ u_prev,
                                                      const SolverState* __restrict__ state, int64_t N, int n_iter2,
                                                      int mode) {
    extern __shared__ double beta_tab[];
    if (state->done) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Lanes at(lane);
    const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * Lanes::kRowsPerWave + at.row();
    const bool ok = at.live() && row < N;
    const double inv_lw = 1.0 / state->l_w;  // as in k_u_phase_mfma
    const int64_t gi = at.load(cm, row, N, ok, inv_lw);
    constexpr bool kEveryLane = !Lanes::kDeadLanesLoadZero;  // the iterate comes in every lane, or 0.0 where the lane is not ok
    double uu = kEveryLane || ok ? u[gi] : 0.0, up = kEveryLane || ok ? u_prev[gi] : 0.0;
    // the momentum coefficients pass through LDS kBetaChunk at a time: any n_iter2 runs (the reference has no limit)
    for (int t0 = 0; t0 < n_iter2; t0 += kBetaChunk) {
        const int nt = n_iter2 - t0 < kBetaChunk ? n_iter2 - t0 : kBetaChunk;
        if (t0 > 0) __syncthreads();  // the previous chunk has been consumed by every wave
        for (int t = threadIdx.x; t < nt; t += 256) beta_tab[t] = beta_g[t0 + t];
        __syncthreads();
        for (int t2 = 0; t2 < nt; ++t2) {
            const double beta = beta_tab[t2];
            const double ut = uu + beta * (uu - up);
            const double base = mode == 1 ? uu : ut;  // deconvolution.py:163 vs :88
            up = uu;
            uu = at.step(ut, base);
        }
    }
    if (ok) {
        u[gi] = uu;
        u_prev[gi] = up;
    }
}

// The inner iterations AND b_u = u^T (D * V) of the rows just finished, in one launch (wide row groups on u16 counts; the
// integer Gram route needs b_u from a stream over V and the counts, k_bu_cols2 as a kernel of its own).  The inner
// iterations are a chain of dependent FP64 instructions with next to no memory traffic, the b_u stream is all memory
// traffic: a workgroup alternates between them on chunks of 16 NSG CpG rows --
//   * all loads of the chunk are issued up front: the rows' c / M (lane = (row, unknown), one row per DPP row, four rows
//     per wave: the DppRow layout of dmf_ustep.h), then the V / count pieces of the b_u stream (lane = two adjacent samples,
//     4 NSG rows per wave), which land while the chains run;
//   * the finished rows go to HBM and into an LDS tile (double buffered: one barrier per chunk);
//   * b_u accumulates per lane over all chunks of the (persistent) workgroup, is summed over the waves at the end and
//     written as one slab per workgroup (layout of k_bu_cols2); the workgroup's share of ||u||_F^2 goes to u2_partials.
// NSG = 128-sample groups (S <= 128 NSG); a workgroup has 4 NSG waves.  Small chunks keep the register count low
// (n_u = 12: ~130): what hides the chains and the load latency is the number of resident workgroups.
constexpr int kInnerBuMaxSteps = 1024;

template <int NU, int NSG, bool ODD>
__global__ __launch_bounds__(256 * NSG) void k_inner_bu(const double* __restrict__ cm, const double* __restrict__ beta_g,
                                                        double* __restrict__ u, double* __restrict__ u_prev,
                                                        const SolverState* __restrict__ state,
                                                        const double* __restrict__ V,
                                                        const unsigned short* __restrict__ D16, int SD, int64_t N, int S,
                                                        int n_iter2, int mode, double* __restrict__ slab,
                                                        double* __restrict__ u2_partials) {
    static_assert(NSG == 1 || NSG == 2, "S <= 256");
    constexpr int NP = NU * (NU + 1) / 2, NV = NU + NP;
    constexpr int NWV = 4 * NSG, kChunk = 16 * NSG, kRows = 4 * NSG;
    constexpr int US = NU + (NU & 1);  // row stride of the LDS tile of finished rows (even: 16-byte reads of pairs)
    typedef double v2d_t __attribute__((ext_vector_type(2)));
    extern __shared__ double lds_ib[];
    double* __restrict__ beta_tab = lds_ib;
    double* __restrict__ u_s = lds_ib + ((n_iter2 + 1) & ~1);  // [2][kChunk][US]
    double* __restrict__ red = u_s + 2 * kChunk * US;          // [NSG][NU][2][64], then [NWV] for ||u||^2
    if (state->done) return;
    for (int t = threadIdx.x; t < n_iter2; t += 256 * NSG) beta_tab[t] = beta_g[t];
    const double inv_lw = 1.0 / state->l_w;  // as in k_u_phase_mfma
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int j = lane & 15, sub = lane >> 4, jc = j < NU ? j : 0;
    const int sg = wave >> 2, wr = wave & 3;
    const int s = sg * 128 + 2 * lane;
    const bool active = s < S;
    // odd S: the row's last sample sits alone in its lane -- its V comes as the upper half of the pair one element lower
    // (never past the end of the row), its partner's count is zero padding; 16-byte loads from 8-byte-aligned addresses:
    // tools/align_probe.hip
    const bool lone = ODD && s == S - 1;
    const int sc = ODD ? (lone ? S - 2 : (active ? s : 0)) : (active ? s : S - 2);
    const int sd = ODD ? (active ? s : 0) : sc;
    typedef double v2d_u __attribute__((ext_vector_type(2), aligned(8)));
    double acc[NU][2];
#pragma unroll
    for (int l = 0; l < NU; ++l) acc[l][0] = acc[l][1] = 0.0;
    double u2 = 0.0;
    __syncthreads();

    const int64_t nchunks = (N + kChunk - 1) / kChunk;
    int it = 0;
    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x, ++it) {
        const int64_t row0 = chunk * kChunk;
        // ---- loads: the chain's operands first (waited for first), then the b_u stream's pieces
        const int64_t row = row0 + wave * 4 + sub;
        const bool ok = j < NU && row < N;
        const int64_t rowc = row < N ? row : 0;
        const double* __restrict__ mine = cm + rowc * NV;
        const double cj = mine[jc];
        double Mneg[NU];
#pragma unroll
        for (int l = 0; l < NU; ++l) Mneg[l] = -mine[NU + (l <= jc ? tri(l, jc) : tri(jc, l))];
        const int64_t gi = rowc * NU + jc;
        double uu = ok ? u[gi] : 0.0, up = ok ? u_prev[gi] : 0.0;
        v2d_t vv[kRows];
        unsigned int dd[kRows];
#pragma unroll
        for (int x = 0; x < kRows; ++x) {
            const int64_t r = row0 + kRows * wr + x;
            const int64_t rc = r < N ? r : N - 1;
            if constexpr (ODD) {
                dd[x] = r < N && active ? *reinterpret_cast<const unsigned int*>(D16 + rc * SD + sd) : 0u;
                const v2d_u vl = *reinterpret_cast<const v2d_u*>(V + rc * S + sc);
                vv[x] = v2d_t{lone ? vl.y : vl.x, vl.y};
            } else {  // (lanes past S accumulate sums nobody reads)
                dd[x] = r < N ? *reinterpret_cast<const unsigned int*>(D16 + rc * SD + sd) : 0u;
                vv[x] = *reinterpret_cast<const v2d_t*>(V + rc * S + sc);
            }
        }
        // ---- the chunk's inner iterations
        for (int t2 = 0; t2 < n_iter2; ++t2) {
            const double beta = beta_tab[t2];
            const double ut = uu + beta * (uu - up);
            const double base = mode == 1 ? uu : ut;  // deconvolution.py:163 vs :88
            up = uu;
            uu = DppRow<NU>::step(ut, base, cj, Mneg, inv_lw);
        }
        double* __restrict__ tile = u_s + (it & 1) * kChunk * US;
        if (ok) {
            u[gi] = uu;
            u_prev[gi] = up;
            u2 = fma(uu, uu, u2);
        }
        if (j < NU) tile[(wave * 4 + sub) * US + j] = ok ? uu : 0.0;
        __syncthreads();  // the tile is complete (and, double buffered, not rewritten before every wave has read it)
        // ---- b_u of this wave's rows
#pragma unroll
        for (int x = 0; x < kRows; ++x) {
            const double t0 = (double)(dd[x] & 0xFFFFu) * vv[x].x;
            const double t1 = (double)(dd[x] >> 16) * vv[x].y;
            const double* __restrict__ ur = tile + (kRows * wr + x) * US;
#pragma unroll
            for (int l = 0; l + 1 < NU; l += 2) {
                const v2d_t u01 = *reinterpret_cast<const v2d_t*>(ur + l);
                acc[l][0] = fma(t0, u01.x, acc[l][0]);
                acc[l][1] = fma(t1, u01.x, acc[l][1]);
                acc[l + 1][0] = fma(t0, u01.y, acc[l + 1][0]);
                acc[l + 1][1] = fma(t1, u01.y, acc[l + 1][1]);
            }
            if constexpr (NU & 1) {
                const double ul = ur[NU - 1];
                acc[NU - 1][0] = fma(t0, ul, acc[NU - 1][0]);
                acc[NU - 1][1] = fma(t1, ul, acc[NU - 1][1]);
            }
        }
    }
    // ---- the workgroup's slab: waves of a sample group summed in wave order
    double* __restrict__ part = red + (size_t)sg * NU * 2 * 64;
    for (int r = 1; r < 4; ++r) {
        __syncthreads();
        if (wr == r) {
#pragma unroll
            for (int l = 0; l < NU; ++l) {
                part[(l * 2 + 0) * 64 + lane] = acc[l][0];
                part[(l * 2 + 1) * 64 + lane] = acc[l][1];
            }
        }
        __syncthreads();
        if (wr == 0) {
#pragma unroll
            for (int l = 0; l < NU; ++l) {
                acc[l][0] += part[(l * 2 + 0) * 64 + lane];
                acc[l][1] += part[(l * 2 + 1) * 64 + lane];
            }
        }
    }
    if (wr == 0 && active) {
#pragma unroll
        for (int l = 0; l < NU; ++l) {
            double* __restrict__ out = slab + ((int64_t)blockIdx.x * NU + l) * S + s;
            out[0] = acc[l][0];
            if (!lone) out[1] = acc[l][1];
        }
    }
    __syncthreads();
    u2 = wave_sum(u2);
    double* __restrict__ u2w = red;  // (the b_u sums have been consumed)
    if (lane == 0) u2w[wave] = u2;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
#pragma unroll
        for (int w = 0; w < NWV; ++w) tot += u2w[w];
        u2_partials[blockIdx.x] = tot;
    }
}

bool u_inner_bu_supported(unsigned v_align, int S, int SD, int n_u, int n_iter2) {
    return n_u >= 1 && n_u <= 16 && S >= 2 && S <= 256 && (SD & 1) == 0 && n_iter2 <= kInnerBuMaxSteps && (v_align & 7) == 0;
}

int u_inner_bu_grid(int64_t N, int S) {
    const int64_t nchunks = S <= 128 ? (N + 15) / 16 : (N + 31) / 32;
    const int64_t cap = S <= 128 ? 2048 : 1024;  // up to eight (four) workgroups of four (eight) waves per CU
    return (int)(nchunks < cap ? (nchunks < 1 ? 1 : nchunks) : cap);
}

// cm + beta as launch_u_inner; slab: u_inner_bu_grid(N, S) x n_u x S doubles; u2_partials: one double per workgroup
static hipError_t launch_u_inner_bu(const ProblemView& p, const IterateView& it, int n_iter2, const UScratch& scratch,
                                    int* grid_out, hipStream_t st) {
    const int S = p.S, n_u = it.n_u;
    if (!u_inner_bu_supported(p.v_align(), S, p.SD, n_u, n_iter2)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_beta_table, dim3(1), dim3(1), 0, st, it.state, n_iter2, scratch.beta);
    const int grid = u_inner_bu_grid(p.N, S);
    *grid_out = grid;
    const int nsg = S <= 128 ? 1 : 2;
    const int us = n_u + (n_u & 1);
    const size_t lds = ((size_t)((n_iter2 + 1) & ~1) + (size_t)2 * 16 * nsg * us + (size_t)nsg * n_u * 2 * 64) * sizeof(double);
    // (1..4: narrow row groups behind the producer: more than 16 known types)
    return dispatch_int<1, 16>(n_u, [&](auto nu) {
        return dispatch_int<1, 2>(nsg, [&](auto nsg_t) {
            return dispatch_bool((S & 1) != 0, [&](auto odd) {
                constexpr int NSG = decltype(nsg_t)::value;
                hipLaunchKernelGGL((k_inner_bu<decltype(nu)::value, NSG, decltype(odd)::value>), dim3((unsigned)grid),
                                   dim3(256 * NSG), lds, st, scratch.cm, scratch.beta, it.u, it.u_prev, it.state, p.V, p.D16,
                                   p.SD, p.N, S, n_iter2, it.mode, scratch.slab, scratch.u2_partials);
                return hipGetLastError();
            });
        });
    });
}

int64_t u_phase_split_cm_doubles(int64_t N, int n_u) { return N * (n_u + (int64_t)n_u * (n_u + 1) / 2); }

// the inner iterations from scratch.cm (N x (n_u + NP) doubles); scratch.beta: n_iter2 doubles of device scratch
static hipError_t launch_u_inner(int64_t N, const IterateView& it, int n_iter2, const UScratch& scratch, hipStream_t st) {
    hipLaunchKernelGGL(k_beta_table, dim3(1), dim3(1), 0, st, it.state, n_iter2, scratch.beta);
    const size_t lds = (size_t)(n_iter2 < kBetaChunk ? n_iter2 : kBetaChunk) * sizeof(double);
    // rows per workgroup of 4 waves: 4 x (64 / n_u) up to four unknowns, 4 x 4 up to sixteen, 4 x 2 beyond (InnerLanes)
    return dispatch_int<1, 32>(it.n_u, [&](auto nu) {
        using Lanes = InnerLanes<decltype(nu)::value>;
        const int64_t rows_per_block = 4 * Lanes::kRowsPerWave;
        const int64_t grid = (N + rows_per_block - 1) / rows_per_block;
        hipLaunchKernelGGL(k_u_inner_rows<Lanes>, dim3((unsigned)grid), dim3(256), lds, st, scratch.cm, scratch.beta, it.u,
                           it.u_prev, it.state, N, n_iter2, it.mode);
        return hipGetLastError();
    });
}

// scratch.cm: N x (n_u + NP) doubles, scratch.beta: n_iter2 doubles (both device scratch owned by the caller)
hipError_t launch_u_phase_split(const ProblemView& p, const IterateView& it, int n_iter2, const UScratch& scratch,
                                hipStream_t st) {
    if (scratch.cm == nullptr || scratch.beta == nullptr) return hipErrorInvalidValue;
    hipError_t e = launch_u_phase_mfma_impl(p, it, n_iter2, scratch.cm, st);
    if (e != hipSuccess) return e;
    return launch_u_inner(p.N, it, n_iter2, scratch, st);
}

// the same with the integer-matrix-core producer of dmf_kernels_cm_i8.hip (n_u <= 16; its preconditions are the caller's)
hipError_t launch_u_phase_split_i8(const ProblemView& p, const IterateView& it, int n_iter2, const UScratch& scratch,
                                   hipStream_t st) {
    if (scratch.cm == nullptr || scratch.beta == nullptr) return hipErrorInvalidValue;
    hipError_t e = launch_cm_i8(p, it, scratch.cm, st);
    if (e != hipSuccess) return e;
    return launch_u_inner(p.N, it, n_iter2, scratch, st);
}

// producer of dmf_kernels_cm_i8.hip, then the inner iterations fused with the b_u stream (k_inner_bu): the whole u phase
// plus b_u and ||u||^2 of the integer Gram route in two launches (+ the momentum table)
hipError_t launch_u_phase_split_i8_bu(const ProblemView& p, const IterateView& it, int n_iter2, const UScratch& scratch,
                                      int* grid_out, hipStream_t st) {
    if (scratch.cm == nullptr || scratch.beta == nullptr || scratch.slab == nullptr || scratch.u2_partials == nullptr)
        return hipErrorInvalidValue;
    hipError_t e = launch_cm_i8(p, it, scratch.cm, st);
    if (e != hipSuccess) return e;
    return launch_u_inner_bu(p, it, n_iter2, scratch, grid_out, st);
}

}  // namespace dmf

