// What the two batched solver families mean the same thing by: the one-launch batch (k_solve_small, dmf_small.h; DESIGN.md
// section 6.2) and the mid-size batch (the k_mid_* kernels, dmf_mid.h; section 6.3).  The common envelope, the per-solve
// scalars and kernel arguments, and the device bodies of the solver arithmetic, each written once over a row range
// [lo, hi) of a solve: the one-launch batch passes all N rows, the mid-size batch a slab.  Included by the four batch
// translation units (dmf_kernels_small.hip, dmf_kernels_mid.hip, dmf_api_small.hip, dmf_api_mid.hip) and nothing else.
//
// Determinism, for every body below: a thread adds its rows in rising order, thread partials go through one fixed tree,
// row slices are added in rising order.  No atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/demethify_hip.h"
#include "dmf_rowlanes.h"

namespace dmf {

// the envelope both families share (dmf_solve_small_supported, dmf_solve_mid_supported); each keeps its own bound on N S
constexpr int kBatchMaxS = 64, kBatchMaxK = 16, kBatchMaxNu = 4;
constexpr int kBatchThreads = 256;
constexpr int kBatchChunk = 16;  // Gram accumulators per pass over the rows
constexpr int kBatchMaxJobs = kBatchMaxK * (kBatchMaxK + 1) / 2 + kBatchMaxK;  // 152
constexpr int kRowsInFlight = 4;  // rows a thread of the (slice, sample) passes loads before it uses any
// a solve's scalars in the workspace; kBsCf: the one-launch batch keeps the current cost there, the mid-size batch the cost
// BEFORE the one its cost partials hold
enum BatchScalar { kBsA1, kBsA2, kBsLw, kBsLwPrev, kBsLh, kBsLhPrev, kBsDsq, kBsRtNorm2, kBsCf, kBatchScalars = 16 };

inline bool batch_supported(int64_t N, int64_t S, int64_t n_c, int64_t n_u, int mode, int64_t max_elements) {
    if (mode != DMF_MODE_PARTIAL && mode != DMF_MODE_UNSUPERVISED) return false;
    if (N < 1 || S < 1 || S > kBatchMaxS || n_c < 0 || n_u < 1 || n_u > kBatchMaxNu || n_c + n_u > kBatchMaxK) return false;
    return N <= max_elements / S;
}

// jobs per sample: the known block (pairs of R_trunc columns and their products with v) and what involves u
__host__ __device__ inline int known_jobs(int n_c) { return n_c * (n_c + 1) / 2 + n_c; }
__host__ __device__ inline int u_jobs(int n_c, int n_u) {
    const int K = n_c + n_u;
    return K * (K + 1) / 2 + K - known_jobs(n_c);
}

__host__ __device__ inline int pow2_at_least(int s) {
    int p = 1;
    while (p < s) p <<= 1;
    return p;
}

// The head of either family's kernel arguments: the resident problem, the caller's starts and the shape.  All read only.
// SmallArgs and MidArgs go on with their own fields and the workspace arrays; what both have there carries the same name
// in both (tol, u, u_prev, alpha, alpha_prev, gk, ratio, scal, iters, done), each at the place it always had in its struct:
// where the kernel arguments lie decides how the compiler loads them, and with another order k_mid_alpha takes 77 VGPRs
// for 44 (profiles/batch_shared_bodies.txt).
struct BatchArgs {
    const double* V = nullptr;        // N_src x S
    const double* D = nullptr;        // N_src x S
    const double* Rt = nullptr;       // N_src x n_c
    const long long* idx = nullptr;   // B x N row indices into the problem, or null: the problem's own rows
    const double* u0 = nullptr;       // B x N x n_u
    const double* alpha0 = nullptr;   // B x K x S
    int64_t N = 0;
    int S = 0, n_c = 0, n_u = 0, mode = 0;
    int64_t n_iter2 = 0;
};

// ---- device bodies.  Reductions over the workgroup's 256 threads through one fixed tree in LDS (red: 256 doubles); not
// dmf_device.h's wave version, which adds in a different order
__device__ __forceinline__ double block_sum(double x, double* red) {
    const int t = threadIdx.x;
    red[t] = x;
    __syncthreads();
#pragma unroll
    for (int off = kBatchThreads / 2; off > 0; off >>= 1) {
        if (t < off) red[t] += red[t + off];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ double block_max(double x, double* red) {
    const int t = threadIdx.x;
    red[t] = x;
    __syncthreads();
#pragma unroll
    for (int off = kBatchThreads / 2; off > 0; off >>= 1) {
        if (t < off) red[t] = fmax(red[t], red[t + off]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// Rows [lo, hi) of one solve: what a workgroup reads of the problem and of the solve.
struct RowRange {
    const double* V;
    const double* D;
    const double* Rt;
    const long long* idx;  // this solve's row list, or null: the identity
    const double* u;       // this solve's current u
    const uint8_t* mask;   // this solve's train mask (the MASK instances): nb bytes per row
    int64_t lo, hi;
    int S, n_c, n_u, K, SP, R, nb;
    __device__ __forceinline__ int64_t row(int64_t i) const { return idx != nullptr ? (int64_t)idx[i] : i; }
    // is element (i, s) kept?  The bits are read from memory (at most 128 KB per solve: they stay in L2)
    __device__ __forceinline__ bool kept(int64_t i, int s) const { return (mask[i * nb + (s >> 3)] >> (s & 7)) & 1; }
};

// The job tables: x_k, x_l over (R_trunc columns, u columns, v = column K) and the packed row of G / b the product goes to.
// known: the pairs of R_trunc columns, then their products with v; else what involves u (the packed rows l >= n_c, then
// b_u).  Returns the number of jobs.
__device__ inline int fill_jobs(short* jk, short* jl, short* jd, int n_c, int K, bool known) {
    const int n_pairs = K * (K + 1) / 2;
    int j = 0;
    const int l0 = known ? 0 : n_c, l1 = known ? n_c : K;
    for (int l = l0; l < l1; ++l)
        for (int k = 0; k <= l; ++k) jk[j] = (short)k, jl[j] = (short)l, jd[j] = (short)(l * (l + 1) / 2 + k), ++j;
    for (int k = l0; k < l1; ++k) jk[j] = (short)k, jl[j] = (short)K, jd[j] = (short)(n_pairs + k), ++j;
    return j;
}

// the momentum ratios (a_{t-1} - 1) / a_t of one phase's next n steps (deconvolution.py:83-84, :95-96): they do not depend
// on the data; returns a_n
__device__ inline double fill_ratios(double am, double* ratio, int64_t n) {
    for (int64_t q = 0; q < n; ++q) {
        const double an = (1.0 + sqrt(1.0 + 4.0 * am * am)) / 2.0;
        ratio[q] = (am - 1.0) / an;
        am = an;
    }
    return am;
}

// Where gram_rows puts a finished job's sum: row jd[job] of the packed G / b in LDS, stride SP (padding columns included) ...
struct GramToLds {
    double* gb;
    const short* jd;
    int SP;
    __device__ __forceinline__ bool takes(int) const { return true; }
    __device__ __forceinline__ void put(int job, int so, double sum) const { gb[(int)jd[job] * SP + so] = sum; }
};
// ... or row `job` of a slab's partials in memory, stride S
struct GramToMemory {
    double* __restrict__ out;
    int S;
    __device__ __forceinline__ bool takes(int so) const { return so < S; }
    __device__ __forceinline__ void put(int job, int so, double sum) const { out[(int64_t)job * S + so] = sum; }
};

// Jobs [j0, j1) of the tables (jk, jl): sum_i d_is x_k x_l over the rows of the range, handed to `to`.  Threads as (slice r,
// sample s); slice r adds rows lo + r, lo + r + R, ... in rising order, the slices are added in rising order.  MASK: d is 0
// where the solve's bit is.  (The tables and the scratch by reference, as members of a caller's struct arrive: by value,
// k_solve_small<1, false, *> takes 2 and 3 VGPRs more; profiles/batch_shared_bodies.txt.  Check with tools/kernel_regs.sh.)
template <bool MASK, class Sink>
__device__ inline void gram_rows(const RowRange& p, const short* const& jk, const short* const& jl, int j0, int j1,
                                 double* const& red, const Sink& to) {
    const int t = threadIdx.x;
    const int s = t & (p.SP - 1), r = t / p.SP;
    const bool active = s < p.S;
    for (int base = j0; base < j1; base += kBatchChunk) {
        const int nj = min(kBatchChunk, j1 - base);
        double acc[kBatchChunk];
#pragma unroll
        for (int j = 0; j < kBatchChunk; ++j) acc[j] = 0.0;
        if (active) {
            // kRowsInFlight rows per trip, so that their loads are in flight together (one wave per SIMD hides no latency);
            // a row past the end reads row i again with weight 0: acc + 0, the sums and their order are the same
            for (int64_t i = p.lo + r; i < p.hi; i += (int64_t)kRowsInFlight * p.R) {
                double d[kRowsInFlight], v[kRowsInFlight];
                const double* rt[kRowsInFlight];
                const double* ui[kRowsInFlight];
#pragma unroll
                for (int q = 0; q < kRowsInFlight; ++q) {
                    const int64_t iq = i + (int64_t)q * p.R;
                    const bool in = iq < p.hi;
                    const int64_t ic = in ? iq : i, g = p.row(ic);
                    if constexpr (MASK) d[q] = in && p.kept(g, s) ? p.D[g * p.S + s] : 0.0;
                    else d[q] = in ? p.D[g * p.S + s] : 0.0;
                    v[q] = p.V[g * p.S + s];
                    rt[q] = p.Rt + g * p.n_c;
                    ui[q] = p.u + ic * p.n_u;
                }
#pragma unroll
                for (int j = 0; j < kBatchChunk; ++j) {
                    if (j < nj) {
                        const int k = jk[base + j], l = jl[base + j];
#pragma unroll
                        for (int q = 0; q < kRowsInFlight; ++q) {
                            const double xk = k < p.n_c ? rt[q][k] : ui[q][k - p.n_c];
                            const double xl = l < p.n_c ? rt[q][l] : (l < p.K ? ui[q][l - p.n_c] : v[q]);
                            acc[j] = fma(d[q] * xk, xl, acc[j]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kBatchChunk; ++j) red[(j * p.R + r) * p.SP + s] = acc[j];
        __syncthreads();
        for (int o = t; o < nj * p.SP; o += kBatchThreads) {
            const int j = o / p.SP, so = o & (p.SP - 1);
            if (to.takes(so)) {
                double sum = 0.0;
                for (int rr = 0; rr < p.R; ++rr) sum += red[(j * p.R + rr) * p.SP + so];
                to.put(base + j, so, sum);
            }
        }
        __syncthreads();
    }
}

// sum_i sum_s d (v - [Rt | u] alpha)^2 over the rows of the range with alpha (K x SP) from LDS (deconvolution.py:15-17);
// MASK as above
template <bool MASK>
__device__ inline double stream_cost(const RowRange& p, const double* al, double* red) {
    const int t = threadIdx.x;
    const int s = t & (p.SP - 1), r = t / p.SP;
    double acc = 0.0;
    if (s < p.S) {
        for (int64_t i = p.lo + r; i < p.hi; i += (int64_t)kRowsInFlight * p.R) {  // (rows in flight as in gram_rows)
            double d[kRowsInFlight], resid[kRowsInFlight];
            const double* rt[kRowsInFlight];
            const double* ui[kRowsInFlight];
#pragma unroll
            for (int q = 0; q < kRowsInFlight; ++q) {
                const int64_t iq = i + (int64_t)q * p.R;
                const bool in = iq < p.hi;
                const int64_t ic = in ? iq : i, g = p.row(ic);
                if constexpr (MASK) d[q] = in && p.kept(g, s) ? p.D[g * p.S + s] : 0.0;
                else d[q] = in ? p.D[g * p.S + s] : 0.0;
                resid[q] = p.V[g * p.S + s];
                rt[q] = p.Rt + g * p.n_c;
                ui[q] = p.u + ic * p.n_u;
            }
            for (int k = 0; k < p.n_c; ++k) {
                const double ak = al[k * p.SP + s];
#pragma unroll
                for (int q = 0; q < kRowsInFlight; ++q) resid[q] = fma(-rt[q][k], ak, resid[q]);
            }
            for (int j = 0; j < p.n_u; ++j) {
                const double aj = al[(p.n_c + j) * p.SP + s];
#pragma unroll
                for (int q = 0; q < kRowsInFlight; ++q) resid[q] = fma(-ui[q][j], aj, resid[q]);
            }
#pragma unroll
            for (int q = 0; q < kRowsInFlight; ++q) acc = fma(d[q] * resid[q], resid[q], acc);
        }
    }
    return block_sum(acc, red);
}

// The u phase of row i of the solve (deconvolution.py:81-90): c_i = sum_s d (v - Rt_i A_known) A_unk and
// M_i = sum_s d A_unk A_unk^T in registers with alpha (K x SP) from LDS, then the T2 inner steps on those
// NU + NU (NU + 1) / 2 numbers, the gradient at u_temp in partial mode and at the previous iterate in unsupervised mode
// (:163).  Replaces the row in u and u_prev; returns u2 with the new row's squares added.  MASK: d is 0 where the bit is.
template <int NU, bool MASK>
__device__ __forceinline__ double u_phase_row(const RowRange& p, int64_t i, const double* al, const double* ratio_u, int64_t T2,
                                              double cap_w, double l_w, int mode, double* u, double* u_prev, double u2) {
    constexpr int NP = NU * (NU + 1) / 2;
    const int S = p.S, n_c = p.n_c, SP = p.SP;
    const int64_t g = p.row(i);
    double rt[kBatchMaxK - 1];
#pragma unroll
    for (int k = 0; k < kBatchMaxK - 1; ++k) rt[k] = k < n_c ? p.Rt[g * n_c + k] : 0.0;
    double c[NU], M[NP];
#pragma unroll
    for (int j = 0; j < NU; ++j) c[j] = 0.0;
#pragma unroll
    for (int q = 0; q < NP; ++q) M[q] = 0.0;
    const double* Vr = p.V + g * S;
    const double* Dr = p.D + g * S;
    unsigned long long bits = 0;  // the row's train bits, sample s in bit s (S <= 64)
    if constexpr (MASK)
        for (int q = 0; q < p.nb; ++q) bits |= (unsigned long long)p.mask[g * p.nb + q] << (8 * q);
#pragma unroll 4
    for (int s = 0; s < S; ++s) {
        double d = Dr[s];
        if constexpr (MASK) d = (bits >> s) & 1 ? d : 0.0;
        double x = Vr[s];
#pragma unroll
        for (int k = 0; k < kBatchMaxK - 1; ++k)
            if (k < n_c) x = fma(-rt[k], al[k * SP + s], x);
        x *= d;
        double au[NU];
#pragma unroll
        for (int j = 0; j < NU; ++j) au[j] = al[(n_c + j) * SP + s];
#pragma unroll
        for (int l = 0; l < NU; ++l) {
            c[l] = fma(x, au[l], c[l]);
            const double dl = d * au[l];
#pragma unroll
            for (int j = 0; j <= l; ++j) M[l * (l + 1) / 2 + j] = fma(dl, au[j], M[l * (l + 1) / 2 + j]);
        }
    }
    double uc[NU], up[NU];
#pragma unroll
    for (int j = 0; j < NU; ++j) uc[j] = u[i * NU + j], up[j] = u_prev[i * NU + j];
    for (int64_t q = 0; q < T2; ++q) {
        const double beta = fmin(ratio_u[q], q == 0 ? cap_w : 0.9999);
        double ut[NU], at[NU];
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            ut[j] = fma(beta, uc[j] - up[j], uc[j]);
            at[j] = mode == DMF_MODE_UNSUPERVISED ? uc[j] : ut[j];  // where the gradient is taken (:163)
        }
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            double gr = c[j];
#pragma unroll
            for (int l = 0; l < NU; ++l) gr = fma(-M[j <= l ? l * (l + 1) / 2 + j : j * (j + 1) / 2 + l], at[l], gr);
            up[j] = uc[j];
            uc[j] = fmin(fmax(ut[j] + gr / l_w, 0.0), 1.0);
        }
    }
#pragma unroll
    for (int j = 0; j < NU; ++j) {
        u[i * NU + j] = uc[j], u_prev[i * NU + j] = up[j];
        u2 = fma(uc[j], uc[j], u2);
    }
    return u2;
}

// deconvolution.py:21-37 on column s of x (K values, stride SP), srt: the column's sort scratch
__device__ inline void project_column_lds(double* x, double* srt, int K, int SP) {
    for (int k = 0; k < K; ++k) {  // insertion sort, descending
        const double v = x[k * SP];
        int j = k;
        while (j > 0 && srt[(j - 1) * SP] < v) {
            srt[j * SP] = srt[(j - 1) * SP];
            --j;
        }
        srt[j * SP] = v;
    }
    double run = 0.0, theta = 0.0, last_shift = 0.0;
    bool any = false;
    for (int j = 0; j < K; ++j) {
        run += srt[j * SP];
        const double shifted = run - 1.0;
        if (srt[j * SP] - shifted / (double)(j + 1) > 0.0) {
            theta = shifted / (double)(j + 1);
            any = true;
        }
        last_shift = shifted;
    }
    if (!any) theta = last_shift / 0.0;  // upstream: rho = -1 -> pi[-1] / 0 (non-finite input only)
    for (int k = 0; k < K; ++k) x[k * SP] = fmax(x[k * SP] - theta, 0.0);
}

// The T2 projected-gradient alpha steps of column s (deconvolution.py:93-102) on the packed G_s, b_s of gb (n_pairs rows of
// G, then b): al, ap, tmp, srt are alpha, alpha_, alpha_temp and the sort scratch, K x SP each; the calling thread owns the
// column
__device__ __forceinline__ void alpha_column_steps(const double* gb, double* al, double* ap, double* tmp, double* srt, int s,
                                                   int K, int SP, int n_pairs, const double* ratio_h, int64_t T2,
                                                   double l_h_prev, double l_h) {
    const double cap_h = 0.9999 * sqrt(l_h_prev / l_h);
    for (int64_t q = 0; q < T2; ++q) {
        const double beta = fmin(ratio_h[q], q == 0 ? cap_h : 0.9999);
        for (int k = 0; k < K; ++k) {
            const double ak = al[k * SP + s];
            tmp[k * SP + s] = fma(beta, ak - ap[k * SP + s], ak);
            ap[k * SP + s] = ak;
        }
        for (int k = 0; k < K; ++k) {
            double gr = gb[(n_pairs + k) * SP + s];
            for (int l = 0; l < K; ++l) {
                const int q2 = k <= l ? l * (l + 1) / 2 + k : k * (k + 1) / 2 + l;
                gr = fma(-gb[q2 * SP + s], tmp[l * SP + s], gr);
            }
            al[k * SP + s] = tmp[k * SP + s] + gr / l_h;
        }
        project_column_lds(al + s, srt + s, K, SP);
    }
}

// ||alpha[n_c:]||^2 of alpha (K x SP) in LDS, over all 256 threads
__device__ __forceinline__ double alpha_u_norm2(const double* al, int n_c, int n_u, int S, int SP, double* red) {
    double w2 = 0.0;
    for (int e = threadIdx.x; e < n_u * S; e += kBatchThreads) {
        const int j = e / S, s = e - j * S;
        w2 = fma(al[(n_c + j) * SP + s], al[(n_c + j) * SP + s], w2);
    }
    return block_sum(w2, red);
}

// g4[l % 4] += G[l] a[lane l of the row] for l = L .. 15, in this order (row_newbcast:l; four chains as in
// k_alpha_frank_wolfe_row16)
template <int L = 0>
__device__ __forceinline__ void gram_row_times_a(double (&g4)[4], double a, const double (&G)[16]) {
    if constexpr (L < 16) {
        g4[L & 3] = fma(G[L], row_mov<0x150 + L>(a), g4[L & 3]);
        gram_row_times_a<L + 1>(g4, a, G);
    }
}

// a = (1 - gamma) a + gamma vertex as numpy evaluates it: two products and a sum, each rounded (:299-300)
__device__ __forceinline__ double frank_wolfe_update(double a, double gamma, double vertex) {
#pragma clang fp contract(off)
    const double keep = (1.0 - gamma) * a, move = gamma * vertex;
    return keep + move;
}

// The purity-constrained alpha phase (deconvolution.py:280-302) of sample s as lane k of the sample's 16-lane row sees it, on
// the packed G_s, b_s of gb and alpha (al), K x SP in LDS: the known block keeps mass purity[s] and the unknown block mass
// 1 - purity[s]; step it moves by 2 / (it + 2) towards the vertex with the smallest gradient entry of each block, lowest index
// first among equal minima (np.argmin).  grad = G a - b, row k of G_s in registers.  Returns the lane's alpha after n_steps
// steps: the caller stores it where k < K and s < S (other lanes run on clamped indices, so that the DPP moves find
// their row complete: n_steps and the caller's loops must be uniform over the wave).  BARRIER: a workgroup barrier between the
// loads and the steps, for a caller whose lanes replace alpha while others may still be reading theirs.
template <bool BARRIER>
__device__ __forceinline__ double frank_wolfe_lane(const double* gb, const double* al, const double* __restrict__ purity, int k,
                                                   int s, int S, int n_c, int K, int SP, int n_pairs, int64_t n_steps) {
    const bool row_ok = k < K, known = k < n_c, unknown = row_ok && !known;
    const int kc = row_ok ? k : K - 1, sc = s < S ? s : S - 1;
    double Grow[16];
#pragma unroll
    for (int l = 0; l < 16; ++l) {
        const int lc = l < K ? l : K - 1;
        const int lo = kc < lc ? kc : lc, hi = kc < lc ? lc : kc;
        const double v = gb[(hi * (hi + 1) / 2 + lo) * SP + sc];
        Grow[l] = (row_ok && l < K) ? v : 0.0;
    }
    const double bk = row_ok ? gb[(n_pairs + kc) * SP + sc] : 0.0;
    const double pur = purity[sc];
    const double mass = known ? pur : 1.0 - pur;  // what this lane's vertex would put on row k
    double a = row_ok ? al[kc * SP + sc] : 0.0;
    if constexpr (BARRIER) __syncthreads();
    for (int64_t it = 0; it < n_steps; ++it) {
        double g4[4] = {-bk, 0.0, 0.0, 0.0};
        gram_row_times_a(g4, a, Grow);
        const double grad = (g4[0] + g4[1]) + (g4[2] + g4[3]);
        double v1 = known ? grad : INFINITY, v2 = unknown ? grad : INFINITY;
        int i1 = k, i2 = k;
        argmin_step<1>(v1, i1, k); argmin_step<2>(v1, i1, k); argmin_step<4>(v1, i1, k); argmin_step<8>(v1, i1, k);
        argmin_step<1>(v2, i2, k); argmin_step<2>(v2, i2, k); argmin_step<4>(v2, i2, k); argmin_step<8>(v2, i2, k);
        const double gamma = 2.0 / (double)(it + 2);
        const bool at_vertex = (known && k == i1) || (unknown && k == i2);
        a = frank_wolfe_update(a, gamma, at_vertex ? mass : 0.0);
    }
    return a;
}

// ---- for the two launchers: more than 64 KB of dynamic LDS need the kernel's limit raised, once per kernel (*raised: the
// caller's flag for it)
inline hipError_t raise_lds_limit(const void* kernel, size_t lds, bool* raised) {
    if (lds > 64 * 1024 && !*raised) {
        const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        *raised = true;
    }
    return hipSuccess;
}

}  // namespace dmf
