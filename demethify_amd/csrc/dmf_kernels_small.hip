// k_solve_small: one workgroup is one solve.  The whole outer loop of mdwbssmf_deconv (demethify/deconvolution.py:190-223)
// or unsupervised_deconv (:107-184) runs inside the kernel for problems small enough that a launch per phase is nothing
// but launch latency: 1 <= n_u <= 4, K = n_c + n_u <= 16, S <= 64, N S <= 2^20.  The grid is B solves of one resident
// problem; solve b has its own (u0, alpha0) and optionally its own row list idx[b][0..N): row i of the solve is row
// idx[b][i] of the problem, read through the index (a bootstrap replicate, bootstrap.py:28, without a gathered copy).
//
// Plan of one outer iteration (DESIGN.md sections 3 and 6.2), 256 threads:
//   u phase     a thread per row: c_i = sum_s d (v - Rt_i A_known) A_unk and M_i = sum_s d A_unk A_unk^T in registers, then
//               the n_iter2 inner steps on those n_u + n_u (n_u + 1) / 2 numbers (:81-90; the gradient at u_temp in
//               partial mode, at the previous iterate in unsupervised mode, :163)
//   l_h         (||R_trunc||^2 + ||u||^2) d (:212)
//   Gram        threads as (row slice r, sample s): the entries of G_s = R^T diag(d_s) R and b_s = R^T diag(d_s) v_s that
//               involve u, kBatchChunk accumulators per pass over the rows, the slices added in rising order; the
//               known x known block is formed once per solve and kept in the workspace
//   alpha phase a thread per sample on its K x K Gram in LDS: n_iter2 steps with the sort-based projection (:93-102, :21-37)
//   l_w         ||alpha[-n_u:]||^2 d (:216)
//   cf          sum d (v - R alpha)^2 over the rows, streaming (:15-17), and the stop test |cf - cf_0| < tol on it (:220)
//
// Determinism: a thread adds its rows in rising order, thread partials are added by one fixed tree, slices in rising
// order -- every order depends on (N, S, n_c, n_u) alone.  No atomics; a workgroup reads nothing another one writes, so
// a solve's result does not depend on B, on its slot or on what else is resident.  All state a later launch needs goes to
// the workspace (dmf_small.h) before the kernel returns, so a solve continues bit for bit however the iterations are cut
// into launches.
//
// LDS: G and b (K (K + 1) / 2 + K rows of SP doubles, SP = S rounded up to a power of two), alpha, alpha_, the
// extrapolated point and the sort scratch (4 K SP), 32 KB of reduction scratch, the job tables: 141 KB at S = 64, K = 16,
// 40 KB for the 350 x 10 example with 5 + 1 types.
//
// The purity variant (PURITY; mdwbssmf_deconv_p, :306-337) keeps the u phase, the Gram, l_w, the cost and the stop test and
// replaces the alpha phase by n_iter2 Frank-Wolfe steps per sample (frank_wolfe_nmf, :280-302) on the same G_s, b_s: one
// sample per 16-lane row, lane k owning row k of G_s in registers, the 16 rows of the workgroup taking samples r, r + 16, ...
// There is no a2, no l_h and no alpha_; the purity vector is an input, not state.
//
// The masked variant (MASK; a bi-cross-validation fold, ic.py:58-89) gives solve b a train mask of its own, packed as
// dmf_problem_mask packs it: wherever the kernel reads a count d_is -- the set-up maximum, the known Gram block, c_i and M_i,
// gram_rows, stream_cost and so the stop test -- it is 0 where the bit is 0 (upstream's counts * train_mask); v of a held-out
// element is still read and only ever multiplied by that 0.  The bits are read from memory, not kept in LDS.  MASK is a
// template parameter: the instances without it are the code they were.  k_small_mask_count (before the first launch) counts a
// solve's kept elements, k_small_holdout (after the last) takes the squared error on the held-out ones.
#include "dmf_small.h"

namespace dmf {

namespace {

constexpr int kJobShorts = 3 * kBatchMaxJobs + 8;  // jk, jl, jd (padded to 8 bytes)

struct Lds {
    double* gb;     // [K (K + 1) / 2 + K][SP]: packed G (row l (l + 1) / 2 + k, k <= l), then b
    double* a;      // [K][SP] alpha
    double* ap;     // [K][SP] alpha_
    double* tmp;    // [K][SP] alpha_temp
    double* srt;    // [K][SP] sort scratch
    double* red;    // [kBatchChunk * 256] reduction scratch
    double* sh;     // [8] broadcast slots
    short* jk;      // job tables: x_k, x_l over (R_trunc columns, u columns, v) and the row of gb
    short* jl;
    short* jd;
};

// The purity-constrained alpha phase (deconvolution.py:280-302) on the G_s, b_s of m.gb, alpha in m.a: row r of the
// workgroup's 16 sixteen-lane rows runs the whole chain (frank_wolfe_lane) of samples r, r + 16, ...; every loop bound is
// uniform over the workgroup, so the DPP moves always find their row complete.
__device__ void frank_wolfe_rows(const Lds& m, const double* __restrict__ purity, int S, int n_c, int K, int SP, int n_pairs,
                                 int64_t n_steps) {
    const int t = threadIdx.x, k = t & 15, row = t >> 4;
    for (int s0 = 0; s0 < S; s0 += kBatchThreads / 16) {
        const int s = s0 + row;
        const double a = frank_wolfe_lane<false>(m.gb, m.a, purity, k, s, S, n_c, K, SP, n_pairs, n_steps);
        if (s < S && k < K) m.a[k * SP + s] = a;
    }
}

}  // namespace

template <int NU, bool PURITY, bool MASK>
__global__ __launch_bounds__(kBatchThreads) void k_solve_small(SmallArgs a) {
    static_assert(!(PURITY && MASK), "a purity run with a mask is not built");
    const int64_t b = blockIdx.x;
    if (!a.first && a.done[b]) return;  // a finished solve's workgroup returns at once
    extern __shared__ double small_lds[];
    const int t = threadIdx.x;
    const int S = a.S, n_c = a.n_c, K = n_c + NU, SP = pow2_at_least(S);
    const int n_pairs = K * (K + 1) / 2;
    Lds m;
    m.gb = small_lds;
    m.a = m.gb + (n_pairs + K) * SP;
    m.ap = m.a + K * SP;
    m.tmp = m.ap + K * SP;
    m.srt = m.tmp + K * SP;
    m.red = m.srt + K * SP;
    m.sh = m.red + kBatchChunk * kBatchThreads;
    m.jk = reinterpret_cast<short*>(m.sh + 8);
    m.jl = m.jk + kBatchMaxJobs;
    m.jd = m.jl + kBatchMaxJobs;

    const int64_t N = a.N;
    double* u = a.u + b * N * NU;
    double* u_prev = a.u_prev + b * N * NU;
    double* ws_alpha = a.alpha + b * K * S;
    double* ws_alpha_prev = a.alpha_prev + b * K * S;
    const int n_known = known_jobs(n_c);
    double* gk = a.gk + b * (int64_t)n_known * S;
    double* ratio_u = a.ratio + b * 2 * a.n_iter2;
    double* ratio_h = ratio_u + a.n_iter2;
    double* scal = a.scal + b * kBatchScalars;

    RowRange p;  // all rows of the solve
    p.V = a.V, p.D = a.D, p.Rt = a.Rt;
    p.idx = a.idx != nullptr ? a.idx + b * N : nullptr;
    p.u = u;
    p.lo = 0, p.hi = N, p.S = S, p.n_c = n_c, p.n_u = NU, p.K = K, p.SP = SP, p.R = kBatchThreads / SP;
    p.nb = (S + 7) / 8;
    p.mask = MASK ? a.mask + b * N * p.nb : nullptr;

    // job tables: the known block (pairs of R_trunc columns in packed order, then their products with v), then what
    // involves u (the packed rows l >= n_c, then b_u): fill_jobs' two tables in one, written out -- with two fill_jobs calls
    // the purity restarts of the 350 x 10 example measured 0.5 % beyond the parent's own repeatability, twice
    // (profiles/batch_shared_bodies.txt)
    if (t == 0) {
        int j = 0;
        for (int l = 0; l < n_c; ++l)
            for (int k = 0; k <= l; ++k) m.jk[j] = (short)k, m.jl[j] = (short)l, m.jd[j] = (short)(l * (l + 1) / 2 + k), ++j;
        for (int k = 0; k < n_c; ++k) m.jk[j] = (short)k, m.jl[j] = (short)K, m.jd[j] = (short)(n_pairs + k), ++j;
        for (int l = n_c; l < K; ++l)
            for (int k = 0; k <= l; ++k) m.jk[j] = (short)k, m.jl[j] = (short)l, m.jd[j] = (short)(l * (l + 1) / 2 + k), ++j;
        for (int k = n_c; k < K; ++k) m.jk[j] = (short)k, m.jl[j] = (short)K, m.jd[j] = (short)(n_pairs + k), ++j;
    }
    const int n_jobs = n_pairs + K;
    const GramToLds to_gb{m.gb, m.jd, SP};

    double a1, a2, l_w, l_w_prev, l_h, l_h_prev, dsq, rt_norm2, cf;
    long long iters;
    if (a.first) {
        // deconvolution.py:192-204: a1 = a2 = 1, u_ = u, alpha_ = alpha, d = max(D)^2 over the solve's rows, l_w, l_h, cf
        const double* u0 = a.u0 + b * N * NU;
        const double* alpha0 = a.alpha0 + b * K * S;
        for (int e = t; e < K * S; e += kBatchThreads) {
            const int k = e / S, s = e - k * S;
            if constexpr (PURITY) m.a[k * SP + s] = alpha0[e];
            else m.a[k * SP + s] = m.ap[k * SP + s] = alpha0[e];
        }
        double u2 = 0.0, rt2 = 0.0, dmax = -INFINITY;
        for (int64_t i = t; i < N; i += kBatchThreads) {
#pragma unroll
            for (int j = 0; j < NU; ++j) {
                const double x = u0[i * NU + j];
                u[i * NU + j] = u_prev[i * NU + j] = x;
                u2 = fma(x, x, u2);
            }
            const int64_t g = p.row(i);
            for (int k = 0; k < n_c; ++k) rt2 = fma(p.Rt[g * n_c + k], p.Rt[g * n_c + k], rt2);
        }
        {
            const int s = t & (SP - 1), r = t / SP;
            if (s < S)
                for (int64_t i = r; i < N; i += p.R) {
                    if constexpr (MASK) {  // the maximum over the kept elements (D.max() of counts * train_mask)
                        if (p.kept(i, s)) dmax = fmax(dmax, p.D[i * S + s]);
                    } else {
                        dmax = fmax(dmax, p.D[p.row(i) * S + s]);
                    }
                }
        }
        dmax = block_max(dmax, m.red);
        dsq = dmax * dmax;
        rt_norm2 = block_sum(rt2, m.red);
        u2 = block_sum(u2, m.red);  // (its barriers also publish u and the job tables)
        l_w = l_w_prev = alpha_u_norm2(m.a, n_c, NU, S, SP, m.red) * dsq;
        l_h = l_h_prev = (rt_norm2 + u2) * dsq;
        a1 = a2 = 1.0;
        iters = 0;
        gram_rows<MASK>(p, m.jk, m.jl, 0, n_known, m.red, to_gb);
        for (int e = t; e < n_known * S; e += kBatchThreads) {
            const int j = e / S, s = e - j * S;
            gk[e] = m.gb[(int)m.jd[j] * SP + s];
        }
        cf = stream_cost<MASK>(p, m.a, m.red);
    } else {
        for (int e = t; e < K * S; e += kBatchThreads) {
            const int k = e / S, s = e - k * S;
            m.a[k * SP + s] = ws_alpha[e];
            if constexpr (!PURITY) m.ap[k * SP + s] = ws_alpha_prev[e];
        }
        __syncthreads();  // (the job tables)
        for (int e = t; e < n_known * S; e += kBatchThreads) {
            const int j = e / S, s = e - j * S;
            m.gb[(int)m.jd[j] * SP + s] = gk[e];
        }
        a1 = scal[kBsA1], a2 = scal[kBsA2], l_w = scal[kBsLw], l_w_prev = scal[kBsLwPrev], l_h = scal[kBsLh];
        l_h_prev = scal[kBsLhPrev], dsq = scal[kBsDsq], rt_norm2 = scal[kBsRtNorm2], cf = scal[kBsCf];
        iters = a.iters[b];
        __syncthreads();
    }

    const int64_t T2 = a.n_iter2;
    int done = 0;
    for (int it = 0; it < a.n_run; ++it) {
        // the momentum ratios of both phases
        if (t == 0 || (!PURITY && t == 64)) {
            const bool u_phase = t == 0;
            m.sh[u_phase ? 0 : 1] = fill_ratios(u_phase ? a1 : a2, u_phase ? ratio_u : ratio_h, T2);
        }
        __syncthreads();
        a1 = m.sh[0];
        if constexpr (!PURITY) a2 = m.sh[1];

        // ---- u phase (:81-90)
        const double cap_w = 0.9999 * sqrt(l_w_prev / l_w);
        double u2 = 0.0;
        for (int64_t i = t; i < N; i += kBatchThreads)
            u2 = u_phase_row<NU, MASK>(p, i, m.a, ratio_u, T2, cap_w, l_w, a.mode, u, u_prev, u2);
        if (T2 > 0) l_w_prev = l_w;
        u2 = block_sum(u2, m.red);  // (its barriers publish u to the workgroup)
        if constexpr (!PURITY) l_h = (rt_norm2 + u2) * dsq;  // :212

        // ---- the u-dependent entries of the per-sample Grams
        gram_rows<MASK>(p, m.jk, m.jl, n_known, n_jobs, m.red, to_gb);

        // ---- alpha phase: Frank-Wolfe under the purity constraint (:280-302), else (:93-102) thread s owns column s
        if constexpr (PURITY) {
            frank_wolfe_rows(m, a.purity, S, n_c, K, SP, n_pairs, T2);
        } else if (t < S) {
            alpha_column_steps(m.gb, m.a, m.ap, m.tmp, m.srt, t, K, SP, n_pairs, ratio_h, T2, l_h_prev, l_h);
        }
        if (T2 > 0) l_h_prev = l_h;
        __syncthreads();
        l_w = alpha_u_norm2(m.a, n_c, NU, S, SP, m.red) * dsq;  // :216

        // ---- cost and stop test (:218-220)
        const double cf_0 = cf;
        cf = stream_cost<MASK>(p, m.a, m.red);
        ++iters;
        if (fabs(cf - cf_0) < a.tol) {
            done = 1;
            break;
        }
    }

    // everything the next launch (or the host) reads
    for (int e = t; e < K * S; e += kBatchThreads) {
        const int k = e / S, s = e - k * S;
        ws_alpha[e] = m.a[k * SP + s];
        if constexpr (!PURITY) ws_alpha_prev[e] = m.ap[k * SP + s];
    }
    if (t == 0) {
        scal[kBsA1] = a1, scal[kBsA2] = a2, scal[kBsLw] = l_w, scal[kBsLwPrev] = l_w_prev, scal[kBsLh] = l_h;
        scal[kBsLhPrev] = l_h_prev, scal[kBsDsq] = dsq, scal[kBsRtNorm2] = rt_norm2, scal[kBsCf] = cf;
        a.iters[b] = iters;
        a.done[b] = done;
    }
}

// n_train[b] = the set bits among the N x S real positions of mask b: thread t counts rows t, t + 256, ..., the 256 integer
// partials are added by one fixed tree.  Bits of samples >= S in a row's last byte are padding and not counted.
__global__ __launch_bounds__(kBatchThreads) void k_small_mask_count(const uint8_t* __restrict__ mask, int64_t N, int S,
                                                                    long long* __restrict__ n_train) {
    __shared__ long long part[kBatchThreads];
    const int t = threadIdx.x, nb = (S + 7) / 8;
    const uint8_t* mb = mask + (int64_t)blockIdx.x * N * nb;
    const unsigned int last = (S & 7) ? (1u << (S & 7)) - 1u : 0xFFu;  // the real bits of a row's last byte
    long long n = 0;
    for (int64_t i = t; i < N; i += kBatchThreads)
        for (int q = 0; q < nb; ++q) n += __popc((unsigned int)mb[i * nb + q] & (q == nb - 1 ? last : 0xFFu));
    part[t] = n;
    __syncthreads();
    for (int off = kBatchThreads / 2; off > 0; off >>= 1) {
        if (t < off) part[t] += part[t + off];
        __syncthreads();
    }
    if (t == 0) n_train[blockIdx.x] = part[0];
}

// sum_sq[b] = sum over the held-out elements (bit 0) of (v - [Rt | u_b] alpha_b)^2 on the problem's full V: threads as
// (row slice r, sample s) like stream_cost, a thread adds its rows in rising order, the partials go through block_sum's tree.
__global__ __launch_bounds__(kBatchThreads) void k_small_holdout(const double* __restrict__ V, const double* __restrict__ Rt,
                                                                 const double* __restrict__ u, const double* __restrict__ alpha,
                                                                 const uint8_t* __restrict__ mask, int64_t N, int S, int n_c,
                                                                 int n_u, double* __restrict__ sum_sq) {
    __shared__ double al[kBatchMaxK * kBatchMaxS];
    __shared__ double red[kBatchThreads];
    const int64_t b = blockIdx.x;
    const int t = threadIdx.x, K = n_c + n_u, SP = pow2_at_least(S), nb = (S + 7) / 8, R = kBatchThreads / SP;
    for (int e = t; e < K * S; e += kBatchThreads) al[e] = alpha[b * K * S + e];
    __syncthreads();
    const double* ub = u + b * N * n_u;
    const uint8_t* mb = mask + b * N * nb;
    const int s = t & (SP - 1), r = t / SP;
    double acc = 0.0;
    if (s < S) {
        for (int64_t i = r; i < N; i += R) {
            if ((mb[i * nb + (s >> 3)] >> (s & 7)) & 1) continue;
            double resid = V[i * S + s];
            for (int k = 0; k < n_c; ++k) resid = fma(-Rt[i * n_c + k], al[k * S + s], resid);
            for (int j = 0; j < n_u; ++j) resid = fma(-ub[i * n_u + j], al[(n_c + j) * S + s], resid);
            acc = fma(resid, resid, acc);
        }
    }
    const double total = block_sum(acc, red);
    if (t == 0) sum_sq[b] = total;
}

hipError_t launch_small_mask_count(const uint8_t* mask, int64_t B, int64_t N, int S, long long* n_train, hipStream_t st) {
    if (mask == nullptr || n_train == nullptr || B < 1 || B > 0x7fffffff || N < 1 || S < 1 || S > kBatchMaxS)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_small_mask_count, dim3((unsigned)B), dim3(kBatchThreads), 0, st, mask, N, S, n_train);
    return hipGetLastError();
}

hipError_t launch_small_holdout(const double* V, const double* Rt, const double* u, const double* alpha, const uint8_t* mask,
                                int64_t B, int64_t N, int S, int n_c, int n_u, double* sum_sq, hipStream_t st) {
    if (V == nullptr || u == nullptr || alpha == nullptr || mask == nullptr || sum_sq == nullptr || B < 1 || B > 0x7fffffff ||
        !batch_supported(N, S, n_c, n_u, DMF_MODE_PARTIAL, kSmallMaxElements) || (n_c > 0 && Rt == nullptr))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_small_holdout, dim3((unsigned)B), dim3(kBatchThreads), 0, st, V, Rt, u, alpha, mask, N, S, n_c, n_u,
                       sum_sq);
    return hipGetLastError();
}

size_t small_lds_bytes(int S, int K) {
    const int SP = pow2_at_least(S);
    const size_t doubles = (size_t)(K * (K + 1) / 2 + K) * SP + 4 * (size_t)K * SP + kBatchChunk * kBatchThreads + 8;
    return doubles * sizeof(double) + (kJobShorts * sizeof(short) + 7) / 8 * 8;
}

template <int NU, bool PURITY, bool MASK = false>
static hipError_t launch_nu(const SmallArgs& a, int64_t B, size_t lds, hipStream_t st) {
    static bool raised = false;
    const hipError_t e = raise_lds_limit(reinterpret_cast<const void*>(&k_solve_small<NU, PURITY, MASK>), lds, &raised);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_solve_small<NU, PURITY, MASK>), dim3((unsigned)B), dim3(kBatchThreads), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_solve_small(const SmallArgs& a, int64_t B, hipStream_t st) {
    if (!batch_supported(a.N, a.S, a.n_c, a.n_u, a.mode, kSmallMaxElements) || B < 1 || B > 0x7fffffff) return hipErrorInvalidValue;
    const size_t lds = small_lds_bytes(a.S, a.n_c + a.n_u);
    if (a.purity != nullptr) {  // the purity variant: partial mode with a known block to hold at that mass
        if (a.mode != DMF_MODE_PARTIAL || a.n_c < 1 || a.mask != nullptr) return hipErrorInvalidValue;
        switch (a.n_u) {
            case 1: return launch_nu<1, true>(a, B, lds, st);
            case 2: return launch_nu<2, true>(a, B, lds, st);
            case 3: return launch_nu<3, true>(a, B, lds, st);
            default: return launch_nu<4, true>(a, B, lds, st);
        }
    }
    if (a.mask != nullptr) {  // a train mask per solve: neither a row list nor the purity variant goes with it
        if (a.idx != nullptr) return hipErrorInvalidValue;
        switch (a.n_u) {
            case 1: return launch_nu<1, false, true>(a, B, lds, st);
            case 2: return launch_nu<2, false, true>(a, B, lds, st);
            case 3: return launch_nu<3, false, true>(a, B, lds, st);
            default: return launch_nu<4, false, true>(a, B, lds, st);
        }
    }
    switch (a.n_u) {
        case 1: return launch_nu<1, false>(a, B, lds, st);
        case 2: return launch_nu<2, false>(a, B, lds, st);
        case 3: return launch_nu<3, false>(a, B, lds, st);
        default: return launch_nu<4, false>(a, B, lds, st);
    }
}

}  // namespace dmf
