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
//               involve u, kSmallChunk accumulators per pass over the rows, the slices added in rising order; the
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
// gram_jobs, stream_cost and so the stop test -- it is 0 where the bit is 0 (upstream's counts * train_mask); v of a held-out
// element is still read and only ever multiplied by that 0.  The bits are read from memory, not kept in LDS.  MASK is a
// template parameter: the instances without it are the code they were.  k_small_mask_count (before the first launch) counts a
// solve's kept elements, k_small_holdout (after the last) takes the squared error on the held-out ones.
#include "dmf_small.h"
#include "dmf_rowlanes.h"

#include "../../include/demethify_hip.h"

namespace dmf {

namespace {

constexpr int kMaxJobs = kSmallMaxK * (kSmallMaxK + 1) / 2 + kSmallMaxK;  // 152
constexpr int kJobShorts = 3 * kMaxJobs + 8;                               // jk, jl, jd (padded to 8 bytes)
constexpr int kRowsInFlight = 4;  // rows a thread of the (slice, sample) passes loads before it uses any

__host__ __device__ inline int pow2_at_least(int s) {
    int p = 1;
    while (p < s) p <<= 1;
    return p;
}

struct Lds {
    double* gb;     // [K (K + 1) / 2 + K][SP]: packed G (row l (l + 1) / 2 + k, k <= l), then b
    double* a;      // [K][SP] alpha
    double* ap;     // [K][SP] alpha_
    double* tmp;    // [K][SP] alpha_temp
    double* srt;    // [K][SP] sort scratch
    double* red;    // [kSmallChunk * 256] reduction scratch
    double* sh;     // [8] broadcast slots
    short* jk;      // job tables: x_k, x_l over (R_trunc columns, u columns, v) and the row of gb
    short* jl;
    short* jd;
};

__device__ __forceinline__ double block_sum(double x, double* red) {
    const int t = threadIdx.x;
    red[t] = x;
    __syncthreads();
#pragma unroll
    for (int off = kSmallThreads / 2; off > 0; off >>= 1) {
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
    for (int off = kSmallThreads / 2; off > 0; off >>= 1) {
        if (t < off) red[t] = fmax(red[t], red[t + off]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// What a solve reads of the problem and of itself.
struct Rows {
    const double* V;
    const double* D;
    const double* Rt;
    const long long* idx;  // null: the identity
    const double* u;       // this solve's current u
    const uint8_t* mask;   // this solve's train mask (the MASK instances): nb bytes per row
    int64_t N;
    int S, n_c, n_u, K, SP, R, nb;
    __device__ __forceinline__ int64_t row(int64_t i) const { return idx != nullptr ? (int64_t)idx[i] : i; }
    // is element (i, s) kept?  The bits are read from memory (at most 128 KB per solve: they stay in L2)
    __device__ __forceinline__ bool kept(int64_t i, int s) const { return (mask[i * nb + (s >> 3)] >> (s & 7)) & 1; }
};

// Jobs [j0, j1) of the job tables: gb[jd][s] = sum_i d_is x_k x_l over the solve's rows.  Threads as (slice r, sample s);
// slice r adds rows r, r + R, ... in rising order, the slices are added in rising order.  MASK: d is 0 where the solve's bit is.
template <bool MASK>
__device__ void gram_jobs(const Rows& p, const Lds& m, int j0, int j1) {
    const int t = threadIdx.x;
    const int s = t & (p.SP - 1), r = t / p.SP;
    const bool active = s < p.S;
    for (int base = j0; base < j1; base += kSmallChunk) {
        const int nj = min(kSmallChunk, j1 - base);
        double acc[kSmallChunk];
#pragma unroll
        for (int j = 0; j < kSmallChunk; ++j) acc[j] = 0.0;
        if (active) {
            // kRowsInFlight rows per trip, so that their loads are in flight together (one wave per SIMD hides no latency);
            // a row past the end reads row i again with weight 0: acc + 0, the sums and their order are the same
            for (int64_t i = r; i < p.N; i += (int64_t)kRowsInFlight * p.R) {
                double d[kRowsInFlight], v[kRowsInFlight];
                const double* rt[kRowsInFlight];
                const double* ui[kRowsInFlight];
#pragma unroll
                for (int q = 0; q < kRowsInFlight; ++q) {
                    const int64_t iq = i + (int64_t)q * p.R;
                    const bool in = iq < p.N;
                    const int64_t ic = in ? iq : i, g = p.row(ic);
                    if constexpr (MASK) d[q] = in && p.kept(g, s) ? p.D[g * p.S + s] : 0.0;
                    else d[q] = in ? p.D[g * p.S + s] : 0.0;
                    v[q] = p.V[g * p.S + s];
                    rt[q] = p.Rt + g * p.n_c;
                    ui[q] = p.u + ic * p.n_u;
                }
#pragma unroll
                for (int j = 0; j < kSmallChunk; ++j) {
                    if (j < nj) {
                        const int k = m.jk[base + j], l = m.jl[base + j];
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
        for (int j = 0; j < kSmallChunk; ++j) m.red[(j * p.R + r) * p.SP + s] = acc[j];
        __syncthreads();
        for (int o = t; o < nj * p.SP; o += kSmallThreads) {
            const int j = o / p.SP, so = o & (p.SP - 1);
            double sum = 0.0;
            for (int rr = 0; rr < p.R; ++rr) sum += m.red[(j * p.R + rr) * p.SP + so];
            m.gb[(int)m.jd[base + j] * p.SP + so] = sum;
        }
        __syncthreads();
    }
}

// sum_i sum_s d (v - [Rt | u] alpha)^2 over the solve's rows with alpha from LDS (deconvolution.py:15-17); MASK as above
template <bool MASK>
__device__ double stream_cost(const Rows& p, const Lds& m) {
    const int t = threadIdx.x;
    const int s = t & (p.SP - 1), r = t / p.SP;
    double acc = 0.0;
    if (s < p.S) {
        for (int64_t i = r; i < p.N; i += (int64_t)kRowsInFlight * p.R) {  // (rows in flight as in gram_jobs)
            double d[kRowsInFlight], resid[kRowsInFlight];
            const double* rt[kRowsInFlight];
            const double* ui[kRowsInFlight];
#pragma unroll
            for (int q = 0; q < kRowsInFlight; ++q) {
                const int64_t iq = i + (int64_t)q * p.R;
                const bool in = iq < p.N;
                const int64_t ic = in ? iq : i, g = p.row(ic);
                if constexpr (MASK) d[q] = in && p.kept(g, s) ? p.D[g * p.S + s] : 0.0;
                else d[q] = in ? p.D[g * p.S + s] : 0.0;
                resid[q] = p.V[g * p.S + s];
                rt[q] = p.Rt + g * p.n_c;
                ui[q] = p.u + ic * p.n_u;
            }
            for (int k = 0; k < p.n_c; ++k) {
                const double ak = m.a[k * p.SP + s];
#pragma unroll
                for (int q = 0; q < kRowsInFlight; ++q) resid[q] = fma(-rt[q][k], ak, resid[q]);
            }
            for (int j = 0; j < p.n_u; ++j) {
                const double aj = m.a[(p.n_c + j) * p.SP + s];
#pragma unroll
                for (int q = 0; q < kRowsInFlight; ++q) resid[q] = fma(-ui[q][j], aj, resid[q]);
            }
#pragma unroll
            for (int q = 0; q < kRowsInFlight; ++q) acc = fma(d[q] * resid[q], resid[q], acc);
        }
    }
    return block_sum(acc, m.red);
}

// deconvolution.py:21-37 on column s of x (K values, stride SP), srt: the column's sort scratch
__device__ void project_column_lds(double* x, double* srt, int K, int SP) {
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

// The purity-constrained alpha phase (deconvolution.py:280-302) on the G_s, b_s of m.gb, alpha in m.a: per sample the known
// block keeps mass purity[s] and the unknown block mass 1 - purity[s]; step k moves by 2 / (k + 2) towards the vertex with
// the smallest gradient entry of each block, lowest index first among equal minima (np.argmin).  grad = G a - b.  Row r
// of the workgroup's 16 sixteen-lane rows runs the whole chain of samples r, r + 16, ...; every loop bound is uniform over
// the workgroup, so the DPP moves always find their row complete.
__device__ void frank_wolfe_rows(const Lds& m, const double* __restrict__ purity, int S, int n_c, int K, int SP, int n_pairs,
                                 int64_t n_steps) {
    const int t = threadIdx.x, k = t & 15, row = t >> 4;
    const bool row_ok = k < K, known = k < n_c, unknown = row_ok && !known;
    const int kc = row_ok ? k : K - 1;
    for (int s0 = 0; s0 < S; s0 += kSmallThreads / 16) {
        const int s = s0 + row;
        const bool col_ok = s < S;
        const int sc = col_ok ? s : S - 1;
        double Grow[16];
#pragma unroll
        for (int l = 0; l < 16; ++l) {
            const int lc = l < K ? l : K - 1;
            const int lo = kc < lc ? kc : lc, hi = kc < lc ? lc : kc;
            const double v = m.gb[(hi * (hi + 1) / 2 + lo) * SP + sc];
            Grow[l] = (row_ok && l < K) ? v : 0.0;
        }
        const double bk = row_ok ? m.gb[(n_pairs + kc) * SP + sc] : 0.0;
        const double pur = purity[sc];
        const double mass = known ? pur : 1.0 - pur;  // what this lane's vertex would put on row k
        double a = row_ok ? m.a[kc * SP + sc] : 0.0;
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
        if (col_ok && row_ok) m.a[k * SP + s] = a;
    }
}

}  // namespace

template <int NU, bool PURITY, bool MASK>
__global__ __launch_bounds__(kSmallThreads) void k_solve_small(SmallArgs a) {
    static_assert(!(PURITY && MASK), "a purity run with a mask is not built");
    constexpr int NP = NU * (NU + 1) / 2;
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
    m.sh = m.red + kSmallChunk * kSmallThreads;
    m.jk = reinterpret_cast<short*>(m.sh + 8);
    m.jl = m.jk + kMaxJobs;
    m.jd = m.jl + kMaxJobs;

    const int64_t N = a.N;
    double* u = a.u + b * N * NU;
    double* u_prev = a.u_prev + b * N * NU;
    double* ws_alpha = a.alpha + b * K * S;
    double* ws_alpha_prev = a.alpha_prev + b * K * S;
    const int n_known = (int)small_known_jobs(n_c);
    double* gk = a.gk + b * (int64_t)n_known * S;
    double* ratio_u = a.ratio + b * 2 * a.n_iter2;
    double* ratio_h = ratio_u + a.n_iter2;
    double* scal = a.scal + b * kSmallScalars;

    Rows p;
    p.V = a.V, p.D = a.D, p.Rt = a.Rt;
    p.idx = a.idx != nullptr ? a.idx + b * N : nullptr;
    p.u = u;
    p.N = N, p.S = S, p.n_c = n_c, p.n_u = NU, p.K = K, p.SP = SP, p.R = kSmallThreads / SP;
    p.nb = (S + 7) / 8;
    p.mask = MASK ? a.mask + b * N * p.nb : nullptr;

    // job tables: the known block (pairs of R_trunc columns in packed order, then their products with v), then what
    // involves u (the packed rows l >= n_c, then b_u)
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

    double a1, a2, l_w, l_w_prev, l_h, l_h_prev, dsq, rt_norm2, cf;
    long long iters;
    if (a.first) {
        // deconvolution.py:192-204: a1 = a2 = 1, u_ = u, alpha_ = alpha, d = max(D)^2 over the solve's rows, l_w, l_h, cf
        const double* u0 = a.u0 + b * N * NU;
        const double* alpha0 = a.alpha0 + b * K * S;
        for (int e = t; e < K * S; e += kSmallThreads) {
            const int k = e / S, s = e - k * S;
            if constexpr (PURITY) m.a[k * SP + s] = alpha0[e];
            else m.a[k * SP + s] = m.ap[k * SP + s] = alpha0[e];
        }
        double u2 = 0.0, rt2 = 0.0, dmax = -INFINITY;
        for (int64_t i = t; i < N; i += kSmallThreads) {
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
        double w2 = 0.0;
        for (int e = t; e < NU * S; e += kSmallThreads) {
            const int j = e / S, s = e - j * S;
            w2 = fma(m.a[(n_c + j) * SP + s], m.a[(n_c + j) * SP + s], w2);
        }
        l_w = l_w_prev = block_sum(w2, m.red) * dsq;
        l_h = l_h_prev = (rt_norm2 + u2) * dsq;
        a1 = a2 = 1.0;
        iters = 0;
        gram_jobs<MASK>(p, m, 0, n_known);
        for (int e = t; e < n_known * S; e += kSmallThreads) {
            const int j = e / S, s = e - j * S;
            gk[e] = m.gb[(int)m.jd[j] * SP + s];
        }
        cf = stream_cost<MASK>(p, m);
    } else {
        for (int e = t; e < K * S; e += kSmallThreads) {
            const int k = e / S, s = e - k * S;
            m.a[k * SP + s] = ws_alpha[e];
            if constexpr (!PURITY) m.ap[k * SP + s] = ws_alpha_prev[e];
        }
        __syncthreads();  // (the job tables)
        for (int e = t; e < n_known * S; e += kSmallThreads) {
            const int j = e / S, s = e - j * S;
            m.gb[(int)m.jd[j] * SP + s] = gk[e];
        }
        a1 = scal[kSmA1], a2 = scal[kSmA2], l_w = scal[kSmLw], l_w_prev = scal[kSmLwPrev], l_h = scal[kSmLh];
        l_h_prev = scal[kSmLhPrev], dsq = scal[kSmDsq], rt_norm2 = scal[kSmRtNorm2], cf = scal[kSmCf];
        iters = a.iters[b];
        __syncthreads();
    }

    const int64_t T2 = a.n_iter2;
    int done = 0;
    for (int it = 0; it < a.n_run; ++it) {
        // the momentum ratios (a_{t-1} - 1) / a_t of both phases (:83-84, :95-96): they do not depend on the data
        if (t == 0 || (!PURITY && t == 64)) {
            double am = t == 0 ? a1 : a2;
            double* ratio = t == 0 ? ratio_u : ratio_h;
            for (int64_t q = 0; q < T2; ++q) {
                const double an = (1.0 + sqrt(1.0 + 4.0 * am * am)) / 2.0;
                ratio[q] = (am - 1.0) / an;
                am = an;
            }
            m.sh[t == 0 ? 0 : 1] = am;
        }
        __syncthreads();
        a1 = m.sh[0];
        if constexpr (!PURITY) a2 = m.sh[1];

        // ---- u phase (:81-90)
        const double cap_w = 0.9999 * sqrt(l_w_prev / l_w);
        double u2 = 0.0;
        for (int64_t i = t; i < N; i += kSmallThreads) {
            const int64_t g = p.row(i);
            double rt[kSmallMaxK - 1];
#pragma unroll
            for (int k = 0; k < kSmallMaxK - 1; ++k) rt[k] = k < n_c ? p.Rt[g * n_c + k] : 0.0;
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
                for (int k = 0; k < kSmallMaxK - 1; ++k)
                    if (k < n_c) x = fma(-rt[k], m.a[k * SP + s], x);
                x *= d;
                double au[NU];
#pragma unroll
                for (int j = 0; j < NU; ++j) au[j] = m.a[(n_c + j) * SP + s];
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
                    at[j] = a.mode == DMF_MODE_UNSUPERVISED ? uc[j] : ut[j];  // where the gradient is taken (:163)
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
        }
        if (T2 > 0) l_w_prev = l_w;
        u2 = block_sum(u2, m.red);  // (its barriers publish u to the workgroup)
        if constexpr (!PURITY) l_h = (rt_norm2 + u2) * dsq;  // :212

        // ---- the u-dependent entries of the per-sample Grams
        gram_jobs<MASK>(p, m, n_known, n_jobs);

        // ---- alpha phase: Frank-Wolfe under the purity constraint (:280-302), else (:93-102) thread s owns column s
        if constexpr (PURITY) {
            frank_wolfe_rows(m, a.purity, S, n_c, K, SP, n_pairs, T2);
        } else if (t < S) {
            const int s = t;
            const double cap_h = 0.9999 * sqrt(l_h_prev / l_h);
            for (int64_t q = 0; q < T2; ++q) {
                const double beta = fmin(ratio_h[q], q == 0 ? cap_h : 0.9999);
                for (int k = 0; k < K; ++k) {
                    const double ak = m.a[k * SP + s];
                    m.tmp[k * SP + s] = fma(beta, ak - m.ap[k * SP + s], ak);
                    m.ap[k * SP + s] = ak;
                }
                for (int k = 0; k < K; ++k) {
                    double gr = m.gb[(n_pairs + k) * SP + s];
                    for (int l = 0; l < K; ++l) {
                        const int q2 = k <= l ? l * (l + 1) / 2 + k : k * (k + 1) / 2 + l;
                        gr = fma(-m.gb[q2 * SP + s], m.tmp[l * SP + s], gr);
                    }
                    m.a[k * SP + s] = m.tmp[k * SP + s] + gr / l_h;
                }
                project_column_lds(m.a + s, m.srt + s, K, SP);
            }
        }
        if (T2 > 0) l_h_prev = l_h;
        __syncthreads();
        double w2 = 0.0;
        for (int e = t; e < NU * S; e += kSmallThreads) {
            const int j = e / S, s = e - j * S;
            w2 = fma(m.a[(n_c + j) * SP + s], m.a[(n_c + j) * SP + s], w2);
        }
        l_w = block_sum(w2, m.red) * dsq;  // :216

        // ---- cost and stop test (:218-220)
        const double cf_0 = cf;
        cf = stream_cost<MASK>(p, m);
        ++iters;
        if (fabs(cf - cf_0) < a.tol) {
            done = 1;
            break;
        }
    }

    // everything the next launch (or the host) reads
    for (int e = t; e < K * S; e += kSmallThreads) {
        const int k = e / S, s = e - k * S;
        ws_alpha[e] = m.a[k * SP + s];
        if constexpr (!PURITY) ws_alpha_prev[e] = m.ap[k * SP + s];
    }
    if (t == 0) {
        scal[kSmA1] = a1, scal[kSmA2] = a2, scal[kSmLw] = l_w, scal[kSmLwPrev] = l_w_prev, scal[kSmLh] = l_h;
        scal[kSmLhPrev] = l_h_prev, scal[kSmDsq] = dsq, scal[kSmRtNorm2] = rt_norm2, scal[kSmCf] = cf;
        a.iters[b] = iters;
        a.done[b] = done;
    }
}

// n_train[b] = the set bits among the N x S real positions of mask b: thread t counts rows t, t + 256, ..., the 256 integer
// partials are added by one fixed tree.  Bits of samples >= S in a row's last byte are padding and not counted.
__global__ __launch_bounds__(kSmallThreads) void k_small_mask_count(const uint8_t* __restrict__ mask, int64_t N, int S,
                                                                    long long* __restrict__ n_train) {
    __shared__ long long part[kSmallThreads];
    const int t = threadIdx.x, nb = (S + 7) / 8;
    const uint8_t* mb = mask + (int64_t)blockIdx.x * N * nb;
    const unsigned int last = (S & 7) ? (1u << (S & 7)) - 1u : 0xFFu;  // the real bits of a row's last byte
    long long n = 0;
    for (int64_t i = t; i < N; i += kSmallThreads)
        for (int q = 0; q < nb; ++q) n += __popc((unsigned int)mb[i * nb + q] & (q == nb - 1 ? last : 0xFFu));
    part[t] = n;
    __syncthreads();
    for (int off = kSmallThreads / 2; off > 0; off >>= 1) {
        if (t < off) part[t] += part[t + off];
        __syncthreads();
    }
    if (t == 0) n_train[blockIdx.x] = part[0];
}

// sum_sq[b] = sum over the held-out elements (bit 0) of (v - [Rt | u_b] alpha_b)^2 on the problem's full V: threads as
// (row slice r, sample s) like stream_cost, a thread adds its rows in rising order, the partials go through block_sum's tree.
__global__ __launch_bounds__(kSmallThreads) void k_small_holdout(const double* __restrict__ V, const double* __restrict__ Rt,
                                                                 const double* __restrict__ u, const double* __restrict__ alpha,
                                                                 const uint8_t* __restrict__ mask, int64_t N, int S, int n_c,
                                                                 int n_u, double* __restrict__ sum_sq) {
    __shared__ double al[kSmallMaxK * kSmallMaxS];
    __shared__ double red[kSmallThreads];
    const int64_t b = blockIdx.x;
    const int t = threadIdx.x, K = n_c + n_u, SP = pow2_at_least(S), nb = (S + 7) / 8, R = kSmallThreads / SP;
    for (int e = t; e < K * S; e += kSmallThreads) al[e] = alpha[b * K * S + e];
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
    if (mask == nullptr || n_train == nullptr || B < 1 || B > 0x7fffffff || N < 1 || S < 1 || S > kSmallMaxS)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_small_mask_count, dim3((unsigned)B), dim3(kSmallThreads), 0, st, mask, N, S, n_train);
    return hipGetLastError();
}

hipError_t launch_small_holdout(const double* V, const double* Rt, const double* u, const double* alpha, const uint8_t* mask,
                                int64_t B, int64_t N, int S, int n_c, int n_u, double* sum_sq, hipStream_t st) {
    if (V == nullptr || u == nullptr || alpha == nullptr || mask == nullptr || sum_sq == nullptr || B < 1 || B > 0x7fffffff ||
        !small_supported(N, S, n_c, n_u, DMF_MODE_PARTIAL) || (n_c > 0 && Rt == nullptr))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_small_holdout, dim3((unsigned)B), dim3(kSmallThreads), 0, st, V, Rt, u, alpha, mask, N, S, n_c, n_u,
                       sum_sq);
    return hipGetLastError();
}

bool small_supported(int64_t N, int64_t S, int64_t n_c, int64_t n_u, int mode) {
    if (mode != DMF_MODE_PARTIAL && mode != DMF_MODE_UNSUPERVISED) return false;
    if (N < 1 || S < 1 || S > kSmallMaxS || n_c < 0 || n_u < 1 || n_u > kSmallMaxNu || n_c + n_u > kSmallMaxK) return false;
    return N <= kSmallMaxElements / S;
}

size_t small_lds_bytes(int S, int K) {
    const int SP = pow2_at_least(S);
    const size_t doubles = (size_t)(K * (K + 1) / 2 + K) * SP + 4 * (size_t)K * SP + kSmallChunk * kSmallThreads + 8;
    return doubles * sizeof(double) + (kJobShorts * sizeof(short) + 7) / 8 * 8;
}

template <int NU, bool PURITY, bool MASK = false>
static hipError_t launch_nu(const SmallArgs& a, int64_t B, size_t lds, hipStream_t st) {
    static bool raised = false;  // more than 64 KB of dynamic LDS need the kernel's limit raised, once
    if (lds > 64 * 1024 && !raised) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_solve_small<NU, PURITY, MASK>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        raised = true;
    }
    hipLaunchKernelGGL((k_solve_small<NU, PURITY, MASK>), dim3((unsigned)B), dim3(kSmallThreads), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_solve_small(const SmallArgs& a, int64_t B, hipStream_t st) {
    if (!small_supported(a.N, a.S, a.n_c, a.n_u, a.mode) || B < 1 || B > 0x7fffffff) return hipErrorInvalidValue;
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
