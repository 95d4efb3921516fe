// The mid-size batch: B independent solves of one resident problem, W >= 1 workgroups per solve, three launches per outer
// iteration for all B solves.  The arithmetic is k_solve_small's and therefore the reference's
// (mdwbssmf_deconv, demethify/deconvolution.py:190-223; unsupervised_deconv, :107-184): the u phase is row-local on c_i, M_i in
// registers, the gradient is taken at u_temp in partial mode and at the previous iterate in unsupervised mode (:163), the
// momentum ratios and caps are the same, the alpha phase uses the sort-based projection (:21-37), l_h, l_w and
// d = max(D)^2 are taken over the solve's rows, the cost is the streaming one (:15-17) and the stop test is
// fabs(cf - cf_0) < tol on it (:220).  Only the orders of the sums over rows differ: a solve's rows are cut into W slabs
// of `rows` rows, slab w belongs to workgroup (b, w), and every sum over rows is a sum per slab followed by a sum of the
// slab partials in rising slab order.
//
// One outer iteration, for all B solves:
//   k_mid_rows   grid W x B.  Prologue: the W cost partials of the previous iteration are added in rising slab order and
//                compared with the cost before it (scal[kMdCf]).  Every workgroup of a solve reads the same numbers in the
//                same order, so all of them take the same decision.  Stop: slab 0 records `done`, nobody touches u.
//                Otherwise the u phase on the slab (a thread per row, alpha in LDS; :81-90), then the slab's partial of
//                ||u||^2 and of the u-dependent Gram jobs, threads as (row slice, sample).
//   k_mid_alpha  grid B.  Slab partials added in rising slab order into G_s, b_s in LDS (the known block from the copy made
//                at set-up), l_h (:212), the n_iter2 alpha steps (:93-102), l_w (:216), the momentum ratios of the NEXT
//                iteration, the scalars, the iteration count; scal[kMdCf] becomes the cost the prologue just used.
//   k_mid_cost   grid W x B.  The slab's partial of the streaming cost of the new iterate.
// Set-up (once per call): k_mid_setup_rows (grid W x B: u_ = u = u0, the slab's maximum count, ||R_trunc||^2, ||u||^2 and
// known Gram jobs), k_mid_setup_fin (grid B: :192-204), k_mid_cost.  k_mid_finish (a thread per solve) adds the cost
// partials and takes the stop decision once more, for the host.
//
// No workgroup waits for another: workgroups meet at launch boundaries only.  No atomics.  A workgroup (b, w) reads what
// solve b's workgroups wrote in EARLIER launches and writes only its own slab's rows and partials (k_mid_alpha: solve b's
// state), so a solve's result is a function of its own inputs and of (N, S, n_c, n_u, rows) alone -- not of B, its slot,
// what else is resident, or how often the host looks.  A solve that has stopped leaves every later launch at the prologue:
// its partials and scal[kMdCf] no longer change, so the decision is the same each time.
//
// The purity-constrained solve (dmf_solve_mid_purity; mdwbssmf_deconv_p, :306-337) runs the same launches with
// k_mid_alpha_fw in k_mid_alpha's place: the same G_s, b_s from the same slab partials, then n_iter2 Frank-Wolfe steps per
// sample (frank_wolfe_nmf, :280-302) with every sample on a 16-lane row of its own, all samples stepping at once in one
// workgroup of 64 ceil(S / 4) threads.  There is no a2, no l_h and no alpha_; the purity vector is an input shared by the B
// solves.  Every other kernel is launched as it is.
#include "dmf_mid.h"
#include "dmf_rowlanes.h"

#include "../../include/demethify_hip.h"

namespace dmf {

namespace {

constexpr int kMaxJobs = kMidMaxK * (kMidMaxK + 1) / 2 + kMidMaxK;  // 152
constexpr int kRowsInFlight = 4;  // rows a thread of the (slice, sample) passes loads before it uses any

__host__ __device__ inline int pow2_at_least(int s) {
    int p = 1;
    while (p < s) p <<= 1;
    return p;
}

__device__ __forceinline__ double block_sum(double x, double* red) {
    const int t = threadIdx.x;
    red[t] = x;
    __syncthreads();
#pragma unroll
    for (int off = kMidThreads / 2; off > 0; off >>= 1) {
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
    for (int off = kMidThreads / 2; off > 0; off >>= 1) {
        if (t < off) red[t] = fmax(red[t], red[t + off]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// Rows [lo, hi) of one solve: what a slab's workgroup reads.
struct Slab {
    const double* V;
    const double* D;
    const double* Rt;
    const long long* idx;  // this solve's row list, or null: the identity
    const double* u;       // this solve's current u
    int64_t lo, hi;
    int S, n_c, n_u, K, SP, R;
    __device__ __forceinline__ int64_t row(int64_t i) const { return idx != nullptr ? (int64_t)idx[i] : i; }
};

__device__ __forceinline__ Slab make_slab(const MidArgs& a, int64_t b, int w, const double* u) {
    Slab p;
    p.V = a.V, p.D = a.D, p.Rt = a.Rt;
    p.idx = a.idx != nullptr ? a.idx + b * a.N : nullptr;
    p.u = u;
    p.lo = (int64_t)w * a.rows;
    p.hi = p.lo + a.rows < a.N ? p.lo + a.rows : a.N;
    p.S = a.S, p.n_c = a.n_c, p.n_u = a.n_u, p.K = a.n_c + a.n_u;
    p.SP = pow2_at_least(a.S);
    p.R = kMidThreads / p.SP;
    return p;
}

// The job tables of k_solve_small: x_k, x_l over (R_trunc columns, u columns, v = column K) and the packed row of G / b the
// product goes to.  known: the pairs of R_trunc columns, then their products with v; else what involves u (the packed rows
// l >= n_c, then b_u).  Returns the number of jobs.
__device__ int fill_jobs(short* jk, short* jl, short* jd, int n_c, int K, bool known) {
    const int n_pairs = K * (K + 1) / 2;
    int j = 0;
    const int l0 = known ? 0 : n_c, l1 = known ? n_c : K;
    for (int l = l0; l < l1; ++l)
        for (int k = 0; k <= l; ++k) jk[j] = (short)k, jl[j] = (short)l, jd[j] = (short)(l * (l + 1) / 2 + k), ++j;
    for (int k = l0; k < l1; ++k) jk[j] = (short)k, jl[j] = (short)K, jd[j] = (short)(n_pairs + k), ++j;
    return j;
}

// out[j][s] = sum over the slab's rows of d_is x_k x_l for the n_jobs jobs of (jk, jl); out has S doubles per job.  Threads as
// (slice r, sample s); slice r adds rows lo + r, lo + r + R, ... in rising order, the slices are added in rising order.
__device__ void gram_slab(const Slab& p, const short* jk, const short* jl, int n_jobs, double* red, double* __restrict__ out) {
    const int t = threadIdx.x;
    const int s = t & (p.SP - 1), r = t / p.SP;
    const bool active = s < p.S;
    for (int base = 0; base < n_jobs; base += kMidChunk) {
        const int nj = min(kMidChunk, n_jobs - base);
        double acc[kMidChunk];
#pragma unroll
        for (int j = 0; j < kMidChunk; ++j) acc[j] = 0.0;
        if (active) {
            // kRowsInFlight rows per trip, so that their loads are in flight together; a row past the end reads row i again
            // with weight 0: acc + 0, the sums and their order are the same
            for (int64_t i = p.lo + r; i < p.hi; i += (int64_t)kRowsInFlight * p.R) {
                double d[kRowsInFlight], v[kRowsInFlight];
                const double* rt[kRowsInFlight];
                const double* ui[kRowsInFlight];
#pragma unroll
                for (int q = 0; q < kRowsInFlight; ++q) {
                    const int64_t iq = i + (int64_t)q * p.R;
                    const bool in = iq < p.hi;
                    const int64_t ic = in ? iq : i, g = p.row(ic);
                    d[q] = in ? p.D[g * p.S + s] : 0.0;
                    v[q] = p.V[g * p.S + s];
                    rt[q] = p.Rt + g * p.n_c;
                    ui[q] = p.u + ic * p.n_u;
                }
#pragma unroll
                for (int j = 0; j < kMidChunk; ++j) {
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
        for (int j = 0; j < kMidChunk; ++j) red[(j * p.R + r) * p.SP + s] = acc[j];
        __syncthreads();
        for (int o = t; o < nj * p.SP; o += kMidThreads) {
            const int j = o / p.SP, so = o & (p.SP - 1);
            if (so < p.S) {
                double sum = 0.0;
                for (int rr = 0; rr < p.R; ++rr) sum += red[(j * p.R + rr) * p.SP + so];
                out[(int64_t)(base + j) * p.S + so] = sum;
            }
        }
        __syncthreads();
    }
}

// sum_i sum_s d (v - [Rt | u] alpha)^2 over the slab's rows with alpha (K x SP) from LDS (deconvolution.py:15-17)
__device__ double stream_cost_slab(const Slab& p, const double* al, double* red) {
    const int t = threadIdx.x;
    const int s = t & (p.SP - 1), r = t / p.SP;
    double acc = 0.0;
    if (s < p.S) {
        for (int64_t i = p.lo + r; i < p.hi; i += (int64_t)kRowsInFlight * p.R) {
            double d[kRowsInFlight], resid[kRowsInFlight];
            const double* rt[kRowsInFlight];
            const double* ui[kRowsInFlight];
#pragma unroll
            for (int q = 0; q < kRowsInFlight; ++q) {
                const int64_t iq = i + (int64_t)q * p.R;
                const bool in = iq < p.hi;
                const int64_t ic = in ? iq : i, g = p.row(ic);
                d[q] = in ? p.D[g * p.S + s] : 0.0;
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

// the momentum ratios (a_{t-1} - 1) / a_t of one phase's next n steps (:83-84, :95-96); returns a_n
__device__ double fill_ratios(double am, double* ratio, int64_t n) {
    for (int64_t q = 0; q < n; ++q) {
        const double an = (1.0 + sqrt(1.0 + 4.0 * am * am)) / 2.0;
        ratio[q] = (am - 1.0) / an;
        am = an;
    }
    return am;
}

// the W cost partials of solve b in rising slab order: the cost of its current iterate
__device__ __forceinline__ double cost_of_partials(const MidArgs& a, int64_t b) {
    const double* pc = a.part_cf + b * a.W;
    double cf = 0.0;
    for (int w = 0; w < a.W; ++w) cf += pc[w];
    return cf;
}

// alpha of solve b (K x S in memory) to LDS (K x SP)
__device__ __forceinline__ void load_alpha(const double* ws_alpha, double* al, int K, int S, int SP) {
    for (int e = threadIdx.x; e < K * S; e += kMidThreads) {
        const int k = e / S, s = e - k * S;
        al[k * SP + s] = ws_alpha[e];
    }
}

// ---- the Frank-Wolfe device helpers of k_solve_small's purity variant (dmf_kernels_small.hip), copied like the row helpers
// above; the lane moves and the argmin butterfly are dmf_rowlanes.h's
// g4[l % 4] += G[l] a[lane l of the row] for l = L .. 15, in this order (row_newbcast:l; four chains)
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

}  // namespace

// ---- set-up, part 1 (grid W x B): the slab's rows of u and u_, its partials of max(D), ||R_trunc||^2, ||u0||^2 and of the
// known Gram jobs
__global__ __launch_bounds__(kMidThreads) void k_mid_setup_rows(MidArgs a) {
    __shared__ double red[kMidChunk * kMidThreads];
    __shared__ short jk[kMaxJobs], jl[kMaxJobs], jd[kMaxJobs];
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x / a.W;
    const int w = (int)(blockIdx.x - b * a.W);
    const int64_t N = a.N;
    const int n_u = a.n_u, n_c = a.n_c, S = a.S;
    double* u = a.u + b * N * n_u;
    double* u_prev = a.u_prev + b * N * n_u;
    const double* u0 = a.u0 + b * N * n_u;
    const Slab p = make_slab(a, b, w, u);
    if (t == 0) fill_jobs(jk, jl, jd, n_c, p.K, true);
    double u2 = 0.0, rt2 = 0.0, dmax = -INFINITY;
    for (int64_t i = p.lo + t; i < p.hi; i += kMidThreads) {
        for (int j = 0; j < n_u; ++j) {
            const double x = u0[i * n_u + j];
            u[i * n_u + j] = u_prev[i * n_u + j] = x;
            u2 = fma(x, x, u2);
        }
        const int64_t g = p.row(i);
        for (int k = 0; k < n_c; ++k) rt2 = fma(p.Rt[g * n_c + k], p.Rt[g * n_c + k], rt2);
    }
    {
        const int s = t & (p.SP - 1), r = t / p.SP;
        if (s < S)
            for (int64_t i = p.lo + r; i < p.hi; i += p.R) dmax = fmax(dmax, p.D[p.row(i) * S + s]);
    }
    dmax = block_max(dmax, red);
    rt2 = block_sum(rt2, red);
    u2 = block_sum(u2, red);  // (its barriers also publish the job tables)
    double* ps = a.part_s + (b * a.W + w) * kMidSlabScalars;
    if (t == 0) ps[0] = u2, ps[1] = rt2, ps[2] = dmax, ps[3] = 0.0;
    gram_slab(p, jk, jl, mid_known_jobs(n_c), red, a.part_g + (b * a.W + w) * (int64_t)a.n_pj * S);
}

// ---- set-up, part 2 (grid B; deconvolution.py:192-204): a1 = a2 = 1, alpha_ = alpha = alpha0, d = max(D)^2, l_w, l_h, the
// known Gram block, the momentum ratios of the first iteration.  scal[kMdCf] = +inf: the first prologue compares the first
// cost with it and does not stop.
__global__ __launch_bounds__(kMidThreads) void k_mid_setup_fin(MidArgs a) {
    __shared__ double red[kMidThreads];
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int S = a.S, n_c = a.n_c, n_u = a.n_u, K = n_c + n_u, W = a.W;
    const double* ps = a.part_s + b * W * kMidSlabScalars;
    double u2 = 0.0, rt2 = 0.0, dmax = -INFINITY;
    for (int w = 0; w < W; ++w) {
        u2 += ps[w * kMidSlabScalars + 0];
        rt2 += ps[w * kMidSlabScalars + 1];
        dmax = fmax(dmax, ps[w * kMidSlabScalars + 2]);
    }
    const double dsq = dmax * dmax;
    const int n_known = mid_known_jobs(n_c);
    double* gk = a.gk + b * (int64_t)n_known * S;
    const double* pg = a.part_g + b * W * (int64_t)a.n_pj * S;
    for (int e = t; e < n_known * S; e += kMidThreads) {
        double sum = 0.0;
        for (int w = 0; w < W; ++w) sum += pg[(int64_t)w * a.n_pj * S + e];
        gk[e] = sum;
    }
    const double* alpha0 = a.alpha0 + b * K * S;
    double* ws_alpha = a.alpha + b * K * S;
    double* ws_alpha_prev = a.alpha_prev + b * K * S;
    for (int e = t; e < K * S; e += kMidThreads) ws_alpha[e] = ws_alpha_prev[e] = alpha0[e];
    double w2 = 0.0;
    for (int e = t; e < n_u * S; e += kMidThreads) w2 = fma(alpha0[n_c * S + e], alpha0[n_c * S + e], w2);
    const double l_w = block_sum(w2, red) * dsq;
    double* scal = a.scal + b * kMidScalars;
    double* ratio_u = a.ratio + b * 2 * a.n_iter2;
    if (t == 0) {
        scal[kMdA1] = fill_ratios(1.0, ratio_u, a.n_iter2);
        scal[kMdLw] = scal[kMdLwPrev] = l_w;
        scal[kMdLh] = scal[kMdLhPrev] = (rt2 + u2) * dsq;
        scal[kMdDsq] = dsq, scal[kMdRtNorm2] = rt2, scal[kMdCf] = INFINITY;
        a.iters[b] = 0;
        a.done[b] = 0;
    }
    if (t == 64) scal[kMdA2] = fill_ratios(1.0, ratio_u + a.n_iter2, a.n_iter2);
}

// ---- the row launch of an outer iteration (grid W x B)
template <int NU>
__global__ __launch_bounds__(kMidThreads) void k_mid_rows(MidArgs a) {
    constexpr int NP = NU * (NU + 1) / 2;
    __shared__ double al[kMidMaxK * kMidMaxS];
    __shared__ double red[kMidChunk * kMidThreads];
    __shared__ short jk[kMaxJobs], jl[kMaxJobs], jd[kMaxJobs];
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x / a.W;
    const int w = (int)(blockIdx.x - b * a.W);
    const double* scal = a.scal + b * kMidScalars;
    // the stop test of the previous iteration (:218-220), taken by every workgroup of the solve on the same numbers
    if (fabs(cost_of_partials(a, b) - scal[kMdCf]) < a.tol) {
        if (w == 0 && t == 0) a.done[b] = 1;
        return;
    }
    const int64_t N = a.N;
    const int S = a.S, n_c = a.n_c, K = n_c + NU;
    double* u = a.u + b * N * NU;
    double* u_prev = a.u_prev + b * N * NU;
    const Slab p = make_slab(a, b, w, u);
    const int SP = p.SP;
    load_alpha(a.alpha + b * K * S, al, K, S, SP);
    if (t == 0) fill_jobs(jk, jl, jd, n_c, K, false);
    const double l_w = scal[kMdLw], l_w_prev = scal[kMdLwPrev];
    const double* ratio_u = a.ratio + b * 2 * a.n_iter2;
    const int64_t T2 = a.n_iter2;
    __syncthreads();

    // ---- u phase (:81-90), a thread per row
    const double cap_w = 0.9999 * sqrt(l_w_prev / l_w);
    double u2 = 0.0;
    for (int64_t i = p.lo + t; i < p.hi; i += kMidThreads) {
        const int64_t g = p.row(i);
        double rt[kMidMaxK - 1];
#pragma unroll
        for (int k = 0; k < kMidMaxK - 1; ++k) rt[k] = k < n_c ? p.Rt[g * n_c + k] : 0.0;
        double c[NU], M[NP];
#pragma unroll
        for (int j = 0; j < NU; ++j) c[j] = 0.0;
#pragma unroll
        for (int q = 0; q < NP; ++q) M[q] = 0.0;
        const double* Vr = p.V + g * S;
        const double* Dr = p.D + g * S;
#pragma unroll 4
        for (int s = 0; s < S; ++s) {
            const double d = Dr[s];
            double x = Vr[s];
#pragma unroll
            for (int k = 0; k < kMidMaxK - 1; ++k)
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
    u2 = block_sum(u2, red);  // (its barriers publish the slab's u to the workgroup)
    if (t == 0) a.part_s[(b * a.W + w) * kMidSlabScalars] = u2;

    // ---- the slab's partial of the u-dependent entries of the per-sample Grams
    gram_slab(p, jk, jl, mid_u_jobs(n_c, NU), red, a.part_g + (b * a.W + w) * (int64_t)a.n_pj * S);
}

// ---- the alpha launch of an outer iteration (grid B)
__global__ __launch_bounds__(kMidThreads) void k_mid_alpha(MidArgs a) {
    const int64_t b = blockIdx.x;
    if (a.done[b]) return;  // (recorded by slab 0 of this iteration's row launch, or by k_mid_finish)
    extern __shared__ double mid_lds[];
    const int t = threadIdx.x;
    const int S = a.S, n_c = a.n_c, n_u = a.n_u, K = n_c + n_u, SP = pow2_at_least(S), W = a.W;
    const int n_pairs = K * (K + 1) / 2;
    double* gb = mid_lds;                    // [K (K + 1) / 2 + K][SP]: packed G, then b
    double* al = gb + (n_pairs + K) * SP;    // [K][SP] alpha
    double* ap = al + K * SP;                // [K][SP] alpha_
    double* tmp = ap + K * SP;               // [K][SP] alpha_temp
    double* srt = tmp + K * SP;              // [K][SP] sort scratch
    double* red = srt + K * SP;              // [256]
    short* jk = reinterpret_cast<short*>(red + kMidThreads);
    short* jl = jk + kMaxJobs;
    short* jdk = jl + kMaxJobs;   // rows of gb of the known jobs
    short* jdu = jdk + kMaxJobs;  // ... and of the u jobs
    double* ws_alpha = a.alpha + b * K * S;
    double* ws_alpha_prev = a.alpha_prev + b * K * S;
    double* scal = a.scal + b * kMidScalars;
    double* ratio_u = a.ratio + b * 2 * a.n_iter2;
    double* ratio_h = ratio_u + a.n_iter2;
    const int n_known = mid_known_jobs(n_c), n_uj = mid_u_jobs(n_c, n_u);
    if (t == 0) {
        fill_jobs(jk, jl, jdk, n_c, K, true);
        fill_jobs(jk, jl, jdu, n_c, K, false);
    }
    load_alpha(ws_alpha, al, K, S, SP);
    load_alpha(ws_alpha_prev, ap, K, S, SP);
    const double cf = cost_of_partials(a, b);  // the cost of the iterate this iteration started from
    double u2 = 0.0;
    for (int w = 0; w < W; ++w) u2 += a.part_s[(b * W + w) * kMidSlabScalars];
    const double l_w_old = scal[kMdLw], l_h_prev = scal[kMdLhPrev], dsq = scal[kMdDsq], rt_norm2 = scal[kMdRtNorm2];
    const double a1 = scal[kMdA1], a2 = scal[kMdA2];
    const int64_t T2 = a.n_iter2;
    __syncthreads();
    const double* gk = a.gk + b * (int64_t)n_known * S;
    for (int e = t; e < n_known * S; e += kMidThreads) {
        const int j = e / S, s = e - j * S;
        gb[(int)jdk[j] * SP + s] = gk[e];
    }
    const double* pg = a.part_g + b * W * (int64_t)a.n_pj * S;
    for (int e = t; e < n_uj * S; e += kMidThreads) {
        const int j = e / S, s = e - j * S;
        double sum = 0.0;
        for (int w = 0; w < W; ++w) sum += pg[(int64_t)w * a.n_pj * S + e];
        gb[(int)jdu[j] * SP + s] = sum;
    }
    const double l_h = (rt_norm2 + u2) * dsq;  // :212
    __syncthreads();

    // ---- alpha phase (:93-102): thread s owns column s
    if (t < S) {
        const int s = t;
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
    __syncthreads();
    double w2 = 0.0;
    for (int e = t; e < n_u * S; e += kMidThreads) {
        const int j = e / S, s = e - j * S;
        w2 = fma(al[(n_c + j) * SP + s], al[(n_c + j) * SP + s], w2);
    }
    const double l_w = block_sum(w2, red) * dsq;  // :216

    // everything the next launches (or the host) read
    for (int e = t; e < K * S; e += kMidThreads) {
        const int k = e / S, s = e - k * S;
        ws_alpha[e] = al[k * SP + s];
        ws_alpha_prev[e] = ap[k * SP + s];
    }
    if (t == 0) {
        scal[kMdA1] = fill_ratios(a1, ratio_u, T2);
        scal[kMdLw] = l_w;
        if (T2 > 0) scal[kMdLwPrev] = l_w_old, scal[kMdLhPrev] = l_h;
        scal[kMdLh] = l_h;
        scal[kMdCf] = cf;
        a.iters[b] += 1;
    }
    if (t == 64) scal[kMdA2] = fill_ratios(a2, ratio_h, T2);  // (after the barriers behind the alpha phase, which read it)
}

// ---- the alpha launch of a purity-constrained outer iteration (grid B, 64 ceil(S / 4) threads): k_mid_alpha's Grams, then
// the Frank-Wolfe steps of deconvolution.py:280-302 as k_solve_small's purity variant takes them -- sample s on the 16-lane
// row s of the workgroup, lane k holding row k of G_s in registers, grad = G a - b, the argmin of each block with the lowest
// index first among equal minima (np.argmin), step 2 / (k + 2), vertex mass purity[s] on the known block and 1 - purity[s]
// on the unknown one.  All samples step at once; n_iter2 is the only bound of the loop the DPP moves sit in, so every wave
// finds its four rows complete (rows past S run on sample S - 1's numbers and write nothing).
__global__ __launch_bounds__(kMidFwMaxThreads) void k_mid_alpha_fw(MidArgs a, const double* __restrict__ purity) {
    const int64_t b = blockIdx.x;
    if (a.done[b]) return;  // (recorded by slab 0 of this iteration's row launch, or by k_mid_finish)
    extern __shared__ double mid_lds[];
    const int t = threadIdx.x, nt = blockDim.x;
    const int S = a.S, n_c = a.n_c, n_u = a.n_u, K = n_c + n_u, SP = pow2_at_least(S), W = a.W;
    const int n_pairs = K * (K + 1) / 2;
    double* gb = mid_lds;                  // [K (K + 1) / 2 + K][SP]: packed G, then b
    double* al = gb + (n_pairs + K) * SP;  // [K][SP] alpha
    double* red = al + K * SP;             // [kMidThreads]: the squares of the unknown block, then their tree
    short* jk = reinterpret_cast<short*>(red + kMidThreads);
    short* jl = jk + kMaxJobs;
    short* jdk = jl + kMaxJobs;   // rows of gb of the known jobs
    short* jdu = jdk + kMaxJobs;  // ... and of the u jobs
    double* ws_alpha = a.alpha + b * K * S;
    double* scal = a.scal + b * kMidScalars;
    const int n_known = mid_known_jobs(n_c), n_uj = mid_u_jobs(n_c, n_u);
    if (t == 0) {
        fill_jobs(jk, jl, jdk, n_c, K, true);
        fill_jobs(jk, jl, jdu, n_c, K, false);
    }
    for (int e = t; e < K * S; e += nt) {
        const int k = e / S, s = e - k * S;
        al[k * SP + s] = ws_alpha[e];
    }
    const double cf = cost_of_partials(a, b);  // the cost of the iterate this iteration started from
    const double l_w_old = scal[kMdLw], dsq = scal[kMdDsq], a1 = scal[kMdA1];
    const int64_t T2 = a.n_iter2;
    __syncthreads();
    const double* gk = a.gk + b * (int64_t)n_known * S;
    for (int e = t; e < n_known * S; e += nt) {
        const int j = e / S, s = e - j * S;
        gb[(int)jdk[j] * SP + s] = gk[e];
    }
    const double* pg = a.part_g + b * W * (int64_t)a.n_pj * S;
    for (int e = t; e < n_uj * S; e += nt) {
        const int j = e / S, s = e - j * S;
        double sum = 0.0;
        for (int w = 0; w < W; ++w) sum += pg[(int64_t)w * a.n_pj * S + e];
        gb[(int)jdu[j] * SP + s] = sum;
    }
    __syncthreads();

    // ---- Frank-Wolfe: lane k of row s
    {
        const int k = t & 15, s = t >> 4;
        const bool row_ok = k < K, known = k < n_c, unknown = row_ok && !known;
        const bool col_ok = s < S;
        const int kc = row_ok ? k : K - 1, sc = col_ok ? s : S - 1;
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
        double x = row_ok ? al[kc * SP + sc] : 0.0;
        __syncthreads();  // (every lane has read its alpha before any is replaced)
        for (int64_t it = 0; it < T2; ++it) {
            double g4[4] = {-bk, 0.0, 0.0, 0.0};
            gram_row_times_a(g4, x, Grow);
            const double grad = (g4[0] + g4[1]) + (g4[2] + g4[3]);
            double v1 = known ? grad : INFINITY, v2 = unknown ? grad : INFINITY;
            int i1 = k, i2 = k;
            argmin_step<1>(v1, i1, k); argmin_step<2>(v1, i1, k); argmin_step<4>(v1, i1, k); argmin_step<8>(v1, i1, k);
            argmin_step<1>(v2, i2, k); argmin_step<2>(v2, i2, k); argmin_step<4>(v2, i2, k); argmin_step<8>(v2, i2, k);
            const double gamma = 2.0 / (double)(it + 2);
            const bool at_vertex = (known && k == i1) || (unknown && k == i2);
            x = frank_wolfe_update(x, gamma, at_vertex ? mass : 0.0);
        }
        if (col_ok && row_ok) al[k * SP + s] = x;
    }
    __syncthreads();

    // ---- l_w = ||alpha[n_c:]||^2 d (:327): the n_u S <= 256 squares, zero-padded to 256, through one fixed tree
    for (int e = t; e < kMidThreads; e += nt) {
        const int j = e / S, s = e - j * S;
        const double x = e < n_u * S ? al[(n_c + j) * SP + s] : 0.0;
        red[e] = x * x;
    }
    __syncthreads();
    for (int off = kMidThreads / 2; off > 0; off >>= 1) {
        for (int e = t; e < off; e += nt) red[e] += red[e + off];
        __syncthreads();
    }
    const double l_w = red[0] * dsq;

    // everything the next launches (or the host) read
    for (int e = t; e < K * S; e += nt) {
        const int k = e / S, s = e - k * S;
        ws_alpha[e] = al[k * SP + s];
    }
    if (t == 0) {
        scal[kMdA1] = fill_ratios(a1, a.ratio + b * 2 * a.n_iter2, T2);
        scal[kMdLw] = l_w;
        if (T2 > 0) scal[kMdLwPrev] = l_w_old;
        scal[kMdCf] = cf;
        a.iters[b] += 1;
    }
}

// ---- the cost launch (grid W x B): the slab's partial of the streaming cost of the current iterate
__global__ __launch_bounds__(kMidThreads) void k_mid_cost(MidArgs a) {
    __shared__ double al[kMidMaxK * kMidMaxS];
    __shared__ double red[kMidThreads];
    const int64_t b = blockIdx.x / a.W;
    const int w = (int)(blockIdx.x - b * a.W);
    if (a.done[b]) return;
    const int K = a.n_c + a.n_u;
    const Slab p = make_slab(a, b, w, a.u + b * a.N * a.n_u);
    load_alpha(a.alpha + b * K * a.S, al, K, a.S, p.SP);
    __syncthreads();
    const double cf = stream_cost_slab(p, al, red);
    if (threadIdx.x == 0) a.part_cf[b * a.W + w] = cf;
}

// ---- cost[b] = the cost of solve b's current iterate, done[b] = its stop test (a thread per solve)
__global__ __launch_bounds__(kMidThreads) void k_mid_finish(MidArgs a, int64_t B) {
    const int64_t b = (int64_t)blockIdx.x * kMidThreads + threadIdx.x;
    if (b >= B) return;
    const double cf = cost_of_partials(a, b);
    a.cost[b] = cf;
    if (fabs(cf - a.scal[b * kMidScalars + kMdCf]) < a.tol) a.done[b] = 1;
}

bool mid_supported(int64_t N, int64_t S, int64_t n_c, int64_t n_u, int mode) {
    if (mode != DMF_MODE_PARTIAL && mode != DMF_MODE_UNSUPERVISED) return false;
    if (N < 1 || S < 1 || S > kMidMaxS || n_c < 0 || n_u < 1 || n_u > kMidMaxNu || n_c + n_u > kMidMaxK) return false;
    return N <= kMidMaxElements / S;
}

bool mid_plan(int64_t N, int64_t S, int64_t rows_per_workgroup, MidPlan* out) {
    if (N < 1 || S < 1 || rows_per_workgroup < 0 || out == nullptr) return false;
    int64_t rows = rows_per_workgroup;
    if (rows == 0) rows = kMidThreads * ((N + (int64_t)kMidThreads * kMidMaxW - 1) / ((int64_t)kMidThreads * kMidMaxW));
    if (rows % kMidThreads != 0) return false;
    const int64_t W = (N + rows - 1) / rows;
    if (W > kMidMaxW) return false;
    int64_t every = S <= ((int64_t)1 << 22) / N ? ((int64_t)1 << 22) / (N * S) : 0;
    every = every < 4 ? 4 : (every > 16 ? 16 : every);
    out->rows = rows, out->W = (int)W, out->check_every = (int)every;
    return true;
}

size_t mid_alpha_lds_bytes(int S, int K) {
    const int SP = pow2_at_least(S);
    const size_t doubles = (size_t)(K * (K + 1) / 2 + K) * SP + 4 * (size_t)K * SP + kMidThreads;
    return doubles * sizeof(double) + (4 * kMaxJobs * sizeof(short) + 7) / 8 * 8;
}

size_t mid_alpha_fw_lds_bytes(int S, int K) {
    const int SP = pow2_at_least(S);
    const size_t doubles = (size_t)(K * (K + 1) / 2 + K) * SP + (size_t)K * SP + kMidThreads;
    return doubles * sizeof(double) + (4 * kMaxJobs * sizeof(short) + 7) / 8 * 8;
}

static bool mid_args_ok(const MidArgs& a, int64_t B) {
    if (!mid_supported(a.N, a.S, a.n_c, a.n_u, a.mode) || B < 1) return false;
    if (a.rows < kMidThreads || a.rows % kMidThreads != 0 || a.W < 1 || a.W > kMidMaxW) return false;
    if ((int64_t)(a.W - 1) * a.rows >= a.N || (int64_t)a.W * a.rows < a.N) return false;  // the slabs cover the rows exactly
    if (a.n_pj != mid_slab_jobs(a.n_c, a.n_u) || a.n_iter2 < 0) return false;
    return B <= 0x7fffffff / a.W;
}

hipError_t launch_mid_setup(const MidArgs& a, int64_t B, hipStream_t st) {
    if (!mid_args_ok(a, B)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mid_setup_rows, dim3((unsigned)(B * a.W)), dim3(kMidThreads), 0, st, a);
    hipLaunchKernelGGL(k_mid_setup_fin, dim3((unsigned)B), dim3(kMidThreads), 0, st, a);
    hipLaunchKernelGGL(k_mid_cost, dim3((unsigned)(B * a.W)), dim3(kMidThreads), 0, st, a);
    return hipGetLastError();
}

template <int NU>
static void launch_rows(const MidArgs& a, int64_t B, hipStream_t st) {
    hipLaunchKernelGGL((k_mid_rows<NU>), dim3((unsigned)(B * a.W)), dim3(kMidThreads), 0, st, a);
}

static hipError_t raise_lds_limit(const void* kernel, size_t lds, bool* raised) {
    if (lds > 64 * 1024 && !*raised) {  // more than 64 KB of dynamic LDS need the kernel's limit raised, once
        const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        *raised = true;
    }
    return hipSuccess;
}

hipError_t launch_mid_iteration(const MidArgs& a, int64_t B, hipStream_t st, const double* purity) {
    if (!mid_args_ok(a, B)) return hipErrorInvalidValue;
    // the purity variant: partial mode with a known block to hold at that mass
    if (purity != nullptr && (a.mode != DMF_MODE_PARTIAL || a.n_c < 1)) return hipErrorInvalidValue;
    const int K = a.n_c + a.n_u;
    const size_t lds = purity != nullptr ? mid_alpha_fw_lds_bytes(a.S, K) : mid_alpha_lds_bytes(a.S, K);
    static bool raised = false, raised_fw = false;
    const hipError_t e = purity != nullptr ? raise_lds_limit(reinterpret_cast<const void*>(&k_mid_alpha_fw), lds, &raised_fw)
                                           : raise_lds_limit(reinterpret_cast<const void*>(&k_mid_alpha), lds, &raised);
    if (e != hipSuccess) return e;
    switch (a.n_u) {
        case 1: launch_rows<1>(a, B, st); break;
        case 2: launch_rows<2>(a, B, st); break;
        case 3: launch_rows<3>(a, B, st); break;
        default: launch_rows<4>(a, B, st); break;
    }
    if (purity != nullptr)  // a 16-lane row per sample, four rows to a wave
        hipLaunchKernelGGL(k_mid_alpha_fw, dim3((unsigned)B), dim3((unsigned)(64 * ((a.S + 3) / 4))), lds, st, a, purity);
    else
        hipLaunchKernelGGL(k_mid_alpha, dim3((unsigned)B), dim3(kMidThreads), lds, st, a);
    hipLaunchKernelGGL(k_mid_cost, dim3((unsigned)(B * a.W)), dim3(kMidThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_mid_finish(const MidArgs& a, int64_t B, hipStream_t st) {
    if (!mid_args_ok(a, B) || a.cost == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mid_finish, dim3((unsigned)((B + kMidThreads - 1) / kMidThreads)), dim3(kMidThreads), 0, st, a, B);
    return hipGetLastError();
}

}  // namespace dmf
