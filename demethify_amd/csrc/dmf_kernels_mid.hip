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
//                compared with the cost before it (scal[kBsCf]).  Every workgroup of a solve reads the same numbers in the
//                same order, so all of them take the same decision.  Stop: slab 0 records `done`, nobody touches u.
//                Otherwise the u phase on the slab (a thread per row, alpha in LDS; :81-90), then the slab's partial of
//                ||u||^2 and of the u-dependent Gram jobs, threads as (row slice, sample).
//   k_mid_alpha  grid B.  Slab partials added in rising slab order into G_s, b_s in LDS (the known block from the copy made
//                at set-up), l_h (:212), the n_iter2 alpha steps (:93-102), l_w (:216), the momentum ratios of the NEXT
//                iteration, the scalars, the iteration count; scal[kBsCf] becomes the cost the prologue just used.
//   k_mid_cost   grid W x B.  The slab's partial of the streaming cost of the new iterate.
// Set-up (once per call): k_mid_setup_rows (grid W x B: u_ = u = u0, the slab's maximum count, ||R_trunc||^2, ||u||^2 and
// known Gram jobs), k_mid_setup_fin (grid B: :192-204), k_mid_cost.  k_mid_finish (a thread per solve) adds the cost
// partials and takes the stop decision once more, for the host.
//
// No workgroup waits for another: workgroups meet at launch boundaries only.  No atomics.  A workgroup (b, w) reads what
// solve b's workgroups wrote in EARLIER launches and writes only its own slab's rows and partials (k_mid_alpha: solve b's
// state), so a solve's result is a function of its own inputs and of (N, S, n_c, n_u, rows) alone -- not of B, its slot,
// what else is resident, or how often the host looks.  A solve that has stopped leaves every later launch at the prologue:
// its partials and scal[kBsCf] no longer change, so the decision is the same each time.
//
// The purity-constrained solve (dmf_solve_mid_purity; mdwbssmf_deconv_p, :306-337) runs the same launches with
// k_mid_alpha_fw in k_mid_alpha's place: the same G_s, b_s from the same slab partials, then n_iter2 Frank-Wolfe steps per
// sample (frank_wolfe_nmf, :280-302) with every sample on a 16-lane row of its own, all samples stepping at once in one
// workgroup of 64 ceil(S / 4) threads.  There is no a2, no l_h and no alpha_; the purity vector is an input shared by the B
// solves.  Every other kernel is launched as it is.
//
// The masked solve (dmf_solve_mid_masked; a bi-cross-validation fold, ic.py:58-89) gives solve b a train mask of its own
// (MidArgs::mask, dmf_problem_mask's packing) and runs the MASK instances of k_mid_setup_rows, k_mid_rows and k_mid_cost: the
// count of an element is 0 where its bit is 0 in the slab's maximum count (taken over the kept elements; -inf from a slab that
// keeps none), the known and the u-dependent Gram jobs, c_i / M_i and the streaming cost, as in k_solve_small<.., MASK>.
// MASK is a template parameter: the instances without it are the code they were.  k_mid_setup_fin, k_mid_alpha and
// k_mid_finish are launched as they are; neither idx nor purity goes with a mask.  Two passes frame the call, a workgroup per
// slab each: k_mid_mask_count before the first launch (a solve's kept elements), k_mid_holdout after the last (the squared
// error on the held-out ones).
#include "dmf_mid.h"

namespace dmf {

namespace {

// rows [w rows, (w + 1) rows) of solve b, cut off at N: what the workgroup of slab w reads.  MASK: with solve b's train mask
// (rows of the solve are rows of the problem there: a masked call has no row list)
template <bool MASK = false>
__device__ __forceinline__ RowRange make_slab(const MidArgs& a, int64_t b, int w, const double* u) {
    RowRange p;
    p.V = a.V, p.D = a.D, p.Rt = a.Rt;
    p.idx = a.idx != nullptr ? a.idx + b * a.N : nullptr;
    p.u = u;
    if constexpr (MASK) p.nb = (a.S + 7) / 8, p.mask = a.mask + b * a.N * p.nb;
    else p.mask = nullptr, p.nb = 0;
    p.lo = (int64_t)w * a.rows;
    p.hi = p.lo + a.rows < a.N ? p.lo + a.rows : a.N;
    p.S = a.S, p.n_c = a.n_c, p.n_u = a.n_u, p.K = a.n_c + a.n_u;
    p.SP = pow2_at_least(a.S);
    p.R = kBatchThreads / p.SP;
    return p;
}

// the slab's rows of the partial Gram jobs of solve b
__device__ __forceinline__ GramToMemory slab_partials(const MidArgs& a, int64_t b, int w) {
    return GramToMemory{a.part_g + (b * a.W + w) * (int64_t)a.n_pj * a.S, a.S};
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
    for (int e = threadIdx.x; e < K * S; e += kBatchThreads) {
        const int k = e / S, s = e - k * S;
        al[k * SP + s] = ws_alpha[e];
    }
}

// The per-sample Grams of solve b in LDS (gb: the packed G, then b; rows of SP doubles): the known block from the copy made
// at set-up, the u-dependent entries as the sum of the W slab partials in rising slab order.  jdk, jdu: the rows of gb of the
// known jobs and of the u jobs (fill_jobs), n_known and n_uj of them; nt: the workgroup's threads.
__device__ __forceinline__ void assemble_grams(const MidArgs& a, int64_t b, double* gb, const short* jdk, const short* jdu,
                                               int n_known, int n_uj, int SP, int nt) {
    const int t = threadIdx.x, S = a.S, W = a.W;
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
}

// k_mid_setup_rows' packed-row table: fill_jobs writes it, the slab partials do not go by it.  At namespace scope, so that both
// instances of the template drop it as the kernel did before it was one (a template's own __shared__ arrays are kept whether
// read or not: 304 B more static LDS)
__shared__ short setup_rows_jd[kBatchMaxJobs];

}  // namespace

// ---- set-up, part 1 (grid W x B): the slab's rows of u and u_, its partials of max(D), ||R_trunc||^2, ||u0||^2 and of the
// known Gram jobs.  MASK: the maximum over the slab's KEPT elements (-inf where it keeps none: k_mid_setup_fin's fmax over the
// slabs is then the solve's kept maximum), the Gram jobs with d = 0 where the bit is
template <bool MASK>
__global__ __launch_bounds__(kBatchThreads) void k_mid_setup_rows(MidArgs a) {
    __shared__ double red[kBatchChunk * kBatchThreads];
    __shared__ short jk[kBatchMaxJobs], jl[kBatchMaxJobs];
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x / a.W;
    const int w = (int)(blockIdx.x - b * a.W);
    const int64_t N = a.N;
    const int n_u = a.n_u, n_c = a.n_c, S = a.S;
    double* u = a.u + b * N * n_u;
    double* u_prev = a.u_prev + b * N * n_u;
    const double* u0 = a.u0 + b * N * n_u;
    const RowRange p = make_slab<MASK>(a, b, w, u);
    if (t == 0) fill_jobs(jk, jl, setup_rows_jd, n_c, p.K, true);
    double u2 = 0.0, rt2 = 0.0, dmax = -INFINITY;
    for (int64_t i = p.lo + t; i < p.hi; i += kBatchThreads) {
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
            for (int64_t i = p.lo + r; i < p.hi; i += p.R) {
                if constexpr (MASK) {  // (D.max() of counts * train_mask, as k_solve_small<.., MASK> takes it)
                    if (p.kept(i, s)) dmax = fmax(dmax, p.D[i * S + s]);
                } else {
                    dmax = fmax(dmax, p.D[p.row(i) * S + s]);
                }
            }
    }
    dmax = block_max(dmax, red);
    rt2 = block_sum(rt2, red);
    u2 = block_sum(u2, red);  // (its barriers also publish the job tables)
    double* ps = a.part_s + (b * a.W + w) * kMidSlabScalars;
    if (t == 0) ps[0] = u2, ps[1] = rt2, ps[2] = dmax, ps[3] = 0.0;
    gram_rows<MASK>(p, jk, jl, 0, known_jobs(n_c), red, slab_partials(a, b, w));
}

// ---- set-up, part 2 (grid B; deconvolution.py:192-204): a1 = a2 = 1, alpha_ = alpha = alpha0, d = max(D)^2, l_w, l_h, the
// known Gram block, the momentum ratios of the first iteration.  scal[kBsCf] = +inf: the first prologue compares the first
// cost with it and does not stop.
__global__ __launch_bounds__(kBatchThreads) void k_mid_setup_fin(MidArgs a) {
    __shared__ double red[kBatchThreads];
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
    const int n_known = known_jobs(n_c);
    double* gk = a.gk + b * (int64_t)n_known * S;
    const double* pg = a.part_g + b * W * (int64_t)a.n_pj * S;
    for (int e = t; e < n_known * S; e += kBatchThreads) {
        double sum = 0.0;
        for (int w = 0; w < W; ++w) sum += pg[(int64_t)w * a.n_pj * S + e];
        gk[e] = sum;
    }
    const double* alpha0 = a.alpha0 + b * K * S;
    double* ws_alpha = a.alpha + b * K * S;
    double* ws_alpha_prev = a.alpha_prev + b * K * S;
    for (int e = t; e < K * S; e += kBatchThreads) ws_alpha[e] = ws_alpha_prev[e] = alpha0[e];
    double w2 = 0.0;
    for (int e = t; e < n_u * S; e += kBatchThreads) w2 = fma(alpha0[n_c * S + e], alpha0[n_c * S + e], w2);
    const double l_w = block_sum(w2, red) * dsq;
    double* scal = a.scal + b * kBatchScalars;
    double* ratio_u = a.ratio + b * 2 * a.n_iter2;
    if (t == 0) {
        scal[kBsA1] = fill_ratios(1.0, ratio_u, a.n_iter2);
        scal[kBsLw] = scal[kBsLwPrev] = l_w;
        scal[kBsLh] = scal[kBsLhPrev] = (rt2 + u2) * dsq;
        scal[kBsDsq] = dsq, scal[kBsRtNorm2] = rt2, scal[kBsCf] = INFINITY;
        a.iters[b] = 0;
        a.done[b] = 0;
    }
    if (t == 64) scal[kBsA2] = fill_ratios(1.0, ratio_u + a.n_iter2, a.n_iter2);
}

// ---- the row launch of an outer iteration (grid W x B).  MASK: c_i, M_i and the Gram jobs with d = 0 where the bit is
template <int NU, bool MASK>
__global__ __launch_bounds__(kBatchThreads) void k_mid_rows(MidArgs a) {
    __shared__ double al[kBatchMaxK * kBatchMaxS];
    __shared__ double red[kBatchChunk * kBatchThreads];
    __shared__ short jk[kBatchMaxJobs], jl[kBatchMaxJobs], jd[kBatchMaxJobs];
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x / a.W;
    const int w = (int)(blockIdx.x - b * a.W);
    const double* scal = a.scal + b * kBatchScalars;
    // the stop test of the previous iteration (:218-220), taken by every workgroup of the solve on the same numbers
    if (fabs(cost_of_partials(a, b) - scal[kBsCf]) < a.tol) {
        if (w == 0 && t == 0) a.done[b] = 1;
        return;
    }
    const int64_t N = a.N;
    const int S = a.S, n_c = a.n_c, K = n_c + NU;
    double* u = a.u + b * N * NU;
    double* u_prev = a.u_prev + b * N * NU;
    const RowRange p = make_slab<MASK>(a, b, w, u);
    const int SP = p.SP;
    load_alpha(a.alpha + b * K * S, al, K, S, SP);
    if (t == 0) fill_jobs(jk, jl, jd, n_c, K, false);
    const double l_w = scal[kBsLw], l_w_prev = scal[kBsLwPrev];
    const double* ratio_u = a.ratio + b * 2 * a.n_iter2;
    const int64_t T2 = a.n_iter2;
    __syncthreads();

    // ---- u phase (:81-90), a thread per row
    const double cap_w = 0.9999 * sqrt(l_w_prev / l_w);
    double u2 = 0.0;
    for (int64_t i = p.lo + t; i < p.hi; i += kBatchThreads)
        u2 = u_phase_row<NU, MASK>(p, i, al, ratio_u, T2, cap_w, l_w, a.mode, u, u_prev, u2);
    u2 = block_sum(u2, red);  // (its barriers publish the slab's u to the workgroup)
    if (t == 0) a.part_s[(b * a.W + w) * kMidSlabScalars] = u2;

    // ---- the slab's partial of the u-dependent entries of the per-sample Grams
    gram_rows<MASK>(p, jk, jl, 0, u_jobs(n_c, NU), red, slab_partials(a, b, w));
}

// ---- the alpha launch of an outer iteration (grid B)
__global__ __launch_bounds__(kBatchThreads) void k_mid_alpha(MidArgs a) {
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
    short* jk = reinterpret_cast<short*>(red + kBatchThreads);
    short* jl = jk + kBatchMaxJobs;
    short* jdk = jl + kBatchMaxJobs;   // rows of gb of the known jobs
    short* jdu = jdk + kBatchMaxJobs;  // ... and of the u jobs
    double* ws_alpha = a.alpha + b * K * S;
    double* ws_alpha_prev = a.alpha_prev + b * K * S;
    double* scal = a.scal + b * kBatchScalars;
    double* ratio_u = a.ratio + b * 2 * a.n_iter2;
    double* ratio_h = ratio_u + a.n_iter2;
    const int n_known = known_jobs(n_c), n_uj = u_jobs(n_c, n_u);
    if (t == 0) {
        fill_jobs(jk, jl, jdk, n_c, K, true);
        fill_jobs(jk, jl, jdu, n_c, K, false);
    }
    load_alpha(ws_alpha, al, K, S, SP);
    load_alpha(ws_alpha_prev, ap, K, S, SP);
    const double cf = cost_of_partials(a, b);  // the cost of the iterate this iteration started from
    double u2 = 0.0;
    for (int w = 0; w < W; ++w) u2 += a.part_s[(b * W + w) * kMidSlabScalars];
    const double l_w_old = scal[kBsLw], l_h_prev = scal[kBsLhPrev], dsq = scal[kBsDsq], rt_norm2 = scal[kBsRtNorm2];
    const double a1 = scal[kBsA1], a2 = scal[kBsA2];
    const int64_t T2 = a.n_iter2;
    __syncthreads();
    assemble_grams(a, b, gb, jdk, jdu, n_known, n_uj, SP, kBatchThreads);
    const double l_h = (rt_norm2 + u2) * dsq;  // :212
    __syncthreads();

    // ---- alpha phase (:93-102): thread s owns column s
    if (t < S) alpha_column_steps(gb, al, ap, tmp, srt, t, K, SP, n_pairs, ratio_h, T2, l_h_prev, l_h);
    __syncthreads();
    const double l_w = alpha_u_norm2(al, n_c, n_u, S, SP, red) * dsq;  // :216

    // everything the next launches (or the host) read
    for (int e = t; e < K * S; e += kBatchThreads) {
        const int k = e / S, s = e - k * S;
        ws_alpha[e] = al[k * SP + s];
        ws_alpha_prev[e] = ap[k * SP + s];
    }
    if (t == 0) {
        scal[kBsA1] = fill_ratios(a1, ratio_u, T2);
        scal[kBsLw] = l_w;
        if (T2 > 0) scal[kBsLwPrev] = l_w_old, scal[kBsLhPrev] = l_h;
        scal[kBsLh] = l_h;
        scal[kBsCf] = cf;
        a.iters[b] += 1;
    }
    if (t == 64) scal[kBsA2] = fill_ratios(a2, ratio_h, T2);  // (after the barriers behind the alpha phase, which read it)
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
    const int S = a.S, n_c = a.n_c, n_u = a.n_u, K = n_c + n_u, SP = pow2_at_least(S);
    const int n_pairs = K * (K + 1) / 2;
    double* gb = mid_lds;                  // [K (K + 1) / 2 + K][SP]: packed G, then b
    double* al = gb + (n_pairs + K) * SP;  // [K][SP] alpha
    double* red = al + K * SP;             // [kBatchThreads]: the squares of the unknown block, then their tree
    short* jk = reinterpret_cast<short*>(red + kBatchThreads);
    short* jl = jk + kBatchMaxJobs;
    short* jdk = jl + kBatchMaxJobs;   // rows of gb of the known jobs
    short* jdu = jdk + kBatchMaxJobs;  // ... and of the u jobs
    double* ws_alpha = a.alpha + b * K * S;
    double* scal = a.scal + b * kBatchScalars;
    const int n_known = known_jobs(n_c), n_uj = u_jobs(n_c, n_u);
    if (t == 0) {
        fill_jobs(jk, jl, jdk, n_c, K, true);
        fill_jobs(jk, jl, jdu, n_c, K, false);
    }
    for (int e = t; e < K * S; e += nt) {
        const int k = e / S, s = e - k * S;
        al[k * SP + s] = ws_alpha[e];
    }
    const double cf = cost_of_partials(a, b);  // the cost of the iterate this iteration started from
    const double l_w_old = scal[kBsLw], dsq = scal[kBsDsq], a1 = scal[kBsA1];
    const int64_t T2 = a.n_iter2;
    __syncthreads();
    assemble_grams(a, b, gb, jdk, jdu, n_known, n_uj, SP, nt);
    __syncthreads();

    // ---- Frank-Wolfe: lane k of row s (the barrier inside: every lane has read its alpha before any is replaced)
    {
        const int k = t & 15, s = t >> 4;
        const double x = frank_wolfe_lane<true>(gb, al, purity, k, s, S, n_c, K, SP, n_pairs, T2);
        if (s < S && k < K) al[k * SP + s] = x;
    }
    __syncthreads();

    // ---- l_w = ||alpha[n_c:]||^2 d (:327): the n_u S <= 256 squares, zero-padded to 256, through one fixed tree
    for (int e = t; e < kBatchThreads; e += nt) {
        const int j = e / S, s = e - j * S;
        const double x = e < n_u * S ? al[(n_c + j) * SP + s] : 0.0;
        red[e] = x * x;
    }
    __syncthreads();
    for (int off = kBatchThreads / 2; off > 0; off >>= 1) {
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
        scal[kBsA1] = fill_ratios(a1, a.ratio + b * 2 * a.n_iter2, T2);
        scal[kBsLw] = l_w;
        if (T2 > 0) scal[kBsLwPrev] = l_w_old;
        scal[kBsCf] = cf;
        a.iters[b] += 1;
    }
}

// ---- the cost launch (grid W x B): the slab's partial of the streaming cost of the current iterate (MASK: on the kept
// elements, hence the stop test on them)
template <bool MASK>
__global__ __launch_bounds__(kBatchThreads) void k_mid_cost(MidArgs a) {
    __shared__ double al[kBatchMaxK * kBatchMaxS];
    __shared__ double red[kBatchThreads];
    const int64_t b = blockIdx.x / a.W;
    const int w = (int)(blockIdx.x - b * a.W);
    if (a.done[b]) return;
    const int K = a.n_c + a.n_u;
    const RowRange p = make_slab<MASK>(a, b, w, a.u + b * a.N * a.n_u);
    load_alpha(a.alpha + b * K * a.S, al, K, a.S, p.SP);
    __syncthreads();
    const double cf = stream_cost<MASK>(p, al, red);
    if (threadIdx.x == 0) a.part_cf[b * a.W + w] = cf;
}

// ---- the two framing passes of a masked call (grid W x B each, a workgroup per slab like every row launch).
// n_part[b W + w] = the set bits among the real S positions of slab w's rows of mask b: thread t counts rows lo + t,
// lo + t + 256, ..., the 256 integer partials go through one tree.  Bits of samples >= S in a row's last byte are padding and
// not counted.  Integers: the host adds a solve's W partials in any order.
__global__ __launch_bounds__(kBatchThreads) void k_mid_mask_count(const uint8_t* __restrict__ mask, int64_t N, int S, int64_t rows,
                                                                  int W, long long* __restrict__ n_part) {
    __shared__ long long part[kBatchThreads];
    const int t = threadIdx.x, nb = (S + 7) / 8;
    const int64_t b = blockIdx.x / W;
    const int w = (int)(blockIdx.x - b * W);
    const int64_t lo = (int64_t)w * rows, hi = lo + rows < N ? lo + rows : N;
    const uint8_t* mb = mask + b * N * nb;
    const unsigned int last = (S & 7) ? (1u << (S & 7)) - 1u : 0xFFu;  // the real bits of a row's last byte
    long long n = 0;
    for (int64_t i = lo + t; i < hi; i += kBatchThreads)
        for (int q = 0; q < nb; ++q) n += __popc((unsigned int)mb[i * nb + q] & (q == nb - 1 ? last : 0xFFu));
    part[t] = n;
    __syncthreads();
    for (int off = kBatchThreads / 2; off > 0; off >>= 1) {
        if (t < off) part[t] += part[t + off];
        __syncthreads();
    }
    if (t == 0) n_part[blockIdx.x] = part[0];
}

// part_h[b W + w] = the slab's partial of the sum over the held-out elements (bit 0) of (v - [R_trunc | u_b] alpha_b)^2 on the
// problem's full V with the workspace's iterate (ic.py:80 before the division): threads as (row slice r, sample s) like
// stream_cost, a thread adds its rows in rising order, the partials go through block_sum's tree.  The caller adds a solve's W
// partials in rising slab order.
__global__ __launch_bounds__(kBatchThreads) void k_mid_holdout(MidArgs a, double* __restrict__ part_h) {
    __shared__ double al[kBatchMaxK * kBatchMaxS];
    __shared__ double red[kBatchThreads];
    const int64_t b = blockIdx.x / a.W;
    const int w = (int)(blockIdx.x - b * a.W);
    const int t = threadIdx.x, S = a.S, n_c = a.n_c, n_u = a.n_u, K = n_c + n_u;
    const RowRange p = make_slab<true>(a, b, w, a.u + b * a.N * n_u);
    const int SP = p.SP;
    load_alpha(a.alpha + b * K * S, al, K, S, SP);
    __syncthreads();
    const int s = t & (SP - 1), r = t / SP;
    double acc = 0.0;
    if (s < S) {
        for (int64_t i = p.lo + r; i < p.hi; i += p.R) {
            if (p.kept(i, s)) continue;
            double resid = p.V[i * S + s];
            for (int k = 0; k < n_c; ++k) resid = fma(-p.Rt[i * n_c + k], al[k * SP + s], resid);
            for (int j = 0; j < n_u; ++j) resid = fma(-p.u[i * n_u + j], al[(n_c + j) * SP + s], resid);
            acc = fma(resid, resid, acc);
        }
    }
    const double total = block_sum(acc, red);
    if (t == 0) part_h[blockIdx.x] = total;
}

// ---- cost[b] = the cost of solve b's current iterate, done[b] = its stop test (a thread per solve)
__global__ __launch_bounds__(kBatchThreads) void k_mid_finish(MidArgs a, int64_t B) {
    const int64_t b = (int64_t)blockIdx.x * kBatchThreads + threadIdx.x;
    if (b >= B) return;
    const double cf = cost_of_partials(a, b);
    a.cost[b] = cf;
    if (fabs(cf - a.scal[b * kBatchScalars + kBsCf]) < a.tol) a.done[b] = 1;
}

bool mid_plan(int64_t N, int64_t S, int64_t rows_per_workgroup, MidPlan* out) {
    if (N < 1 || S < 1 || rows_per_workgroup < 0 || out == nullptr) return false;
    int64_t rows = rows_per_workgroup;
    if (rows == 0) rows = kBatchThreads * ((N + (int64_t)kBatchThreads * kMidMaxW - 1) / ((int64_t)kBatchThreads * kMidMaxW));
    if (rows % kBatchThreads != 0) return false;
    const int64_t W = (N + rows - 1) / rows;
    if (W > kMidMaxW) return false;
    int64_t every = S <= ((int64_t)1 << 22) / N ? ((int64_t)1 << 22) / (N * S) : 0;
    every = every < 4 ? 4 : (every > 16 ? 16 : every);
    out->rows = rows, out->W = (int)W, out->check_every = (int)every;
    return true;
}

size_t mid_alpha_lds_bytes(int S, int K) {
    const int SP = pow2_at_least(S);
    const size_t doubles = (size_t)(K * (K + 1) / 2 + K) * SP + 4 * (size_t)K * SP + kBatchThreads;
    return doubles * sizeof(double) + (4 * kBatchMaxJobs * sizeof(short) + 7) / 8 * 8;
}

size_t mid_alpha_fw_lds_bytes(int S, int K) {
    const int SP = pow2_at_least(S);
    const size_t doubles = (size_t)(K * (K + 1) / 2 + K) * SP + (size_t)K * SP + kBatchThreads;
    return doubles * sizeof(double) + (4 * kBatchMaxJobs * sizeof(short) + 7) / 8 * 8;
}

static bool mid_args_ok(const MidArgs& a, int64_t B) {
    if (!batch_supported(a.N, a.S, a.n_c, a.n_u, a.mode, kMidMaxElements) || B < 1) return false;
    if (a.rows < kBatchThreads || a.rows % kBatchThreads != 0 || a.W < 1 || a.W > kMidMaxW) return false;
    if ((int64_t)(a.W - 1) * a.rows >= a.N || (int64_t)a.W * a.rows < a.N) return false;  // the slabs cover the rows exactly
    if (a.n_pj != mid_slab_jobs(a.n_c, a.n_u) || a.n_iter2 < 0) return false;
    if (a.mask != nullptr && a.idx != nullptr) return false;  // a train mask per solve: no row list goes with it
    return B <= 0x7fffffff / a.W;
}

hipError_t launch_mid_setup(const MidArgs& a, int64_t B, hipStream_t st) {
    if (!mid_args_ok(a, B)) return hipErrorInvalidValue;
    const dim3 slabs((unsigned)(B * a.W)), threads(kBatchThreads);
    if (a.mask != nullptr) hipLaunchKernelGGL(k_mid_setup_rows<true>, slabs, threads, 0, st, a);
    else hipLaunchKernelGGL(k_mid_setup_rows<false>, slabs, threads, 0, st, a);
    hipLaunchKernelGGL(k_mid_setup_fin, dim3((unsigned)B), threads, 0, st, a);
    if (a.mask != nullptr) hipLaunchKernelGGL(k_mid_cost<true>, slabs, threads, 0, st, a);
    else hipLaunchKernelGGL(k_mid_cost<false>, slabs, threads, 0, st, a);
    return hipGetLastError();
}

template <int NU>
static void launch_rows(const MidArgs& a, int64_t B, hipStream_t st) {
    const dim3 slabs((unsigned)(B * a.W)), threads(kBatchThreads);
    if (a.mask != nullptr) hipLaunchKernelGGL((k_mid_rows<NU, true>), slabs, threads, 0, st, a);
    else hipLaunchKernelGGL((k_mid_rows<NU, false>), slabs, threads, 0, st, a);
}

hipError_t launch_mid_iteration(const MidArgs& a, int64_t B, hipStream_t st, const double* purity) {
    if (!mid_args_ok(a, B)) return hipErrorInvalidValue;
    // the purity variant: partial mode with a known block to hold at that mass
    if (purity != nullptr && (a.mode != DMF_MODE_PARTIAL || a.n_c < 1 || a.mask != nullptr)) return hipErrorInvalidValue;
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
        hipLaunchKernelGGL(k_mid_alpha, dim3((unsigned)B), dim3(kBatchThreads), lds, st, a);
    if (a.mask != nullptr) hipLaunchKernelGGL(k_mid_cost<true>, dim3((unsigned)(B * a.W)), dim3(kBatchThreads), 0, st, a);
    else hipLaunchKernelGGL(k_mid_cost<false>, dim3((unsigned)(B * a.W)), dim3(kBatchThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_mid_mask_count(const uint8_t* mask, int64_t B, int64_t N, int S, int64_t rows, int W, long long* n_part,
                                 hipStream_t st) {
    if (mask == nullptr || n_part == nullptr || B < 1 || N < 1 || S < 1 || S > kBatchMaxS || rows < kBatchThreads || W < 1 ||
        W > kMidMaxW || (int64_t)(W - 1) * rows >= N || (int64_t)W * rows < N || B > 0x7fffffff / W)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mid_mask_count, dim3((unsigned)(B * W)), dim3(kBatchThreads), 0, st, mask, N, S, rows, W, n_part);
    return hipGetLastError();
}

hipError_t launch_mid_holdout(const MidArgs& a, int64_t B, double* part_h, hipStream_t st) {
    if (!mid_args_ok(a, B) || a.mask == nullptr || part_h == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mid_holdout, dim3((unsigned)(B * a.W)), dim3(kBatchThreads), 0, st, a, part_h);
    return hipGetLastError();
}

hipError_t launch_mid_finish(const MidArgs& a, int64_t B, hipStream_t st) {
    if (!mid_args_ok(a, B) || a.cost == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mid_finish, dim3((unsigned)((B + kBatchThreads - 1) / kBatchThreads)), dim3(kBatchThreads), 0, st, a, B);
    return hipGetLastError();
}

}  // namespace dmf
