// Reference-based regression (wls_intercept, init_func.py:8-14) for every sample at once.
//
// scikit-learn centres R = [R_trunc | u] and the target t by their weighted means, scales the rows by sqrt(w) and hands the
// result to scipy's NNLS.  With w = d_s and the per-sample sums  sw = sum w,  st = sum w t,  m_k = sum w R_k,
// r_k = sum w t R_k,  G_kl = sum w R_k R_l  the centred normal equations are
//     A^T A = G - m m^T / sw          A^T y = r - m st / sw
// and the NNLS solution depends on (A^T A, A^T y) alone.  G is the dense part of the packed Gram the library already builds
// (dmf_problem::gb_known, a solver's gb); k_wls_moments streams the rows once for the first moments, k_nnls_intercept runs
// Lawson-Hanson on the K x K system of one sample per wave.
#include "dmf_dispatch.h"
#include "dmf_internal.h"

namespace dmf {

constexpr int kWlsCols = 16;  // columns of R resident per lane in k_wls_moments (one grid.z slice per 16 columns)

// ------------------------------------------------------------------------------------------------ first moments
// Lane = sample, wave = row (k_bu_cols' layout): a row's R values are wave-uniform loads, four rows in flight per wave.
// U16: the row's weight and target come from (X16, D16) -- x = v d exactly, so w t = x (target v) or d x (target d v) is an
// integer product -- else from V and the f64 counts.  Grid (row blocks, 64-sample blocks, 16-column slices); the four waves
// of a workgroup are summed in fixed order into one slab per workgroup:
//     slab[bx][row][S], rows 0..K-1 = m_k, K..2K-1 = r_k, 2K = sw, 2K+1 = st (the last two from column slice 0).
template <bool U16>
__global__ __launch_bounds__(256) void k_wls_moments(const double* __restrict__ V, const double* __restrict__ D,
                                                     const unsigned short* __restrict__ X16,
                                                     const unsigned short* __restrict__ D16, int SD,
                                                     const double* __restrict__ Rt, int n_c, const double* __restrict__ u,
                                                     int n_u, int64_t N, int S, int target_dv, double* __restrict__ slab) {
    constexpr int KC = kWlsCols, kRows = 4, NACC = 2 * KC + 2;
    __shared__ double red[3][NACC][64];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int s = blockIdx.y * 64 + lane;
    const bool active = s < S;
    const int sc = active ? s : S - 1;
    const int K = n_c + n_u, c0 = blockIdx.z * KC;
    double am[KC], ar[KC], sw = 0.0, st = 0.0;
#pragma unroll
    for (int j = 0; j < KC; ++j) am[j] = ar[j] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * 4;
    for (int64_t i0 = (int64_t)blockIdx.x * 4 + wave; i0 < N; i0 += kRows * stride) {
        double w[kRows], wt[kRows];
        int64_t row[kRows];
#pragma unroll
        for (int x = 0; x < kRows; ++x) {
            const int64_t i = i0 + x * stride;
            row[x] = i < N ? i : N - 1;
            if constexpr (U16) {
                const double d = i < N ? (double)D16[row[x] * SD + sc] : 0.0;
                const double xm = (double)X16[row[x] * SD + sc];
                w[x] = d;
                wt[x] = i < N ? (target_dv ? d * xm : xm) : 0.0;
            } else {
                const double d = i < N ? D[row[x] * S + sc] : 0.0;
                const double v = V[row[x] * S + sc];
                w[x] = d;
                wt[x] = d * (target_dv ? d * v : v);
            }
        }
#pragma unroll
        for (int x = 0; x < kRows; ++x) {
            sw += w[x];
            st += wt[x];
            const double* __restrict__ rt_row = Rt + row[x] * n_c;
            const double* __restrict__ u_row = u + row[x] * n_u;
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                const int c = c0 + j;  // (wave-uniform)
                if (c < K) {
                    const double rv = c < n_c ? rt_row[c] : u_row[c - n_c];
                    am[j] = fma(w[x], rv, am[j]);
                    ar[j] = fma(wt[x], rv, ar[j]);
                }
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            red[wave - 1][j][lane] = am[j];
            red[wave - 1][KC + j][lane] = ar[j];
        }
        red[wave - 1][2 * KC][lane] = sw;
        red[wave - 1][2 * KC + 1][lane] = st;
    }
    __syncthreads();
    if (wave == 0 && active) {
        double* __restrict__ out = slab + (int64_t)blockIdx.x * (2 * K + 2) * S + s;
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const int c = c0 + j;
            if (c < K) {
                out[(int64_t)c * S] = ((am[j] + red[0][j][lane]) + red[1][j][lane]) + red[2][j][lane];
                out[(int64_t)(K + c) * S] = ((ar[j] + red[0][KC + j][lane]) + red[1][KC + j][lane]) + red[2][KC + j][lane];
            }
        }
        if (c0 == 0) {
            out[(int64_t)(2 * K) * S] = ((sw + red[0][2 * KC][lane]) + red[1][2 * KC][lane]) + red[2][2 * KC][lane];
            out[(int64_t)(2 * K + 1) * S] = ((st + red[0][2 * KC + 1][lane]) + red[1][2 * KC + 1][lane]) + red[2][2 * KC + 1][lane];
        }
    }
}

// mom[row][s] = the slabs' sum in a fixed order: thread group g (of four) adds slabs g, g + 4, ... in rising order, the
// four shares are then added as ((0 + 1) + 2) + 3.  Grid (64-sample blocks, rows).
__global__ __launch_bounds__(256) void k_wls_reduce(const double* __restrict__ slab, int n_slabs, int n_rows, int S,
                                                    double* __restrict__ mom) {
    __shared__ double part[3][64];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int s = blockIdx.x * 64 + lane, row = blockIdx.y;
    const bool active = s < S;
    const int sc = active ? s : S - 1;
    double acc = 0.0;
    for (int b = grp; b < n_slabs; b += 4) acc += slab[((int64_t)b * n_rows + row) * S + sc];
    if (grp > 0) part[grp - 1][lane] = acc;
    __syncthreads();
    if (grp == 0 && active) mom[(int64_t)row * S + s] = ((acc + part[0][lane]) + part[1][lane]) + part[2][lane];
}

int wls_moments_grid(int64_t N) {
    int64_t want = (N + 4 * 4 - 1) / (4 * 4);
    if (want > 512) want = 512;
    return (int)(want < 1 ? 1 : want);
}

int64_t wls_slab_doubles(int64_t N, int S, int K) { return (int64_t)wls_moments_grid(N) * (2 * K + 2) * S; }

hipError_t launch_wls_moments(const ProblemView& p, const double* u, int n_u, int target_dv, double* slab, double* mom,
                              hipStream_t st) {
    const int K = p.n_c + n_u, nbx = wls_moments_grid(p.N);
    const dim3 grid(nbx, (p.S + 63) / 64, (K + kWlsCols - 1) / kWlsCols), block(256);
    const bool u16 = p.X16 != nullptr && p.D16 != nullptr;
    const hipError_t e = dispatch_bool(u16, [&](auto f) {
        hipLaunchKernelGGL((k_wls_moments<decltype(f)::value>), grid, block, 0, st, p.V, p.D, p.X16, p.D16, p.SD, p.Rt, p.n_c, u,
                           n_u, p.N, p.S, target_dv, slab);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_wls_reduce, dim3((p.S + 63) / 64, 2 * K + 2), block, 0, st, slab, nbx, 2 * K + 2, p.S, mom);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ active-set solve
// One wave per sample.  LDS: M[K][LD] (LD = K | 1) holds the centred normal matrix in its upper triangle (diagonal
// included) and the Cholesky factor of the current passive block, by passive ordinal, in its strict lower triangle.
// Every loop below has a fixed bound; every branch around a barrier or a shuffle is wave-uniform.

__device__ __forceinline__ double wls_a(const double* M, int LD, int i, int j) { return M[(i < j ? i : j) * LD + (i < j ? j : i)]; }

// Cholesky of the passive block (rows / columns plist[0..np)), left-looking, lane = row.  false: a pivot fell below
// tol_k * A_jj (the column depends on the ones before it as far as f64 normal equations can tell).
__device__ bool wls_factor(double* M, int LD, const int* plist, const double* adiag, double* ldiag, int np, int lane,
                           double tol_k) {
    const int pi = lane < np ? plist[lane] : 0;
    for (int j = 0; j < np; ++j) {
        const int pj = plist[j];
        double v = 0.0;
        if (lane >= j && lane < np) {
            v = wls_a(M, LD, pi, pj);
            for (int k = 0; k < j; ++k) v -= M[lane * LD + k] * M[j * LD + k];
        }
        const double piv = __shfl(v, j);
        if (!(piv > tol_k * adiag[pj])) return false;
        const double d = sqrt(piv);
        if (lane == j) ldiag[j] = d;
        if (lane > j && lane < np) M[lane * LD + j] = v / d;
        __syncthreads();
    }
    return true;
}

// L L^T s = rhs for the factor above; rhs and the result by passive ordinal (lane = ordinal)
__device__ double wls_solve(const double* M, int LD, const double* ldiag, int np, int lane, double rhs) {
    double acc = 0.0, z = 0.0;
    for (int j = 0; j < np; ++j) {
        const double zj = __shfl((rhs - acc) / ldiag[j], j);
        if (lane == j) z = zj;
        if (lane > j && lane < np) acc = fma(M[lane * LD + j], zj, acc);
    }
    double sol = 0.0;
    acc = 0.0;
    for (int j = np - 1; j >= 0; --j) {
        const double sj = __shfl((z - acc) / ldiag[j], j);
        if (lane == j) sol = sj;
        if (lane < j) acc = fma(M[j * LD + lane], sj, acc);
    }
    return sol;
}

// Lawson-Hanson as scipy's nnls runs it (enter the largest positive dual; a candidate whose own coefficient comes out
// non-positive is dropped for this round; step back along x + a (s - x) while a passive coefficient is non-positive; at
// most 3 K solves), on the normal equations.  status: 0 solved, 1 not solved here (the K x K matrix is rank-deficient to
// K eps, a pivot fell below that, or the cap was reached), 2 the weights sum to zero.  out (K x S) <- coef / max(sum coef,
// 1e-10) for status 0 only.
__global__ __launch_bounds__(64) void k_nnls_intercept(const double* __restrict__ gb, const double* __restrict__ mom, int K,
                                                       int S, double* __restrict__ out, int* __restrict__ status) {
    extern __shared__ double wls_lds[];
    const int s = blockIdx.x, lane = threadIdx.x;
    const int LD = K | 1;
    double* M = wls_lds;
    double* adiag = M + K * LD;
    double* ldiag = adiag + K;
    double* xs = ldiag + K;
    int* plist = reinterpret_cast<int*>(xs + K);
    int* pflag = plist + K;
    const bool var = lane < K;
    const double sw = mom[(int64_t)(2 * K) * S + s], st = mom[(int64_t)(2 * K + 1) * S + s];
    if (!(sw > 0.0)) {
        if (lane == 0) status[s] = 2;
        return;
    }
    const double m_i = var ? mom[(int64_t)lane * S + s] : 0.0;
    const double r_i = var ? mom[(int64_t)(K + lane) * S + s] : 0.0;
    for (int j = 0; j < K; ++j) {
        const double m_j = __shfl(m_i, j);
        if (lane <= j) M[lane * LD + j] = gb[(int64_t)tri(lane, j) * S + s] - m_i * m_j / sw;
    }
    const double b_i = r_i - m_i * st / sw;
    if (var) {
        adiag[lane] = M[lane * LD + lane];
        xs[lane] = 0.0;
        plist[lane] = lane;
        pflag[lane] = 0;
    }
    __syncthreads();
    const double tol_k = (double)K * 0x1p-52;
    const int cap = 3 * K;
    int code = 0;
    if (!wls_factor(M, LD, plist, adiag, ldiag, K, lane, tol_k)) code = 1;
    int np = 0, iter = 0;
    bool optimal = false;  // no dual left to enter: the Kuhn-Tucker conditions hold
    for (int outer = 0; outer <= cap && code == 0; ++outer) {
        // dual of the variables outside the passive set
        const bool free_var = var && pflag[lane] == 0;
        double w = 0.0;
        if (free_var) {
            w = b_i;
            for (int q = 0; q < np; ++q) {
                const int j = plist[q];
                w -= wls_a(M, LD, lane, j) * xs[j];
            }
        }
        __syncthreads();
        unsigned long long rejected = 0;
        bool entered = false;
        double sol = 0.0;
        for (int c = 0; c < K; ++c) {
            double wm = (free_var && !((rejected >> lane) & 1ull)) ? w : -1.0;
            int im = lane;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double wo = __shfl_xor(wm, off);
                const int io = __shfl_xor(im, off);
                if (wo > wm || (wo == wm && io < im)) wm = wo, im = io;
            }
            if (!(wm > 0.0)) break;
            if (lane == 0) plist[np] = im;
            __syncthreads();
            if (++iter > cap || !wls_factor(M, LD, plist, adiag, ldiag, np + 1, lane, tol_k)) {
                code = 1;
                break;
            }
            sol = wls_solve(M, LD, ldiag, np + 1, lane, __shfl(b_i, lane <= np ? plist[lane] : 0));
            if (__shfl(sol, np) > 0.0) {
                if (lane == 0) pflag[im] = 1;
                np += 1;
                entered = true;
                break;
            }
            rejected |= 1ull << im;
        }
        __syncthreads();
        if (code != 0) break;
        if (!entered) {
            optimal = true;
            break;
        }
        // the passive solve is feasible, or x steps towards it until a coefficient reaches zero and leaves the set
        bool settled = false;
        for (int inner = 0; inner <= K; ++inner) {
            const bool pas = lane < np;
            const int pi = pas ? plist[lane] : 0;
            const double xq = pas ? xs[pi] : 0.0;
            const bool bad = pas && !(sol > 0.0);
            if (__ballot(bad) == 0ull) {
                if (pas) xs[pi] = sol;
                __syncthreads();
                settled = true;
                break;
            }
            double ratio = bad ? (xq > 0.0 ? xq / (xq - sol) : 0.0) : 2.0;
            double rm = ratio;
            int qa = lane;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double ro = __shfl_xor(rm, off);
                const int qo = __shfl_xor(qa, off);
                if (ro < rm || (ro == rm && qo < qa)) rm = ro, qa = qo;
            }
            double xn = xq + rm * (sol - xq);
            if (lane == qa) xn = 0.0;
            const bool keep = pas && xn > 0.0;
            const unsigned long long mask = __ballot(keep);
            const int pos = __popcll(mask & ((1ull << lane) - 1ull));
            __syncthreads();
            if (pas) {
                xs[pi] = keep ? xn : 0.0;
                if (!keep) pflag[pi] = 0;
            }
            if (keep) plist[pos] = pi;
            np = __popcll(mask);
            __syncthreads();
            if (np == 0) {
                settled = true;
                break;
            }
            if (++iter > cap || !wls_factor(M, LD, plist, adiag, ldiag, np, lane, tol_k)) {
                code = 1;
                break;
            }
            sol = wls_solve(M, LD, ldiag, np, lane, __shfl(b_i, lane < np ? plist[lane] : 0));
        }
        if (code == 0 && !settled) code = 1;
        if (code != 0) break;
    }
    if (code == 0 && !optimal) code = 1;
    if (code != 0) {
        if (lane == 0) status[s] = code;
        return;
    }
    const double x_i = var ? xs[lane] : 0.0;
    double total = x_i;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) total += __shfl_xor(total, off);
    if (var) out[(int64_t)lane * S + s] = x_i / fmax(total, 1e-10);
    if (lane == 0) status[s] = 0;
}

hipError_t launch_nnls_intercept(const double* gb, const double* mom, int K, int S, double* out, int* status, hipStream_t st) {
    const int LD = K | 1;
    const size_t lds = ((size_t)K * LD + 3 * (size_t)K) * sizeof(double) + 2 * (size_t)K * sizeof(int);
    hipLaunchKernelGGL(k_nnls_intercept, dim3(S), dim3(64), lds, st, gb, mom, K, S, out, status);
    return hipGetLastError();
}

}  // namespace dmf
