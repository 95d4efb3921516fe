// The SVD initialiser (constrained_nndsvd / nndsvd_initialize, init_func.py:17-82) without an SVD of the N x S matrix.
//
// The reference factors Yres = max(Y - R_trunc H1, 1e-8) (or Y itself, unsupervised) as U diag(sigma) E^T and builds the
// NNDSVD factors from the leading `rank` triples.  Here the S x S Gram C = Yres^T Yres is accumulated on the FP64 matrix
// cores in one pass over the rows (k_svd_gram), the host takes its symmetric eigendecomposition (sigma_j = sqrt(lambda_j),
// e_j), a second pass projects the rows on the e_j / sigma_j (k_svd_project: t_ij = u_ij, with the norms of the positive
// and negative parts of every column), and k_svd_finish turns T into u0 in place.  Yres is never stored: both passes form
// it on the fly from the resident f64 V, R_trunc and H1.
//
// Shapes: any N >= 1, S <= 512, n_c <= 64, rank <= 64, and k_svd_project's LDS within the 160 KB of a CU (the e_j / sigma_j
// columns live there: every rank up to S = 256, rank 30 at S = 512).
//
// Budget.  k_svd_gram, 256 threads: LDS = a 16-row tile of Yres, 16 x (S rounded up to 64, + 16) doubles = 34 KB at
// S = 256, 66 KB at S = 512; H1 is not staged (it would be 96 KB at n_c = 48, S = 256): a thread owns a column of the tile,
// reads H1[c][s] once per c and tile -- a coalesced load that the 16 rows share -- and R_trunc[row][c] through the scalar
// cache (the row is wave-uniform).  Accumulators: NB (1 or 2) 64 x 64 blocks of C per wave, 16 tiles x 4 doubles each, i.e.
// 128 / 256 of the 512 registers a lane of a one-wave-per-SIMD workgroup has (hipcc: 119 + 128 and 255 + 216 VGPRs + AGPRs,
// no spills; three blocks spill).  A workgroup so covers 8 of the NG (NG + 1) / 2 block pairs, NG = ceil(S / 64): all of
// them up to S = 192, two workgroups per row slab at S = 256 (10 pairs), five at S = 512 (36); each forms the tile again.
// k_svd_project: LDS = S x rank doubles + an 8-row tile (<= 33 KB) + 4 KB of partial norms, 160 KB at most
// (149 KB at S = 256, rank = 64).
//
// Every sum has a fixed order: a workgroup walks its row tiles in rising order, writes its partial result to a slab of
// its own, and a reduce kernel adds the slabs as k_wls_reduce does.  The grids depend on (N, S) alone, so do the results.
// No atomics on doubles; no workgroup waits for another.
#include "dmf_dispatch.h"
#include "dmf_internal.h"

namespace dmf {

using v4d = __attribute__((ext_vector_type(4))) double;

constexpr int kSvdThreads = 256;
constexpr int kSvdGramRows = 16;     // rows per tile of k_svd_gram (4 k-steps of v_mfma_f64_16x16x4_f64)
constexpr int kSvdProjectRows = 8;   // rows per tile of k_svd_project
constexpr int kSvdPad = 16;          // doubles between the rows of a tile: consecutive rows start 32 banks apart
constexpr int kSvdMaxGrid = 256;     // workgroups of a pass at most (one per CU)

__host__ __device__ inline int svd_sp(int S) { return (S + 63) / 64 * 64; }

// ROWS rows of Yres from row0 on -> tile[ROWS][LD], columns [S, SP) and rows past N zero.  Thread = column.  neg / bad:
// the thread's counts of negative and non-finite entries of Y.
template <int ROWS>
__device__ __forceinline__ void svd_fill_tile(const double* __restrict__ V, const double* __restrict__ Rt,
                                              const double* __restrict__ H1, int n_c, int64_t N, int S, int SP, int LD,
                                              int64_t row0, double* __restrict__ tile, int& neg, int& bad) {
    for (int s = threadIdx.x; s < SP; s += kSvdThreads) {
        double y[ROWS];
        const bool in = s < S;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int64_t row = row0 + r;
            const bool live = in && row < N;
            const double v = live ? V[row * S + s] : 0.0;
            y[r] = v;
            neg += v < 0.0;
            bad += !(fabs(v) <= 1.79769313486231570815e308);
        }
        if (n_c > 0 && in) {
            for (int c = 0; c < n_c; ++c) {
                const double h = H1[(int64_t)c * S + s];
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const int64_t row = row0 + r < N ? row0 + r : N - 1;  // (wave-uniform: a scalar load)
                    y[r] = fma(-Rt[row * n_c + c], h, y[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < ROWS; ++r) y[r] = row0 + r < N ? fmax(y[r], 1e-8) : 0.0;
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) tile[r * LD + s] = y[r];
    }
}

// ------------------------------------------------------------------------------------------------ C = Yres^T Yres
// Grid (row slabs, groups of 4 NB block pairs).  C is cut into 64 x 64 blocks; the pairs (bi <= bj) are numbered
// p = tri(bi, bj); wave w of workgroup (bx, by) owns the pairs 4 NB by + 4 b + w, b < NB.  Per 4-row strip of the tile a
// lane holds, for each of the block's four 16-column tiles, the element [row l >> 4][column l & 15]: as the A operand it
// is Yres^T (m = sample, k = row), as the B operand Yres (k = row, n = sample).
// slab[bx][p][64][64] <- the workgroup's share of block p (diagonal blocks whole); flags[bx][2] <- (negative, non-finite)
// entries of Y among the workgroup's rows, from the by = 0 workgroups.
template <int NB>
__global__ __launch_bounds__(kSvdThreads) void k_svd_gram(const double* __restrict__ V, const double* __restrict__ Rt,
                                                          const double* __restrict__ H1, int n_c, int64_t N, int S,
                                                          double* __restrict__ slab, int* __restrict__ flags) {
    extern __shared__ double svd_lds[];
    __shared__ int cnt[2];
    const int SP = svd_sp(S), LD = SP + kSvdPad, NG = SP / 64, P = NG * (NG + 1) / 2;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int lrow = lane >> 4, lcol = lane & 15;
    int bi[NB], bj[NB];
    bool own[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int p = (blockIdx.y * NB + b) * 4 + wave;
        own[b] = p < P;
        int j = 0;
        while ((j + 1) * (j + 2) / 2 <= p && j + 1 < NG) ++j;
        bj[b] = j;
        bi[b] = own[b] ? p - j * (j + 1) / 2 : 0;
    }
    v4d acc[NB][4][4];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int ta = 0; ta < 4; ++ta)
#pragma unroll
            for (int tb = 0; tb < 4; ++tb) acc[b][ta][tb] = v4d{0.0, 0.0, 0.0, 0.0};
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    int neg = 0, bad = 0;
    const int64_t n_tiles = (N + kSvdGramRows - 1) / kSvdGramRows;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        __syncthreads();  // (the previous tile has been read)
        svd_fill_tile<kSvdGramRows>(V, Rt, H1, n_c, N, S, SP, LD, t * kSvdGramRows, svd_lds, neg, bad);
        __syncthreads();
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (!own[b]) continue;  // (wave-uniform)
#pragma unroll
            for (int strip = 0; strip < kSvdGramRows / 4; ++strip) {
                const double* __restrict__ row = svd_lds + (strip * 4 + lrow) * LD + lcol;
                double a[4], bb[4];
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    a[x] = row[64 * bi[b] + 16 * x];
                    bb[x] = row[64 * bj[b] + 16 * x];
                }
#pragma unroll
                for (int ta = 0; ta < 4; ++ta)
#pragma unroll
                    for (int tb = 0; tb < 4; ++tb)
                        acc[b][ta][tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ta], bb[tb], acc[b][ta][tb], 0, 0, 0);
            }
        }
    }
    // C/D layout of the f64 form: register r of lane l is element [row (l >> 4) + 4 r][column l & 15]
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (!own[b]) continue;
        const int p = (blockIdx.y * NB + b) * 4 + wave;
        double* __restrict__ out = slab + ((int64_t)blockIdx.x * P + p) * 4096;
#pragma unroll
        for (int ta = 0; ta < 4; ++ta)
#pragma unroll
            for (int tb = 0; tb < 4; ++tb)
#pragma unroll
                for (int r = 0; r < 4; ++r) out[(16 * ta + lrow + 4 * r) * 64 + 16 * tb + lcol] = acc[b][ta][tb][r];
    }
    if (blockIdx.y == 0) {
        __syncthreads();
        if (neg) atomicAdd(&cnt[0], neg);
        if (bad) atomicAdd(&cnt[1], bad);
        __syncthreads();
        if (threadIdx.x < 2) flags[blockIdx.x * 2 + threadIdx.x] = cnt[threadIdx.x];
    }
}

// C[i][j] = C[j][i] = the slabs' sum of element (i, j), i <= j, in k_wls_reduce's order: thread group g (of four) adds
// slabs g, g + 4, ... in rising order, the shares are added as ((0 + 1) + 2) + 3.  Grid (64-column blocks, rows).
__global__ __launch_bounds__(256) void k_svd_gram_reduce(const double* __restrict__ slab, int n_slabs, int S,
                                                         double* __restrict__ C) {
    __shared__ double part[3][64];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int i = blockIdx.y, j = blockIdx.x * 64 + lane;
    const int NG = svd_sp(S) / 64, P = NG * (NG + 1) / 2;
    const bool active = j < S && i <= j;
    double acc = 0.0;
    if (active) {
        const int p = tri(i >> 6, blockIdx.x);
        const double* __restrict__ src = slab + (int64_t)p * 4096 + (i & 63) * 64 + lane;
        for (int b = grp; b < n_slabs; b += 4) acc += src[(int64_t)b * P * 4096];
    }
    if (grp > 0) part[grp - 1][lane] = acc;
    __syncthreads();
    if (grp == 0 && active) {
        const double v = ((acc + part[0][lane]) + part[1][lane]) + part[2][lane];
        C[(int64_t)i * S + j] = v;
        C[(int64_t)j * S + i] = v;
    }
}

int svd_gram_blocks_per_wave(int S) {
    const int NG = svd_sp(S) / 64, P = NG * (NG + 1) / 2;
    const int nb = (P + 3) / 4;
    return nb > 2 ? 2 : nb;  // (three blocks per wave spill: 384 accumulator registers beside the tile fill's)
}

static int svd_gram_ny(int S) {
    const int NG = svd_sp(S) / 64, P = NG * (NG + 1) / 2, per = 4 * svd_gram_blocks_per_wave(S);
    return (P + per - 1) / per;
}

int svd_gram_grid(int64_t N, int S) {
    int64_t want = (N + kSvdGramRows - 1) / kSvdGramRows;
    const int cap = kSvdMaxGrid / svd_gram_ny(S);
    if (want > cap) want = cap;
    return (int)(want < 1 ? 1 : want);
}

int64_t svd_gram_slab_doubles(int64_t N, int S) {
    const int NG = svd_sp(S) / 64, P = NG * (NG + 1) / 2;
    return (int64_t)svd_gram_grid(N, S) * P * 4096;
}

size_t svd_project_lds_bytes(int S, int rank) {
    return ((size_t)S * rank + (size_t)kSvdProjectRows * (svd_sp(S) + kSvdPad) + 2 * kSvdThreads) * sizeof(double);
}

bool svd_supported(int S, int n_c, int rank) {
    return S >= 1 && S <= kSvdMaxS && n_c >= 0 && n_c <= kSvdMaxNc && rank >= 0 && rank <= kSvdMaxRank &&
           svd_project_lds_bytes(S, rank) <= kSvdMaxLds;
}

hipError_t launch_svd_gram(const ProblemView& p, const double* H1, double* slab, int* flags, double* C, hipStream_t st) {
    const int nbx = svd_gram_grid(p.N, p.S), ny = svd_gram_ny(p.S);
    const size_t lds = (size_t)kSvdGramRows * (svd_sp(p.S) + kSvdPad) * sizeof(double);
    const hipError_t e = dispatch_int<1, 2>(svd_gram_blocks_per_wave(p.S), [&](auto nb) {
        constexpr int NB = decltype(nb)::value;
        const hipError_t er = raise_dynamic_lds<k_svd_gram<NB>>(lds);
        if (er != hipSuccess) return er;
        hipLaunchKernelGGL((k_svd_gram<NB>), dim3(nbx, ny), dim3(kSvdThreads), lds, st, p.V, p.Rt, H1, p.n_c, p.N, p.S, slab,
                           flags);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_svd_gram_reduce, dim3(svd_sp(p.S) / 64, p.S), dim3(256), 0, st, slab, nbx, p.S, C);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ T = Yres E / sigma
// LDS: Es[S][rank] (the e_j / sigma_j columns), an 8-row tile of Yres, the partial norms.  Thread (j = tid % RP,
// g = tid / RP), RP = rank rounded up to a power of two: component j of the rows g, g + 256 / RP, ... of the tile; a lane's
// dot product runs over the samples in four interleaved chains of fixed order.  T[N][rank] <- t; slab[bx][2][rank] <- the workgroup's sums of
// max(t, 0)^2 and max(-t, 0)^2 per component (thread groups added in rising order).
__global__ __launch_bounds__(kSvdThreads) void k_svd_project(const double* __restrict__ V, const double* __restrict__ Rt,
                                                             const double* __restrict__ H1, int n_c, int64_t N, int S,
                                                             const double* __restrict__ Es, int rank, int RP,
                                                             double* __restrict__ T, double* __restrict__ slab) {
    extern __shared__ double svd_lds[];
    const int SP = svd_sp(S), LD = SP + kSvdPad;
    double* es = svd_lds;
    double* tile = es + (int64_t)S * rank;
    double* red = tile + kSvdProjectRows * LD;  // [2][kSvdThreads]
    for (int x = threadIdx.x; x < S * rank; x += kSvdThreads) es[x] = Es[x];
    const int j = threadIdx.x & (RP - 1), g = threadIdx.x / RP, ng = kSvdThreads / RP;
    const bool comp = j < rank;
    double pos = 0.0, ngt = 0.0;
    int neg = 0, bad = 0;
    const int64_t n_tiles = (N + kSvdProjectRows - 1) / kSvdProjectRows;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        __syncthreads();
        svd_fill_tile<kSvdProjectRows>(V, Rt, H1, n_c, N, S, SP, LD, t * kSvdProjectRows, tile, neg, bad);
        __syncthreads();
        for (int r = g; r < kSvdProjectRows; r += ng) {
            const int64_t row = t * kSvdProjectRows + r;
            if (!comp || row >= N) continue;
            const double* __restrict__ y = tile + r * LD;
            double a4[4] = {0.0, 0.0, 0.0, 0.0};  // (four chains, sample s in chain s & 3, added as ((0 + 1) + 2) + 3)
            int s = 0;
            for (; s + 4 <= S; s += 4)
#pragma unroll
                for (int x = 0; x < 4; ++x) a4[x] = fma(y[s + x], es[(s + x) * rank + j], a4[x]);
            for (int x = 0; s < S; ++s, ++x) a4[x] = fma(y[s], es[s * rank + j], a4[x]);
            const double acc = ((a4[0] + a4[1]) + a4[2]) + a4[3];
            T[row * rank + j] = acc;
            const double tp = fmax(acc, 0.0), tn = fmax(-acc, 0.0);
            pos = fma(tp, tp, pos);
            ngt = fma(tn, tn, ngt);
        }
    }
    red[threadIdx.x] = pos;
    red[kSvdThreads + threadIdx.x] = ngt;
    __syncthreads();
    if (g == 0 && comp) {
        double sp = 0.0, sn = 0.0;
        for (int x = 0; x < ng; ++x) {
            sp += red[x * RP + j];
            sn += red[kSvdThreads + x * RP + j];
        }
        slab[((int64_t)blockIdx.x * 2) * rank + j] = sp;
        slab[((int64_t)blockIdx.x * 2 + 1) * rank + j] = sn;
    }
}

// out[e] = the slabs' sum of element e (of `len`), slabs in rising order.  One thread per element.
__global__ __launch_bounds__(256) void k_svd_sum_slabs(const double* __restrict__ slab, int n_slabs, int len,
                                                       double* __restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= len) return;
    double acc = 0.0;
    for (int b = 0; b < n_slabs; ++b) acc += slab[(int64_t)b * len + e];
    out[e] = acc;
}

int svd_project_grid(int64_t N) {
    int64_t want = (N + kSvdProjectRows - 1) / kSvdProjectRows;
    if (want > kSvdMaxGrid) want = kSvdMaxGrid;
    return (int)(want < 1 ? 1 : want);
}

int64_t svd_project_slab_doubles(int64_t N, int rank) { return (int64_t)svd_project_grid(N) * 2 * rank; }

hipError_t launch_svd_project(const ProblemView& p, const double* H1, const double* Es, int rank, double* T, double* slab,
                              double* norms, hipStream_t st) {
    int RP = 1;
    while (RP < rank) RP *= 2;
    const int nbx = svd_project_grid(p.N);
    const size_t lds = svd_project_lds_bytes(p.S, rank);
    const hipError_t e = raise_dynamic_lds<k_svd_project>(lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_svd_project, dim3(nbx), dim3(kSvdThreads), lds, st, p.V, p.Rt, H1, p.n_c, p.N, p.S, Es, rank, RP, T,
                       slab);
    const hipError_t el = hipGetLastError();
    if (el != hipSuccess) return el;
    hipLaunchKernelGGL(k_svd_sum_slabs, dim3((2 * rank + 255) / 256), dim3(256), 0, st, slab, nbx, 2 * rank, norms);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ u0 from T, in place
// init_func.py:50, :64 / :67, :70 and the clip of :31 (deconvolution.py:136): x = c_j |t| (sign 0: component 0) or
// c_j max(s_j t, 0); x < 1e-11 -> 0; clip to [0, 1].  A NaN stays one, as in numpy.
__global__ __launch_bounds__(256) void k_svd_finish(double* __restrict__ T, int64_t n, int rank, SvdColumns cols) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
        const int j = (int)(e % rank);
        const double t = T[e], sg = cols.sign[j];
        double x = cols.scale[j] * (sg == 0.0 ? fabs(t) : fmax(sg * t, 0.0));
        if (x < 1e-11) x = 0.0;
        if (x > 1.0) x = 1.0;
        T[e] = x;
    }
}

hipError_t launch_svd_finish(double* T, int64_t N, int rank, const SvdColumns& cols, hipStream_t st) {
    const int64_t n = N * rank;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_svd_finish, dim3((int)blocks), dim3(256), 0, st, T, n, rank, cols);
    return hipGetLastError();
}

}  // namespace dmf
