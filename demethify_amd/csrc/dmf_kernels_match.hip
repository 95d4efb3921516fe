// Component matching for the bootstrap: which unknown type of a replicate is which unknown type of the anchor solve.
//
// k_match_gram: P[a][b] = sum_j u[j][a] anchor[idx[j]][b], a, b < n_u -- the inner products of the replicate's profile
// columns with the anchor's, the anchor's rows taken where the replicate's rows were drawn.  u is a solver's iterate
// (N x n_u, in HBM), anchor n_anchor_rows x n_u, idx the replicate's int64 row draw (null: the identity).  One pass over u
// and the gathered anchor rows: N (16 n_u + 8) bytes and N n_u^2 FMAs, plain vector FP64.
// k_copy_cols_permuted: dst[i][b] = u[i][src_col[b]], the device-to-device copy of the profiles with the columns renamed.
// k_first_fill / k_first_occurrence / k_copy_rows_first: the same copy with the rows put back by CpG (end of this file).
//
// Budget.  k_match_gram, 256 threads, at most one workgroup per CU (kMatchMaxGrid).  LDS, static: a tile of R = 2048 / n_u
// rows of u (a contiguous chunk of at most 2048 doubles), the same rows of the anchor (gathered, n_u contiguous doubles
// each) and the tile's R row indices: 48 KB.  A thread owns (pair, row group): with NP = n_u^2 pairs, PS = NP rounded up to
// a power of two (256 at most) and NG = 256 / PS row groups, thread t adds rows g, g + NG, ... of the tile for pair
// p = t % PS (g = t / PS); beyond 256 pairs (n_u > 16) NG = 1 and a thread owns the NACC pairs t, t + 256, ...: 4 accumulators up
// to n_u = 32, 16 up to n_u = 64.
//
// Every sum has a fixed order: a thread walks its rows in rising order over the workgroup's tiles in rising order, the row
// groups are added in rising order, the workgroup writes its share to a slab of its own, and the slabs are added in rising
// order (launch_sum_slabs).  Grid and tile depend on (N, n_u) alone, so does the result.  No atomics on doubles; no
// workgroup waits for another.
//
// An index outside [0, n_anchor_rows) is never dereferenced: its row contributes zeros and is counted in the workgroup's
// integer flag, for the caller to refuse the result.
#include "dmf_dispatch.h"
#include "dmf_internal.h"

namespace dmf {

constexpr int kMatchThreads = 256;
constexpr int kMatchTileDoubles = 2048;  // doubles of u (and of the anchor) per tile
constexpr int kMatchMaxGrid = 256;       // workgroups at most (one per CU)

__host__ __device__ inline int match_tile_rows(int n_u) { return kMatchTileDoubles / n_u; }

template <int NACC>
__global__ __launch_bounds__(kMatchThreads) void k_match_gram(const double* __restrict__ u, const double* __restrict__ anchor,
                                                              const long long* __restrict__ idx, int64_t N,
                                                              int64_t n_anchor_rows, int n_u, int PS,
                                                              double* __restrict__ slab, int* __restrict__ flags) {
    __shared__ double ut[kMatchTileDoubles];
    __shared__ double at[kMatchTileDoubles];
    __shared__ long long ix[kMatchTileDoubles];
    __shared__ int n_bad;
    const int NP = n_u * n_u, R = match_tile_rows(n_u), NG = kMatchThreads / PS;
    const int t = threadIdx.x, p0 = t & (PS - 1), g = t / PS;
    int pa[NACC], pb[NACC];
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        const int p = p0 + k * kMatchThreads;  // (NACC > 1: PS = 256)
        const int q = p < NP ? p : 0;
        pa[k] = q / n_u;
        pb[k] = q - pa[k] * n_u;
        acc[k] = 0.0;
    }
    if (t == 0) n_bad = 0;
    int bad = 0;
    const int64_t n_tiles = (N + R - 1) / R;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = tile * R;
        const int rows = (int)(N - row0 < R ? N - row0 : R);
        __syncthreads();  // (the previous tile has been read)
        for (int r = t; r < rows; r += kMatchThreads) {
            long long v = idx != nullptr ? idx[row0 + r] : (long long)(row0 + r);
            if (v < 0 || v >= n_anchor_rows) {
                v = -1;
                ++bad;
            }
            ix[r] = v;
        }
        const double* __restrict__ src = u + row0 * n_u;
        for (int e = t; e < rows * n_u; e += kMatchThreads) ut[e] = src[e];
        __syncthreads();
        for (int e = t; e < rows * n_u; e += kMatchThreads) {
            const int r = e / n_u, c = e - r * n_u;
            const long long v = ix[r];
            at[e] = v >= 0 ? anchor[v * n_u + c] : 0.0;
        }
        __syncthreads();
        for (int r = g; r < rows; r += NG) {
            const double* __restrict__ ur = ut + r * n_u;
            const double* __restrict__ ar = at + r * n_u;
#pragma unroll
            for (int k = 0; k < NACC; ++k) acc[k] = fma(ur[pa[k]], ar[pb[k]], acc[k]);
        }
    }
    __syncthreads();
    if (bad) atomicAdd(&n_bad, bad);
    double* __restrict__ out = slab + (int64_t)blockIdx.x * NP;
    if constexpr (NACC == 1) {
        ut[t] = acc[0];
        __syncthreads();
        if (g == 0 && p0 < NP) {
            double sum = 0.0;
            for (int x = 0; x < NG; ++x) sum += ut[x * PS + p0];
            out[p0] = sum;
        }
    } else {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NACC; ++k) {
            const int p = p0 + k * kMatchThreads;
            if (p < NP) out[p] = acc[k];
        }
    }
    if (t == 0) flags[blockIdx.x] = n_bad;
}

// out[e] = the slabs' sum of element e (of `len`), slabs in rising order.  One thread per element.
__global__ __launch_bounds__(256) void k_match_sum_slabs(const double* __restrict__ slab, int n_slabs, int len,
                                                         double* __restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= len) return;
    double acc = 0.0;
    for (int b = 0; b < n_slabs; ++b) acc += slab[(int64_t)b * len + e];
    out[e] = acc;
}

int match_gram_grid(int64_t N, int n_u) {
    const int R = match_tile_rows(n_u);
    int64_t want = (N + R - 1) / R;
    if (want > kMatchMaxGrid) want = kMatchMaxGrid;
    return (int)(want < 1 ? 1 : want);
}

int64_t match_gram_slab_doubles(int64_t N, int n_u) { return (int64_t)match_gram_grid(N, n_u) * n_u * n_u; }

hipError_t launch_match_gram(const double* u, const double* anchor, const long long* idx, int64_t N, int64_t n_anchor_rows,
                             int n_u, double* slab, int* flags, double* P, hipStream_t st) {
    if (n_u < 1 || n_u > kMaxK || N < 1) return hipErrorInvalidValue;
    const int NP = n_u * n_u, grid = match_gram_grid(N, n_u);
    int PS = 1;
    while (PS < NP && PS < kMatchThreads) PS *= 2;
    const int nacc = NP <= kMatchThreads ? 1 : NP <= 4 * kMatchThreads ? 4 : 16;
    auto launch = [&](auto n) {
        constexpr int NACC = decltype(n)::value;
        hipLaunchKernelGGL((k_match_gram<NACC>), dim3(grid), dim3(kMatchThreads), 0, st, u, anchor, idx, N, n_anchor_rows, n_u,
                           PS, slab, flags);
        return hipGetLastError();
    };
    const hipError_t e = nacc == 1   ? launch(std::integral_constant<int, 1>{})
                         : nacc == 4 ? launch(std::integral_constant<int, 4>{})
                                     : launch(std::integral_constant<int, 16>{});
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_match_sum_slabs, dim3((NP + 255) / 256), dim3(256), 0, st, slab, grid, NP, P);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ dst = u[:, src_col]
__global__ __launch_bounds__(256) void k_copy_cols_permuted(const double* __restrict__ u, double* __restrict__ dst, int64_t n,
                                                            int n_u, MatchColumns cols) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
        const int64_t i = e / n_u;
        const int b = (int)(e - i * n_u);
        dst[e] = u[i * n_u + cols.src[b]];
    }
}

hipError_t launch_copy_cols_permuted(const double* u, double* dst, int64_t N, int n_u, const MatchColumns& cols,
                                     hipStream_t st) {
    if (n_u < 1 || n_u > kMaxK || N < 1) return hipErrorInvalidValue;
    const int64_t n = N * n_u;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_copy_cols_permuted, dim3((int)blocks), dim3(256), 0, st, u, dst, n, n_u, cols);
    return hipGetLastError();
}

// --------------------------------------------------------------------------- dst[c] = u[first position that drew CpG c]
// A replicate's rows by CpG: row j of u belongs to CpG idx[j]; CpG c takes the row of its lowest position, a pure gather.
// k_first_fill marks every CpG "not drawn" and clears the counter; k_first_occurrence lowers first[idx[j]] to j with an
// integer atomic minimum, whose result does not depend on the order the positions arrive in; k_copy_rows_first moves the
// rows, one thread per destination element (coalesced stores, n_u contiguous doubles per gathered row), NaN where the CpG
// was not drawn.  No floating-point arithmetic: a copied value keeps its bits.
__global__ __launch_bounds__(256) void k_first_fill(long long* __restrict__ first, int64_t n, unsigned long long* n_bad) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < n; c += stride) first[c] = kNotDrawn;
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_bad = 0;
}

__global__ __launch_bounds__(256) void k_first_occurrence(const long long* __restrict__ idx, int64_t M, int64_t n_dst_rows,
                                                          long long* first, unsigned long long* n_bad) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    unsigned long long bad = 0;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < M; j += stride) {
        const long long c = idx[j];
        if (c < 0 || c >= n_dst_rows) ++bad;
        else atomicMin(&first[c], (long long)j);
    }
    if (bad) atomicAdd(n_bad, bad);
}

__global__ __launch_bounds__(256) void k_copy_rows_first(const double* __restrict__ u, const long long* __restrict__ first,
                                                         double* __restrict__ dst, int64_t n, int n_u, MatchColumns cols) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
        const int64_t c = e / n_u;
        const int b = (int)(e - c * n_u);
        const long long j = first[c];
        dst[e] = j == kNotDrawn ? __longlong_as_double(0x7ff8000000000000LL) : u[j * n_u + cols.src[b]];
    }
}

static int copy_blocks(int64_t n) {
    const int64_t blocks = (n + 255) / 256;
    return (int)(blocks > 4096 ? 4096 : blocks);
}

hipError_t launch_first_occurrence(const long long* idx, int64_t M, int64_t n_dst_rows, long long* first,
                                   unsigned long long* n_bad, hipStream_t st) {
    if (M < 1 || n_dst_rows < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_first_fill, dim3(copy_blocks(n_dst_rows)), dim3(256), 0, st, first, n_dst_rows, n_bad);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_first_occurrence, dim3(copy_blocks(M)), dim3(256), 0, st, idx, M, n_dst_rows, first, n_bad);
    return hipGetLastError();
}

hipError_t launch_copy_rows_first(const double* u, const long long* first, double* dst, int64_t n_dst_rows, int n_u,
                                  const MatchColumns& cols, hipStream_t st) {
    if (n_u < 1 || n_u > kMaxK || n_dst_rows < 1) return hipErrorInvalidValue;
    const int64_t n = n_dst_rows * n_u;
    hipLaunchKernelGGL(k_copy_rows_first, dim3(copy_blocks(n)), dim3(256), 0, st, u, first, dst, n, n_u, cols);
    return hipGetLastError();
}

}  // namespace dmf
