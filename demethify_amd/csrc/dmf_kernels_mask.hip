// Hold-out masks (dmf_problem_mask): a resident problem with the held-out elements' counts set to zero, derived where the
// data lives -- what bi-cross-validation (ic.py:58-89: `counts * train_mask`) builds per fold, and what a caller with
// missing entries needs.
//
// The mask is bit-packed row-major, ceil(S / 8) bytes per row, sample s = bit (s & 7) of byte (s >> 3), 1 = kept.  One wave
// per destination row: per 512 samples lane l loads ONE mask byte, that of samples 8 l .. 8 l + 7 -- exactly the eight u16
// elements of its 16-byte piece of the D16 / X16 rows, so the byte expands to the lane's store masks in registers; the f64
// rows of V and D go through the same pass with lane-consecutive (coalesced) elements, each lane fetching its bit from the
// lane that holds the byte (one __shfl per 64 elements).  No element reads a mask bit from memory on its own.
#include <cstdint>

#include "dmf_internal.h"

namespace dmf {

typedef unsigned int v4u __attribute__((ext_vector_type(4)));

namespace {

// kept / held-out bits of the eight samples c .. c + 7 of row `row` (c a multiple of 8); bits of samples >= S are neither
__device__ __forceinline__ void mask_byte(const unsigned char* __restrict__ bits, int64_t row, int nb, int S, int c,
                                          unsigned int* keep, unsigned int* hold) {
    unsigned int valid = 0u, b = 0u;
    if (c < S) {
        valid = S - c >= 8 ? 0xFFu : (1u << (S - c)) - 1u;
        b = bits[row * nb + (c >> 3)];
    }
    *keep = b & valid;
    *hold = ~b & valid;
}

// the two u16 elements 2 e, 2 e + 1 of a lane's eight: all-ones halves where the bit is set
__device__ __forceinline__ unsigned int pair_mask(unsigned int m, int e) {
    return (((m >> (2 * e)) & 1u) ? 0x0000FFFFu : 0u) | (((m >> (2 * e + 1)) & 1u) ? 0xFFFF0000u : 0u);
}

}  // namespace

// dst = src where kept, 0 where held out, for V and D (f64, [N][S]) and -- src16 != null -- D16 and X16 (u16, [N16][SD], rows
// >= N and samples >= S zero); W16 (D16's layout) <- 1 where held out, 0 elsewhere.  stats[3] (zeroed by the launcher) <-
// { bits of the largest kept count as a non-negative double, sum of the kept x, number of held-out elements }: one atomic
// per workgroup and statistic (see k_gather_rows_u16 for why).
__global__ __launch_bounds__(256) void k_mask_rows(const double* __restrict__ srcV, const double* __restrict__ srcD,
                                                   const unsigned short* __restrict__ src16,
                                                   const unsigned short* __restrict__ srcX,
                                                   const unsigned char* __restrict__ bits, double* __restrict__ dstV,
                                                   double* __restrict__ dstD, unsigned short* __restrict__ dst16,
                                                   unsigned short* __restrict__ dstX, unsigned short* __restrict__ W16,
                                                   int64_t N, int64_t n_rows, int S, int SD, int nb,
                                                   unsigned long long* __restrict__ stats) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double dmax = 0.0;
    unsigned long long xs = 0, nt = 0;
    const int width = src16 != nullptr ? SD : (S + 7) / 8 * 8;  // samples a row's chunks cover
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n_rows; r += (int64_t)gridDim.x * 4) {
        const bool live = r < N;  // (wave-uniform; rows N .. N16 of the u16 copies are zero)
        for (int cb = 0; cb < width; cb += 512) {
            const int c = cb + lane * 8;
            unsigned int keep = 0u, hold = 0u;
            if (live) mask_byte(bits, r, nb, S, c, &keep, &hold);
            nt += __popc(hold);
            if (src16 != nullptr && c < SD) {
                v4u d = v4u{0u, 0u, 0u, 0u}, x = d, w = d;
                if (live) {
                    d = *reinterpret_cast<const v4u*>(src16 + r * SD + c);
                    if (srcX != nullptr) x = *reinterpret_cast<const v4u*>(srcX + r * SD + c);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const unsigned int m = pair_mask(keep, e);
                        d[e] &= m;
                        x[e] &= m;
                        xs += (x[e] & 0xFFFFu) + (x[e] >> 16);
                        w[e] = ((hold >> (2 * e)) & 1u) | (((hold >> (2 * e + 1)) & 1u) << 16);
                    }
                }
                *reinterpret_cast<v4u*>(dst16 + r * SD + c) = d;
                if (dstX != nullptr) *reinterpret_cast<v4u*>(dstX + r * SD + c) = x;
                *reinterpret_cast<v4u*>(W16 + r * SD + c) = w;
            }
            if (live) {  // the f64 rows: element cb + 64 j + lane, its bit in the byte of lane 8 j + (lane >> 3)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const unsigned int kb = (unsigned int)__shfl((int)keep, 8 * j + (lane >> 3), 64);
                    const int col = cb + 64 * j + lane;
                    if (col < S) {
                        const bool k = (kb >> (lane & 7)) & 1u;
                        const int64_t at = r * S + col;
                        const double d = k ? srcD[at] : 0.0;
                        dstD[at] = d;
                        dstV[at] = k ? srcV[at] : 0.0;
                        dmax = fmax(dmax, d);
                    }
                }
            }
        }
    }
    unsigned long long mx = (unsigned long long)__double_as_longlong(dmax);  // (non-negative doubles order as their bits)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(mx, off, 64);
        mx = mx > o ? mx : o;
        xs += __shfl_xor(xs, off, 64);
        nt += __shfl_xor(nt, off, 64);
    }
    __shared__ unsigned long long wst[4][3];
    if (lane == 0) wst[wave][0] = mx, wst[wave][1] = xs, wst[wave][2] = nt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = wst[0][0], x = wst[0][1], n = wst[0][2];
        for (int w = 1; w < 4; ++w) m = m > wst[w][0] ? m : wst[w][0], x += wst[w][1], n += wst[w][2];
        if (m > 0) atomicMax(stats, m);
        if (x > 0) atomicAdd(stats + 1, x);
        if (n > 0) atomicAdd(stats + 2, n);
    }
}

// W[N][S] (f64) <- 1 where held out, 0 where kept: the weights of the hold-out error for the shapes whose cost kernel reads
// f64 counts (k_cost)
__global__ __launch_bounds__(256) void k_holdout_weights_f64(const unsigned char* __restrict__ bits, double* __restrict__ W,
                                                             int64_t N, int S, int nb) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int width = (S + 7) / 8 * 8;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < N; r += (int64_t)gridDim.x * 4) {
        for (int cb = 0; cb < width; cb += 512) {
            unsigned int keep = 0u, hold = 0u;
            mask_byte(bits, r, nb, S, cb + lane * 8, &keep, &hold);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned int hb = (unsigned int)__shfl((int)hold, 8 * j + (lane >> 3), 64);
                const int col = cb + 64 * j + lane;
                if (col < S) W[r * S + col] = ((hb >> (lane & 7)) & 1u) ? 1.0 : 0.0;
            }
        }
    }
}

hipError_t launch_mask_problem(const double* srcV, const double* srcD, const unsigned short* src16,
                               const unsigned short* srcX, const unsigned char* bits, double* dstV, double* dstD,
                               unsigned short* dst16, unsigned short* dstX, unsigned short* W16, int64_t N, int64_t N16, int S,
                               int SD, unsigned long long* stats, hipStream_t st) {
    if (bits == nullptr || srcV == nullptr || srcD == nullptr || dstV == nullptr || dstD == nullptr || stats == nullptr)
        return hipErrorInvalidValue;
    if (src16 != nullptr && (dst16 == nullptr || W16 == nullptr || SD < S || SD % 8 != 0 || N16 < N)) return hipErrorInvalidValue;
    if (src16 == nullptr && (dst16 != nullptr || srcX != nullptr || dstX != nullptr)) return hipErrorInvalidValue;
    if ((srcX == nullptr) != (dstX == nullptr)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(stats, 0, 3 * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    const int64_t n_rows = src16 != nullptr ? N16 : N;
    int64_t g = (n_rows + 3) / 4;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    hipLaunchKernelGGL(k_mask_rows, dim3((unsigned)g), dim3(256), 0, st, srcV, srcD, src16, srcX, bits, dstV, dstD, dst16, dstX,
                       W16, N, n_rows, S, SD, (S + 7) / 8, stats);
    return hipGetLastError();
}

hipError_t launch_holdout_weights_f64(const unsigned char* bits, double* W, int64_t N, int S, hipStream_t st) {
    int64_t g = (N + 3) / 4;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    hipLaunchKernelGGL(k_holdout_weights_f64, dim3((unsigned)g), dim3(256), 0, st, bits, W, N, S, (S + 7) / 8);
    return hipGetLastError();
}

}  // namespace dmf
