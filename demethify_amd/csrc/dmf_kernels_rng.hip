// Hold-out mask draw (dmf_mask_draw): `np.random.rand(N, S) < fraction` of numpy's legacy global generator (ic.py:68), bit for
// bit, written straight into the packed form dmf_problem_mask reads -- so that a bi-cross-validation fold's mask never
// exists on the host.
//
// The generator is MT19937.  One regeneration of its 624-word key is three groups of mutually independent words
//     tw(a, b) = (y >> 1) ^ (y & 1 ? 0x9908b0df : 0),  y = (a & 0x80000000) | (b & 0x7fffffff)
//     i in [0, 227):    new[i] = old[i + 397] ^ tw(old[i], old[i + 1])
//     i in [227, 454):  new[i] = new[i - 227] ^ tw(old[i], old[i + 1])
//     i in [454, 623):  new[i] = new[i - 227] ^ tw(old[i], old[i + 1]);  new[623] = new[396] ^ tw(old[623], new[0])
// which is as far as the recurrence itself parallelises.  Beyond that the stream is cut into segments whose starting keys
// come from the caller's by polynomial jump-ahead (k_mt_jump, dmf_mt_jump.hip), one workgroup per segment
// (k_mask_draw_segments); a draw of one segment is k_mask_draw.  Either way a workgroup of 256 threads walks its stream, the
// key ping-ponging between two LDS arrays (old is read while new is written), a barrier after each group.  random_sample
// makes a double from two consecutive tempered words, k / 2^53 with k = (a >> 5) 2^26 + (b >> 6), so `x < fraction` is the
// integer compare k < T with the host's T = ceil(fraction 2^53): no floating point here.
//
// A "stretch" is the part of the stream one key serves: stretch 0 the key as given from position p (or, for position 624,
// its first regeneration), every later one 624 words = 312 doubles.  With p odd a double straddles two stretches: its `a`
// is word 623 of the previous key, still intact in the other LDS array.  Element j of the row-major N x S matrix is double
// j of the stream; thread by thread the compare bits of a stretch are gathered per wave (__ballot) into a ring of 2048
// bits indexed by j mod 2048, in 64-bit slots aligned in j -- the one slot a stretch shares with its predecessor is
// merged by the lane that writes it.  A byte of the output holds at most 8 consecutive j (sample s = bit (s & 7) of byte
// (s >> 3), ceil(S / 8) bytes per row, padding bits zero), so the bytes that a stretch completes are cut out of the ring and
// stored by consecutive lanes; a byte that a stretch leaves partly filled waits in the ring for the next.  The emission of
// stretch t runs between the first two barriers of regeneration t + 1, which saves it a barrier of its own.
#include <cstdint>

#include "dmf_batch.h"
#include "dmf_internal.h"
#include "dmf_mt_jump.h"

namespace dmf {

namespace {

constexpr int kMtN = 624, kMtM = 397, kRingSlots = 32;  // (ring: 32 x 64 bits >= 7 waiting + 313 new + 63 of alignment)

__device__ __forceinline__ unsigned int mt_twist(unsigned int a, unsigned int b) {
    const unsigned int y = (a & 0x80000000u) | (b & 0x7fffffffu);
    return (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

__device__ __forceinline__ unsigned int mt_temper(unsigned int y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// What has been emitted so far (uniform over the workgroup): the next byte is byte `col` of row `row`.
struct Emitted {
    unsigned long long row = 0;
    unsigned int col = 0;
};

// Stores every byte that lies wholly below element (row_c, s_c) -- the first element not drawn yet -- and is not out yet.
__device__ __forceinline__ void emit_bytes(const unsigned long long* ring, unsigned char* __restrict__ bits,
                                           unsigned long long S, unsigned int nb, unsigned long long row_c,
                                           unsigned int s_c, Emitted& done, unsigned long long& kept) {
    const unsigned int count = (unsigned int)((row_c - done.row) * nb) + (s_c >> 3) - done.col;  // (<= 320)
    for (unsigned int i = threadIdx.x; i < count; i += blockDim.x) {
        // byte done.col + i counted on from row done.row: a handful of rows at most where a row has 8 bytes or more (a
        // stretch completes 39 + 312 / S bytes), so no division there
        unsigned int cb = done.col + i, up = 0;
        if (nb >= 8) {
            while (cb >= nb) cb -= nb, ++up;
        } else {
            up = cb / nb;
            cb -= up * nb;
        }
        const unsigned long long r = done.row + up;
        const unsigned long long j0 = r * S + 8ull * cb, left = S - 8ull * cb;
        const unsigned int n = left >= 8 ? 8u : (unsigned int)left;
        const unsigned int at = (unsigned int)j0 & (64 * kRingSlots - 1), slot = at >> 6, sh = at & 63;
        unsigned long long v = ring[slot] >> sh;
        if (sh > 56) v |= ring[(slot + 1) & (kRingSlots - 1)] << (64 - sh);
        const unsigned int b = (unsigned int)v & ((1u << n) - 1u);
        bits[r * nb + cb] = (unsigned char)b;
        kept += __popc(b);
    }
    done.row = row_c, done.col = s_c >> 3;
}

// The first element at or behind double j that begins a byte, as (row, sample): (N, 0) from N S on.
__device__ __forceinline__ void byte_start(unsigned long long j, unsigned long long N, unsigned long long S,
                                           unsigned long long& row, unsigned int& s) {
    if (j >= N * S) {
        row = N, s = 0;
        return;
    }
    row = j / S;
    unsigned long long r = (j - row * S + 7) & ~7ull;
    if (r >= S) ++row, r = 0;
    s = (unsigned int)r;
}

// The stretch loop of one workgroup of 256 threads over the blocks t_first..t_last of the stream (block t = the words
// [624 t, 624 t + 624), the stream's word p the first that makes a double).  key[0] holds the key of block t_first, or with
// regen_first the key before it; ring is zero.  Drawn and stored are the doubles from element (row_c, s_c) up to j_end, a
// range that begins and ends where a byte does (or is empty).  Returns the LDS array that holds the key of block t_last;
// kept: this thread's share of the ones.
__device__ __forceinline__ int draw_stretches(unsigned int (*key)[kMtN], unsigned long long* ring, int p, bool regen_first,
                                              unsigned long long t_first, unsigned long long t_last,
                                              unsigned long long row_c, unsigned int s_c, unsigned long long j_end,
                                              unsigned long long S, unsigned long long T,
                                              unsigned char* __restrict__ bits, unsigned long long& kept) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned int nb = (unsigned int)((S + 7) / 8);
    int cur = 0;  // the LDS array that holds the key of the stretch in hand
    // (row_c, s_c): the first element not drawn yet
    unsigned long long jb = row_c * S + s_c;
    Emitted done;
    done.row = row_c, done.col = s_c >> 3;
    for (unsigned long long t = t_first; t <= t_last; ++t) {
        if (t > t_first || regen_first) {
            const unsigned int* __restrict__ o = key[cur];
            unsigned int* __restrict__ n = key[cur ^ 1];
            if (tid < 227) n[tid] = o[tid + kMtM] ^ mt_twist(o[tid], o[tid + 1]);
            __syncthreads();
            // (the bits of the stretch before are in the ring since the barrier above; the next to write it is this
            // stretch's compare, behind two more barriers)
            emit_bytes(ring, bits, S, nb, row_c, s_c, done, kept);
            if (tid < 227) n[tid + 227] = n[tid] ^ mt_twist(o[tid + 227], o[tid + 228]);
            __syncthreads();
            if (tid < 169) n[tid + 454] = n[tid + 227] ^ mt_twist(o[tid + 454], o[tid + 455]);
            if (tid == 169) n[623] = n[396] ^ mt_twist(o[623], n[0]);
            __syncthreads();
            cur ^= 1;
        }
        // the doubles this stretch completes: [ja, jb_new), double j from the words p + 2 j and p + 2 j + 1 of the stream
        const unsigned long long first = t * kMtN, ja = jb;
        unsigned long long jb_new = ((t + 1) * kMtN - (unsigned long long)p) / 2;
        jb_new = jb_new < j_end ? jb_new : j_end;
        jb_new = jb_new > ja ? jb_new : ja;  // (a range that begins behind this stretch)
        const int rel0 = (int)((long long)((unsigned long long)p + 2 * ja) - (long long)first);  // `a` of double ja: -1 = straddles
        const unsigned long long base = ja & ~63ull;
        const unsigned int* __restrict__ k_cur = key[cur];
        const unsigned int* __restrict__ k_prev = key[cur ^ 1];
        for (int pass = 0; pass < 2; ++pass) {
            const unsigned long long chunk = base + 64ull * (pass * 4 + wave);  // (wave-uniform)
            if (chunk >= jb_new) continue;
            const unsigned long long j = chunk + lane;
            bool bit = false;
            if (j >= ja && j < jb_new) {
                const int rel = rel0 + 2 * (int)(j - ja);
                const unsigned int wa = rel >= 0 ? k_cur[rel] : k_prev[kMtN - 1];
                const unsigned long long a = mt_temper(wa) >> 5, b = mt_temper(k_cur[rel + 1]) >> 6;
                bit = ((a << 26) + b) < T;
            }
            const unsigned long long votes = __ballot(bit);
            if (lane == 0) {
                const unsigned int slot = (unsigned int)(chunk >> 6) & (kRingSlots - 1);
                ring[slot] = (chunk < ja ? ring[slot] : 0ull) | votes;  // (bits below ja: the stretch before wrote them)
            }
        }
        // advance (row_c, s_c) by the doubles drawn: at most 313, i.e. five rows from 64 samples on; a 32-bit division below
        unsigned long long s_new = s_c + (jb_new - ja);
        if (S >= 64) {
            while (s_new >= S) s_new -= S, ++row_c;
        } else {
            const unsigned int q = (unsigned int)s_new / (unsigned int)S;
            row_c += q;
            s_new -= (unsigned long long)q * S;
        }
        s_c = (unsigned int)s_new;
        jb = jb_new;
    }
    __syncthreads();
    emit_bytes(ring, bits, S, nb, row_c, s_c, done, kept);  // (jb = j_end: every byte of the range is out)
    return cur;
}

// The workgroup's ones, summed wave by wave in a fixed order; the value is thread 0's.
__device__ __forceinline__ unsigned long long sum_kept(unsigned long long kept, unsigned long long* wave_kept) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) kept += __shfl_xor(kept, off, 64);
    if (lane == 0) wave_kept[wave] = kept;
    __syncthreads();
    return wave_kept[0] + wave_kept[1] + wave_kept[2] + wave_kept[3];
}

}  // namespace

// key_io[624]: the generator's key, in and out (the key as of the last regeneration); p = position % 624 of the first word
// to use, regen_first: the position was 624.  bits <- the packed N x S mask (every byte written), result[0] <- number of
// ones, result[1] <- the position after the last word used (1..624).  Launched as ONE workgroup of 256 threads.
__global__ __launch_bounds__(256) void k_mask_draw(unsigned int* __restrict__ key_io, int p, int regen_first,
                                                   unsigned long long N, unsigned long long S, unsigned long long T,
                                                   unsigned char* __restrict__ bits,
                                                   unsigned long long* __restrict__ result) {
    __shared__ unsigned int key[2][kMtN];
    __shared__ unsigned long long ring[kRingSlots];
    __shared__ unsigned long long wave_kept[4];
    const int tid = threadIdx.x;
    const unsigned long long M = N * S, last_word = (unsigned long long)p + 2 * M - 1, t_last = last_word / kMtN;
    for (int i = tid; i < kMtN; i += 256) key[0][i] = key_io[i];
    if (tid < kRingSlots) ring[tid] = 0;
    __syncthreads();

    unsigned long long kept = 0;
    const int cur = draw_stretches(key, ring, p, regen_first != 0, 0, t_last, 0, 0, M, S, T, bits, kept);

    for (int i = tid; i < kMtN; i += 256) key_io[i] = key[cur][i];
    const unsigned long long ones = sum_kept(kept, wave_kept);
    if (tid == 0) {
        result[0] = ones;
        result[1] = last_word % kMtN + 1;
    }
}

// The same draw cut into segments of c blocks on numpy's own 624-word grid, one workgroup of 256 threads per segment: block
// 0 is the caller's key (used from word p = the position, 0..624), segment s the blocks [c s, c s + c).  keys[s][624]: for
// s = 0 the caller's key, for s >= 1 the key of block c s - 1 -- the block BEFORE the segment, which the workgroup
// regenerates once: with p odd the first double of a segment has its `a` in word 623 of that block.  A double belongs to
// the block of its second word, and a byte to the segment that holds its first element: the workgroup skips the leading
// doubles of a byte begun before its segment and draws the (at most 7) doubles behind its segment that finish its last
// byte, so every byte is stored by exactly one workgroup.  counts[s] <- the ones of the bytes it stored; the workgroup whose
// segment holds the last word used hands back key_out[624] (the key of that block) and result[1] (the position behind that
// word, 1..624).  The grid is last block / c + 1 workgroups.
__global__ __launch_bounds__(256) void k_mask_draw_segments(const unsigned int* __restrict__ keys,
                                                            unsigned int* __restrict__ key_out, int p,
                                                            unsigned long long c, unsigned long long N,
                                                            unsigned long long S, unsigned long long T,
                                                            unsigned char* __restrict__ bits,
                                                            unsigned long long* __restrict__ result,
                                                            unsigned long long* __restrict__ counts) {
    __shared__ unsigned int key[2][kMtN];
    __shared__ unsigned long long ring[kRingSlots];
    __shared__ unsigned long long wave_kept[4];
    const int tid = threadIdx.x;
    const unsigned long long seg = blockIdx.x;
    const unsigned long long M = N * S, last_word = (unsigned long long)p + 2 * M - 1, t_end = last_word / kMtN;
    const unsigned long long t0 = c * seg, t1 = c * (seg + 1) < t_end + 1 ? c * (seg + 1) : t_end + 1;
    // the doubles the segment's blocks complete, [j0, j1), and the bytes that begin among them, [j_first, j_end)
    unsigned long long j0 = seg == 0 ? 0 : (t0 * kMtN - (unsigned long long)p) / 2, j1 = (t1 * kMtN - (unsigned long long)p) / 2;
    j0 = j0 < M ? j0 : M, j1 = j1 < M ? j1 : M;
    unsigned long long row_first, row_end;
    unsigned int s_first, s_end;
    byte_start(j0, N, S, row_first, s_first);
    byte_start(j1, N, S, row_end, s_end);
    const unsigned long long j_first = row_first * S + s_first, j_end = row_end * S + s_end;
    unsigned long long t_last = t1 - 1;  // the last block to regenerate: the segment's, or the one that finishes its last byte
    if (j_end > j_first) {
        const unsigned long long t_byte = ((unsigned long long)p + 2 * j_end - 1) / kMtN;
        t_last = t_byte > t_last ? t_byte : t_last;
    }
    const unsigned int* __restrict__ mine = keys + seg * kMtN;
    for (int i = tid; i < kMtN; i += 256) key[0][i] = mine[i];
    if (tid < kRingSlots) ring[tid] = 0;
    __syncthreads();

    unsigned long long kept = 0;
    const int cur = draw_stretches(key, ring, p, seg > 0, t0, t_last, row_first, s_first, j_end, S, T, bits, kept);

    const bool holds_last = t_end >= t0 && t_end < t1;  // (then j_end = N S and t_last = t_end)
    if (holds_last)
        for (int i = tid; i < kMtN; i += 256) key_out[i] = key[cur][i];
    const unsigned long long ones = sum_kept(kept, wave_kept);
    if (tid == 0) {
        counts[seg] = ones;
        if (holds_last) result[1] = last_word % kMtN + 1;
    }
}

// One workgroup of 640 threads per job: row job.dst of keys[..][624] <- row job.src carried forward by the polynomial whose
// non-zero terms are terms[job.first .. job.first + job.n_terms) (ascending exponents <= 19937; dmf_mt_jump.hip).  No job of a
// launch reads a row that a job of the same launch writes.  The raw sequence that follows the source key -- 32 regenerations
// by the three-group scheme above, each written behind the block it reads -- is laid out in (dynamic) LDS, x[0 .. 33 * 624);
// result word m is the XOR of x[i + m] over the terms i: one thread per word, the term list read by all of them alike, no
// barrier between terms.
__global__ __launch_bounds__(640) void k_mt_jump(unsigned int* keys, const MtJumpJob* __restrict__ jobs,
                                                 const unsigned short* __restrict__ all_terms) {
    extern __shared__ unsigned int x[];
    const int tid = threadIdx.x;
    const MtJumpJob job = jobs[blockIdx.x];
    const unsigned short* __restrict__ terms = all_terms + job.first;
    const int n_terms = job.n_terms;
    const unsigned int* k = keys + (size_t)job.src * kMtN;
    if (tid < kMtN) x[tid] = k[tid];
    __syncthreads();
    for (int b = 0; b + 1 < kMtJumpBlocks; ++b) {
        const unsigned int* o = x + b * kMtN;
        unsigned int* n = x + (b + 1) * kMtN;
        if (tid < 227) n[tid] = o[tid + kMtM] ^ mt_twist(o[tid], o[tid + 1]);
        __syncthreads();
        if (tid < 227) n[tid + 227] = n[tid] ^ mt_twist(o[tid + 227], o[tid + 228]);
        __syncthreads();
        if (tid < 169) n[tid + 454] = n[tid + 227] ^ mt_twist(o[tid + 454], o[tid + 455]);
        if (tid == 169) n[623] = n[396] ^ mt_twist(o[623], n[0]);
        __syncthreads();
    }
    if (tid < kMtN) {
        unsigned int acc = 0;
        int i = 0;
        for (; i + 8 <= n_terms; i += 8) {
            unsigned int v = 0;
#pragma unroll
            for (int u = 0; u < 8; ++u) v ^= x[(int)terms[i + u] + tid];  // (<= 19937 + 623 < 33 * 624)
            acc ^= v;
        }
        for (; i < n_terms; ++i) acc ^= x[(int)terms[i] + tid];
        keys[(size_t)job.dst * kMtN + tid] = acc;
    }
}

hipError_t launch_mask_draw(unsigned int* key_io, int pos, int64_t N, int64_t S, unsigned long long threshold,
                            unsigned char* bits, unsigned long long* result, hipStream_t st) {
    if (key_io == nullptr || bits == nullptr || result == nullptr || pos < 0 || pos > kMtN || N < 1 || S < 1 ||
        S > kMaskDrawMaxS || N > kMaskDrawMaxElements / S)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mask_draw, dim3(1), dim3(256), 0, st, key_io, pos % kMtN, pos == kMtN ? 1 : 0,
                       (unsigned long long)N, (unsigned long long)S, threshold, bits, result);
    return hipGetLastError();
}

hipError_t launch_mask_draw_segments(const unsigned int* keys, unsigned int* key_out, int pos, int64_t c, int64_t N, int64_t S,
                                     unsigned long long threshold, unsigned char* bits, unsigned long long* result,
                                     unsigned long long* counts, hipStream_t st) {
    if (keys == nullptr || key_out == nullptr || bits == nullptr || result == nullptr || counts == nullptr || pos < 0 ||
        pos > kMtN || c < 1 || N < 1 || S < 1 || S > kMaskDrawMaxS || N > kMaskDrawMaxElements / S)
        return hipErrorInvalidValue;
    const unsigned long long t_end = ((unsigned long long)pos + 2ull * (unsigned long long)N * (unsigned long long)S - 1) / kMtN;
    const unsigned long long W = t_end / (unsigned long long)c + 1;
    if (W > (unsigned long long)kMaskDrawMaxSegments) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mask_draw_segments, dim3((unsigned)W), dim3(256), 0, st, keys, key_out, pos, (unsigned long long)c,
                       (unsigned long long)N, (unsigned long long)S, threshold, bits, result, counts);
    return hipGetLastError();
}

hipError_t launch_mt_jump(unsigned int* keys, const MtJumpJob* jobs, int64_t n_jobs, const unsigned short* terms,
                          hipStream_t st) {
    if (keys == nullptr || jobs == nullptr || terms == nullptr || n_jobs < 1 || n_jobs > kMaskDrawMaxSegments)
        return hipErrorInvalidValue;
    static bool raised = false;
    constexpr size_t lds = (size_t)kMtJumpWords * sizeof(unsigned int);  // 82 368 bytes: above the 64 KB a kernel gets unasked
    const hipError_t e = raise_lds_limit(reinterpret_cast<const void*>(&k_mt_jump), lds, &raised);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mt_jump, dim3((unsigned)n_jobs), dim3(640), lds, st, keys, jobs, terms);
    return hipGetLastError();
}

}  // namespace dmf
