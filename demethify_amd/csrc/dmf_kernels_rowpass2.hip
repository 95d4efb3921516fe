// Row pass, second generation: the u phase of one outer iteration (deconvolution.py:81-90 / :157-164) plus the
// part of the alpha phase's right-hand side that needs V (b_u = u^T (D * V)) in ONE read of V (f64) and of the
// counts stored as u16 (D16: exact, 2 bytes per element instead of 8; built once per problem).  The u-dependent
// Gram entries that need no V (cross = Rt^T diag(d) u, uu = u^T diag(d) u) are left to the integer matrix-core
// kernel of dmf_kernels_gram_i8.hip, which reads the counts as 8-bit planes.
//
// Against the first-generation kernel (dmf_kernels_fused.hip) the FP64 work per element drops from 92 to 33 FMA
// (phase C's 58 cross / uu products are gone), which is what that kernel was bound by; a workgroup is one wave per
// 64-sample column group, holds its alpha-derived MFMA operands in registers instead of a 33 KB LDS copy, and needs
// one 16-row tile buffer only, so several workgroups share a CU: while one of them runs the row-local inner iterations
// (one wave, a dependent chain), the others keep the FP64 pipe busy with their contractions.
//
// Per 16-row block, per workgroup (waves = column groups):
//   tile    prefetched global loads (V: 16 B per lane, two rows per instruction; D16: 16 B = 8 counts per lane)
//           -> LDS tile of the wave's own column group (V f64, the counts as the u16 they arrive as)
//           (XS, the problem carries X16: x = d v loaded and stored like the counts, V not read -- see the template)
//   phase A FP64-MFMA contractions on the tile in the row-on-lane layout (as dmf_kernels_rowpass_mfma.hip):
//           E = V - Rt a_known (16x16x4), c = a_unk (D*E)^T (4x4x4, 4 blocks); M = D P^T exactly on the i8 MFMA
//           (16x16x64, counts and P = alpha_j alpha_l as balanced 8-bit digits) -> partial c / M
//   -- barrier X --
//   phase B (one wave, round robin) sums the partials and runs the n_iter2 accelerated projected-gradient steps,
//           lane = (row, unknown); u / u_ go to HBM and u to LDS
//   -- barrier Y --
//   phase C b_u[j][s] += sum_rows u_j (d v) on the 4x4x4 FP64 MFMA, accumulators in registers across all blocks
// Rows beyond N in the last block read a clamped V row and zero counts (D16 is zero-padded to a multiple of 16 rows
// and of 64 columns), so they add nothing; their u is never stored.
//
// Preconditions (checked by the launcher / the solver): 2 <= S <= 256 (odd S: see the tile prefetch), n_c <= 16, n_u <= 4, counts integral and
// <= 32639 (nd = 1: <= 127), alpha within [0, 1] (true of every iterate: columns on the simplex).
#include "dmf_device.h"
#include "dmf_dispatch.h"
#include "dmf_internal.h"
#include "dmf_ustep.h"
#include "dmf_fixedpoint.h"
#include "dmf_rowpass_image.h"
#include <cstdlib>
#include <type_traits>

namespace dmf {

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef unsigned int v2u __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));

// Diagnostic build only (tools/rowpass2_probe.hip defines DMF_STAMPS): per-wave cycle sums of the kernel's segments
// go to a debug buffer of their own; the product build compiles none of it.
#ifdef DMF_STAMPS
#define DMF2_NSTAMP 20  // (16..19: the deferred-C schedule's segments of a wave's phase-C cycles)
#define DMF2_STAMP_DECL unsigned long long st_last = dmf2_stamp(), st_seg[DMF2_NSTAMP] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define DMF2_STAMP(i) { const unsigned long long st_now = dmf2_stamp(); st_seg[i] += st_now - st_last; st_last = st_now; }
// (slot 15: the wave's HW_ID register -- SIMD in bits 5:4 -- so the probe can see where the waves sit)
#define DMF2_STAMP_FLUSH                                                                                        \
    st_seg[15] = __builtin_amdgcn_s_getreg(4 | (31 << 11));                                                     \
    if (lane == 0) for (int i_ = 0; i_ < DMF2_NSTAMP; ++i_) stamps_out[((size_t)blockIdx.x * 4 + wave) * DMF2_NSTAMP + i_] = st_seg[i_];
__device__ __forceinline__ unsigned long long dmf2_stamp() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define DMF2_SUB_BEGIN unsigned long long st_sub = dmf2_stamp();
#define DMF2_SUB(i) { const unsigned long long st_now = dmf2_stamp(); st_seg[i] += st_now - st_sub; st_sub = st_now; }
#else
#define DMF2_STAMP_DECL
#define DMF2_STAMP(i)
#define DMF2_STAMP_FLUSH
#define DMF2_SUB_BEGIN
#define DMF2_SUB(i)
#endif

// Diagnostic switches (tools/rowpass2_probe.hip times the kernel without either from this source): DMF_CHAIN_NO_UNROLL
// (the written-out step loop at kUnrolledSteps), DMF_CHAIN_NO_I32 (M digit pairs joined in i32 before the conversion).
#ifndef DMF_V2_STAGGER
#define DMF_V2_STAGGER 12  // x 64 cycles: how long the waves that do not run phase B hold back their prefetch
#endif
#ifndef DMF_V2_DEFER_PRIO
#define DMF_V2_DEFER_PRIO 1  // s_setprio of the deferred phase C (phase B runs at 3, the tile stores at 1)
#endif
#ifndef DMF_V2_STAGGER_DEFER
#define DMF_V2_STAGGER_DEFER 0  // the same on the deferred-C schedule, whose other waves are not idle
#endif

namespace {
constexpr int kRowV = 66;  // V tile row: 64 samples + 16 B pad (f64)
constexpr int kRowD = 72;  // count tile row: 64 samples as u16 + 16 B pad (36 dwords: rows 4, 8, 12 apart start 16, 32, 48 banks apart)
constexpr int kTileVBytes2 = 16 * kRowV * 8;
constexpr int kTileDBytes2 = 16 * kRowD * 2;
constexpr int kTileBytes2 = kTileVBytes2 + kTileDBytes2;  // one column group: V (f64), counts (u16, as they arrive)
constexpr int kTileBytesX = 2 * kTileDBytes2;               // X16 form: counts and methylated counts, both u16
constexpr int kRingBlockBytes = 16 * 64;                    // deferred-C schedule: a block's x as bytes, 16 rows x 64 samples
constexpr int kRingBytes = 6 * kRingBlockBytes;             // ... a wave's ring: three pairs of blocks
constexpr int kDeferUbufSets = 6;                           // ... and the workgroup's u of three pairs
constexpr int kTileDBytes8 = kRowpassImageBytes;            // byte form: a block's counts as bytes, the image of D8 (no padding)
}  // namespace

template <int NU, bool AT_PREV>
__device__ __forceinline__ void inner_steps(double& uu, double& up, double cj, const double (&Ms)[NU], int b_lo, int b_hi,
                                            int t_end, int lane0) {
    int t2 = 0;
    for (; t2 + 1 < t_end; t2 += 2) {
        inner_step<NU, AT_PREV>(uu, up, cj, Ms, b_lo, b_hi, t2, lane0);      // new u in `up`, previous u in `uu`
        inner_step<NU, AT_PREV>(up, uu, cj, Ms, b_lo, b_hi, t2 + 1, lane0);  // and back
    }
    if (t2 < t_end) {
        inner_step<NU, AT_PREV>(uu, up, cj, Ms, b_lo, b_hi, t2, lane0);
        const double tmp = uu;
        uu = up;
        up = tmp;
    }
}

// The CLI's default n_iter2 has its step loop written out: beta_t then comes from a CONSTANT lane, so the v_readlane pair
// of a step waits for no scalar add (a lane select written by the scalar unit costs wait states before v_readlane may
// use it) and stands off the dependent chain, and the loop's counter, compare and branch are gone.  Same values, same
// arithmetic, same order.  (An even count: (u, u_) swap roles every step.)
constexpr int kUnrolledSteps = 20;

template <int NU, bool AT_PREV>
__device__ __forceinline__ void inner_steps_unrolled(double& uu, double& up, double cj, const double (&Ms)[NU], int b_lo, int b_hi,
                                                     int lane0) {
    static_assert(kUnrolledSteps % 2 == 0 && kUnrolledSteps <= 64, "pairs of steps; beta_t in lane t of one register pair");
#pragma unroll
    for (int t2 = 0; t2 < kUnrolledSteps; t2 += 2) {
        inner_step<NU, AT_PREV>(uu, up, cj, Ms, b_lo, b_hi, t2, lane0);
        inner_step<NU, AT_PREV>(up, uu, cj, Ms, b_lo, b_hi, t2 + 1, lane0);
    }
}

// MAXW: most waves (64-sample column groups) a workgroup may have.  4: S <= 256, two workgroups per CU.  8: S <= 512, ONE
// workgroup of up to eight waves per CU -- nothing hides its phase B, but a block then carries twice the samples, so the
// time per element is that of the four-wave form (measured: DESIGN.md section 5).
// XS: the problem's methylated read counts x = d v are exact integers (X16, u16, D16's layout; dmf_problem_create checks
// |fma(v, d, -x)| <= 8 ulp of x): the kernel never needs V itself, only d v -- phase A forms w = d (v - Rt a1) as
// fma(d, -Rt a1, x), phase C multiplies u by x -- and reads 4 bytes per element instead of 10.  V is not read.
// PAIR (XS, MAXW = 4, NW >= 2, launched where rowpass_v2_plan says pair): two blocks per barrier cycle, their phases B at the
// same time on two waves -- see the block loop.  Each block of a pair has its own tile, slot and ubuf set.
// DEFER_C (PAIR, four waves, every x <= 255, launched where the plan says defer_c): a wave runs phase C only in the barrier
// cycles in which it is not one of the two phase-B waves, for the two pairs then pending, between barriers X and Y; x
// goes from the staging registers into a ring of three pairs per wave as BYTES and is kept nowhere else (phase A reads
// it there too: no x tile), u waits in ubuf sets of three pairs -- see the block loop.
// BYTES (DEFER_C, the problem carries the byte images X8 / D8 of dmf_rowpass_image.h): x and the counts arrive as the bytes
// the ring and the count tile hold -- one 16-byte load and one 16-byte LDS write per lane, block and array, no permute;
// phase A reads its four counts as one dword, the integer product its digits from bytes.  X16 / D16 are not read: the
// images come in their parameters (D16 = D8, X16 = X8), so that the other instances' arguments stay what they were.
template <int NKC, int NU, int MAXW = 4, bool XS = false, bool PAIR = false, bool DEFER_C = false, bool BYTES = false>
__global__ __launch_bounds__(64 * MAXW, MAXW == 4 ? 2 : 1) void k_rowpass_v2(
    const double* __restrict__ V, const unsigned short* __restrict__ D16, const unsigned short* __restrict__ X16, int SD,
    const double* __restrict__ Rtp,
    const double* __restrict__ alpha, double* __restrict__ u, double* __restrict__ u_prev,
    const SolverState* __restrict__ state, int64_t N, int S, int n_c, int n_iter2, int mode, int nd,
    double* __restrict__ slab, double* __restrict__ u2_partials
#ifdef DMF_STAMPS
    , unsigned long long* __restrict__ stamps_out
#endif
    ) {
    static_assert(NU >= 1 && NU <= 4, "one phase-B pass per block, 4x4x4 MFMA for the c product");
    static_assert(!PAIR || (XS && MAXW == 4), "the pair schedule: X16 form, two workgroups per CU");
    static_assert(!DEFER_C || PAIR, "the deferred-C schedule is a pair schedule");
    static_assert(!BYTES || DEFER_C, "the byte images are the deferred-C schedule's");
    constexpr int NSET = PAIR ? 2 : 1;  // tile / slot sets: blocks in flight per barrier cycle
    constexpr int NUB = DEFER_C ? kDeferUbufSets : NSET;  // ubuf sets (DEFER_C: pair p's blocks in sets 2 (p % 3), + 1)
    constexpr int NCT = 4 * NKC;
    constexpr int NP = NU * (NU + 1) / 2;
    // a (row, unknown j) slot of a wave's partial sums: { c_j, M_jj, M_j(j+1), .. (round the row) } pre-scaled by 1 / l_w (M negated),
    // padded to whole 16-byte pieces -- phase B fetches its lane's slot with SLOT / 2 ds_read_b128 per column group
    constexpr int SLOT = (NU + 2) & ~1;
    constexpr int NV = NU * SLOT;  // doubles per row
    extern __shared__ double lds_dyn[];
    if (state->done) return;

    const int NW = blockDim.x >> 6;  // column groups = waves
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int wcol0 = wave * 64;

    // LDS carve-up (doubles unless noted): beta[n_iter2 (even)] | ubuf[NUB][16][NU] | red[NSET][MAXW][16][NU][SLOT] |
    //   u2[MAXW] | tiles[NSET][NW]{ V f64 [16][66], counts u16 [16][72] }  (XS: { counts u16 [16][72], x u16 [16][72] })
    //   (DEFER_C: tiles hold the counts only; BYTES: as u8 [16][64] in the ring slot's order) | ring[NW][3 pairs][2 blocks]{ x u8 [16][64] }
    double* __restrict__ beta_tab = lds_dyn;
    double* __restrict__ ubuf = beta_tab + ((n_iter2 + 1) & ~1);
    double* __restrict__ red = ubuf + NUB * 16 * NU;
    double* __restrict__ u2red = red + NSET * MAXW * NV * 16;
    constexpr int TB = XS ? (BYTES ? kTileDBytes8 : DEFER_C ? kTileDBytes2 : kTileBytesX) : kTileBytes2;
    char* __restrict__ tile = reinterpret_cast<char*>(u2red + MAXW) + (size_t)wave * TB;  // (this wave's tile of set 0)
    // the counts stay u16 in the tile (LINEAR rows: no piece swap): phase A and phase C convert what they read, the integer
    // product builds its balanced byte digits from 32 bytes of a row -- converting at the tile store (f32 copy + two digit
    // planes: 52 vector instructions and 8 LDS writes per block and wave, on every wave's critical path) cost 9 % of the kernel.
    // (XS) x in the same linear layout as the counts, read with the same offsets: no swizzle
    struct BlockTile {
        double* V;              // (V form)
        unsigned short *D, *X;  // counts; (XS) x
    };
    auto block_tile = [&](int set) {  // this wave's tile of set `set`
        char* const t = tile + (size_t)set * NW * TB;
        unsigned short* const d = reinterpret_cast<unsigned short*>(t + (XS ? 0 : kTileVBytes2));
        return BlockTile{reinterpret_cast<double*>(t), d, d + 16 * kRowD};
    };
    // (DEFER_C) this wave's x ring behind the tiles: block b of pair p in slot 2 (p % 3) + b, from its tile store in cycle p to
    // its last phase C in cycle p + 2 (the drain at the latest); pair p + 3 follows behind that in this wave's own program
    // order.  A slot's 16 rows of 64 bytes stand in the order (row & 3, row >> 2), and row r's 16 dwords are rotated by
    // 4 (r & 3): the four rows R, R + 4, R + 8, R + 12 that one phase-C read touches are then 64 consecutive dwords, and the
    // 16 rows x 4 dwords of one phase-A read fall into 64 different banks -- no padding, no bank conflict on either.
    unsigned int* const ring = reinterpret_cast<unsigned int*>(tile + (size_t)(NSET * NW - wave) * TB + (size_t)wave * kRingBytes);
    auto ring_at = [&](int slot, int row, int dword) {
        return ring + slot * (kRingBlockBytes / 4) + (4 * (row & 3) + (row >> 2)) * 16 + ((dword + 4 * (row & 3)) & 15);
    };
    static_assert(rowpass_image_dword(7, 9) == (4 * 3 + 1) * 16 + ((9 + 12) & 15) && kRingBlockBytes == kRowpassImageBytes,
                  "a ring slot is an image of dmf_rowpass_image.h");
    // (BYTES) the count tile of set `set` holds the same image: the strip read of phase A is the ring's, and the 16 samples
    // 16 q .. 16 q + 15 of row m16 that the integer product reads per lane are one 16-byte piece of it -- the 16 lanes that a
    // ds_read_b128 serves together (see the tile swizzle below) touch 16 different pieces modulo 256 bytes
    auto dtile8 = [&](int set) { return reinterpret_cast<unsigned int*>(tile + (size_t)set * NW * TB); };

    // momentum coefficients of the inner steps (deconvolution.py:83-85): from the host's row of ratios when there is one
    // (SolverState), else the recurrence itself by one thread -- n_iter2 square roots and divisions in a row, ~5 us
    if (const double* __restrict__ mrow = momentum_row(state, n_iter2)) {
        const double lw_prev = state->l_w_prev, lw = state->l_w;
        for (int t2 = threadIdx.x; t2 < n_iter2; t2 += blockDim.x)
            beta_tab[t2] = fmin(mrow[2 + t2], t2 == 0 ? 0.9999 * sqrt(lw_prev / lw) : 0.9999);  // l_w_ = l_w behind step 0 (:89)
    } else if (threadIdx.x == 0) {
        fill_momentum_table(state, n_iter2, beta_tab);
    }
    // the partial-sum slots of column groups this workgroup does not have stay zero (phase B adds all MAXW of them,
    // unrolled, so that its LDS reads go out in one batch)
    for (int i = threadIdx.x; i < NSET * MAXW * NV * 16; i += blockDim.x) red[i] = 0.0;
    // x / l_w as x * (1 / l_w), folded into the operands that produce c and M: <= 1 ulp from the division
    const double inv_lw = 1.0 / state->l_w;
    // M arrives as an exact integer multiple of 2^-52; phase B adds -M x / l_w.  (Wave-uniform: kept on the scalar side.)
    const double m_scale_v = -inv_lw * 0x1p-52;
    const double m_scale = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(m_scale_v)),
                                            __builtin_amdgcn_readfirstlane(__double2loint(m_scale_v)));

    // ---- alpha-derived MFMA A operands of this wave's four 16-sample strips, in registers for the whole launch
    const int m16 = lane & 15, q = lane >> 4;
    // Tile swizzle.  A 16-byte LDS read is served in four groups of 16 lanes that are NOT the four rows of 16 lanes
    // ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, and the same + 32): with lane = (row m16, sample piece q) a group holds
    // rows 0-3 / 12-15 at piece q0 and rows 4-11 at piece q0 + 1 (or the other way round), and in any LINEAR layout two of
    // those 16 lanes share a bank.  So rows 4..11 of every tile keep their 16-byte pieces pairwise swapped (a sample s of
    // such a row sits where s ^ 4 would; V only: the u16 counts are read in 8-byte and 2-byte pieces, which a linear row with a
    // 36-dword stride serves without conflicts) -- then each group
    // reads 16 different rows at one piece offset, and the odd piece stride (33) makes that conflict-free.
    const int sw_row = (m16 >= 4 && m16 < 12) ? 1 : 0;  // is row m16 a swapped row (phase A: lane = (row, piece))
    const int qs = q ^ sw_row;                           // where this lane's piece q sits in row m16
    // Phase C reads with lane = (row quad member q, sample m16): rows R + 8 (q & 1) + 4 (q >> 1), R = 0..3, so that the two
    // rows a 32-lane group of a ds_read_b64 touches lie 8 apart -- 8 x 132 dwords = 32 banks: the halves of the 64
    const int c_row = 8 * (q & 1) + 4 * (q >> 1);
    const int mC = m16 ^ ((q == 1 || q == 2) ? 4 : 0);   // (rows 8..11 and 4..7 are swapped rows)
    const int e_col = wcol0 + 4 * (m16 & 3) + (m16 >> 2);  // + 16 t: first product, m <-> sample
    const int k_col = wcol0 + 4 * q;                        // + 16 t + r: k-step r, k = q <-> sample
    double a1r[4][NKC > 0 ? NKC : 1];  // -alpha_known[k = 4 kc + q][sample]
    double a2r[4][4];                  // alpha_unk[m16 & 3][sample] (c product, 4x4x4: block = 4 rows, i = unknown)
    // M product (M_i[pair] = sum_s alpha_j alpha_l d_is) on the INTEGER matrix cores, exactly: the counts are one or two
    // balanced 8-bit digits, P = alpha_j alpha_l in [0, 1] seven digits of rint(P 2^52) (dmf_fixedpoint.h), one
    // v_mfma_i32_16x16x64_i8 per digit covers the wave's 64 samples (A = count digits [row][sample], B = digit t of
    // P [sample][pair]).  An FP64 MFMA holds the SIMD's FP64 pipe for 64 cycles, and this product was 16 of the 28 per
    // block and wave -- time during which the other workgroup's phases B and C on the same SIMD could not issue.
    v4i pdg[7];  // B operands: digit t of P[pair = m16][samples 16 q .. 16 q + 15 of this column group]
    int pj = 0, pl = 0;  // pair m16 = (pj <= pl)
    while ((pl + 1) * (pl + 2) / 2 <= m16) ++pl;
    pj = m16 - pl * (pl + 1) / 2;
    {
        const bool pair_ok = m16 < NP;
        const bool a2_ok = (m16 & 3) < NU;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int kc = 0; kc < NKC; ++kc) {
                const int row = kc * 4 + q, col = e_col + 16 * t;
                a1r[t][kc] = (row < n_c && col < S) ? -alpha[(int64_t)row * S + col] : 0.0;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = k_col + 16 * t + r;
                a2r[t][r] = (col < S && a2_ok) ? alpha[(int64_t)(n_c + (m16 & 3)) * S + col] * inv_lw : 0.0;
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {  // four samples per dword of each digit
            unsigned int lo[4], hi[4], tl[4], th[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int col = wcol0 + 16 * q + 4 * g + i;
                const bool in = pair_ok && col < S;
                const double aj = in ? alpha[(int64_t)(n_c + pj) * S + col] : 0.0;
                const double al = in ? alpha[(int64_t)(n_c + pl) * S + col] : 0.0;
                z_to_biased(aj, al, lo[i], hi[i]);
            }
            transpose4(lo, tl);
            transpose4(hi, th);
            pdg[0][g] = (int)(tl[0] ^ 0x80808080u);
            pdg[1][g] = (int)(tl[1] ^ 0x80808080u);
            pdg[2][g] = (int)(tl[2] ^ 0x80808080u);
            pdg[3][g] = (int)(tl[3] ^ 0x80808080u);
            pdg[4][g] = (int)(th[0] ^ 0x80808080u);
            pdg[5][g] = (int)(th[1] ^ 0x80808080u);
            pdg[6][g] = (int)th[2];
        }
    }
    __syncthreads();  // beta_tab, the zeroed slots

    double bu[4] = {0.0, 0.0, 0.0, 0.0};  // b_u[unknown q][sample 16 t + m16] of this wave's column group, t = 0..3
    double u2_acc = 0.0;
    DMF2_STAMP_DECL
    const int64_t nblk = (N + 15) / 16;
    const int nk = (int)((nblk - blockIdx.x + gridDim.x - 1) / gridDim.x);  // blocks of this workgroup

    // global -> register staging: V load i covers rows 2i, 2i+1 (lane -> row half, 2 samples);
    // D16 / X16 load i covers rows 8i .. 8i+7 (lane -> row lane >> 3, 8 samples); one staging set per block in flight
    const int ld_row = lane >> 5;
    const int ld_col = (lane & 31) * 2;
    int ld_gcol = wcol0 + ld_col;
    // ragged last column group: clamped samples meet zero counts.  Odd S: the row's last sample shares its pair with the
    // next row's first element (or, on the last row, with a zero from the descriptor's range check) -- a finite value
    // against a zero count; rows then start 8 bytes off a 16-byte boundary every other time, which 16-byte buffer loads
    // take (tools/align_probe.hip).
    const int last_pair = (S - 1) & ~1;
    if (ld_gcol > last_pair) ld_gcol = last_pair;
    const int d_row = lane >> 3, d_col = (lane & 7) * 8;
    // (tile swizzle at the stores: V rows 2 i, 2 i + 1 are swapped rows for i = 2..5)
    const int ld_col_sw = ((lane & 31) ^ 2) * 2;
    v2d pv[NSET][XS ? 1 : 8];  // (XS: V is not read)
    v4u pd[NSET][BYTES ? 1 : 2], px[NSET][BYTES ? 1 : XS ? 2 : 1];  // (BYTES: a lane's 16 bytes of the block's image)
    double nrt[NSET][NKC > 0 ? NKC : 1];
    double pu, pup;  // u / u_ of lane (row, unknown) for the wave that runs the block's inner iterations
    constexpr int RPWB = 64 / NU;  // >= 16 rows per wave: one phase-B pass covers the block
    const int rl = lane / NU, jb = lane - rl * NU;
    const bool b_lane = rl < 16 && rl < RPWB;
    // The block's loads are BUFFER loads: address = descriptor base (scalar: array + block offset, recomputed per block on
    // the scalar unit) + a loop-invariant per-lane byte offset + a scalar / immediate offset per instruction -- no vector
    // address arithmetic at all (the flat-address form of this prefetch cost ~80 vector instructions per block and wave,
    // and the row pass is bound by the SIMD's issue slots).  The descriptor's range check replaces the clamps of the
    // last, partial block: rows at or beyond N read as zero, and their counts are zero.
    const unsigned int v_off = (unsigned int)(ld_row * S + ld_gcol) * 8u;               // V: row ld_row of a row pair
    const unsigned int d_off = BYTES ? (unsigned int)(wave * kRowpassImageBytes + lane * 16)  // (BYTES) piece `lane` of the wave's image
                                     : (unsigned int)(d_row * SD + wcol0 + d_col) * 2u;     // counts: row d_row of eight
    const unsigned int r_off = (unsigned int)(m16 * NCT + q) * 8u;                      // R_trunc (padded copy): row m16
    const unsigned int u_off = b_lane ? (unsigned int)lane * 8u : 0xFFFFFFF0u;          // u / u_: (row, unknown) = lane
    auto span = [](int64_t bytes) { return (unsigned int)(bytes < 0 ? 0 : (bytes > 0x7FFFFFFF ? 0x7FFFFFFF : bytes)); };
    // u / u_ of block blk.  FIRST in a prefetch's batch: the tile store's wait for the (younger) tile loads then covers
    // them, and phase B finds its u / u_ complete without a vmcnt wait of its own -- a wait there would also cover the
    // NEXT block's prefetch, issued just before barrier X, and put a whole HBM round trip on the critical path.
    auto prefetch_u = [&](int64_t blk) {
        const int64_t r0 = blk * 16;
        const int64_t left = N - r0;  // rows of the arrays from this block on (> 0)
        const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc((void*)(u + r0 * NU), 0, span(left * NU * 8), 0x00020000);
        const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc((void*)(u_prev + r0 * NU), 0, span(left * NU * 8), 0x00020000);
        const v2u a = __builtin_amdgcn_raw_buffer_load_b64(ru, u_off, 0, 0);
        const v2u b = __builtin_amdgcn_raw_buffer_load_b64(rp, u_off, 0, 0);
        pu = __hiloint2double((int)a.y, (int)a.x);
        pup = __hiloint2double((int)b.y, (int)b.x);
    };
    // R_trunc rows and the tile data of block blk into staging set `set`
    auto prefetch_tile = [&](int64_t blk, int set) {
        const int64_t r0 = blk * 16;
        const int64_t left = N - r0;
        if (NKC > 0) {
            const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc((void*)(Rtp + r0 * NCT), 0, span(left * NCT * 8), 0x00020000);
#pragma unroll
            for (int kc = 0; kc < NKC; ++kc) {
                const v2u a = __builtin_amdgcn_raw_buffer_load_b64(rr, r_off, kc * 32, 0);
                nrt[set][kc] = __hiloint2double((int)a.y, (int)a.x);
            }
        }
        if constexpr (BYTES) {
            // (both images are zero-padded to whole blocks and to SD: always in range; a block's SD / 64 images are consecutive)
            const unsigned char* const X8 = reinterpret_cast<const unsigned char*>(X16);
            const unsigned char* const D8 = reinterpret_cast<const unsigned char*>(D16);
            const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(X8 + r0 * SD), 0, span((int64_t)16 * SD), 0x00020000);
            const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)(D8 + r0 * SD), 0, span((int64_t)16 * SD), 0x00020000);
            px[set][0] = __builtin_amdgcn_raw_buffer_load_b128(rx, d_off, 0, 0);
            pd[set][0] = __builtin_amdgcn_raw_buffer_load_b128(rd, d_off, 0, 0);
        } else if constexpr (!XS) {
            const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void*)(V + r0 * S), 0, span(left * S * 8), 0x00020000);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const v4u a = __builtin_amdgcn_raw_buffer_load_b128(rv, v_off, 2 * i * S * 8, 0);
                pv[set][i] = v2d{__hiloint2double((int)a.y, (int)a.x), __hiloint2double((int)a.w, (int)a.z)};
            }
        } else {
            // (X16 is zero-padded like the counts: always in range)
            const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(X16 + r0 * SD), 0, span((int64_t)16 * SD * 2), 0x00020000);
            px[set][0] = __builtin_amdgcn_raw_buffer_load_b128(rx, d_off, 0, 0);
            px[set][1] = __builtin_amdgcn_raw_buffer_load_b128(rx, d_off, 8 * SD * 2, 0);
        }
        if constexpr (!BYTES) {
            // (the count copy is zero-padded to whole blocks of 16 rows: always in range)
            const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)(D16 + r0 * SD), 0, span((int64_t)16 * SD * 2), 0x00020000);
            pd[set][0] = __builtin_amdgcn_raw_buffer_load_b128(rd, d_off, 0, 0);
            pd[set][1] = __builtin_amdgcn_raw_buffer_load_b128(rd, d_off, 8 * SD * 2, 0);
        }
    };
    // the block of a barrier cycle starting at block index s whose phase B this wave runs (1: block s + 1, pairs only), and
    // so the block whose u / u_ it prefetches (a wave that runs none loads block s's: never used)
    auto pair_set = [&](int s) { return (PAIR && s + 1 < nk && wave == (s + 1) % NW) ? 1 : 0; };
    if (nk > 0) {
        prefetch_u(blockIdx.x + (int64_t)pair_set(0) * gridDim.x);
        prefetch_tile(blockIdx.x, 0);
        if (PAIR && nk > 1) prefetch_tile(blockIdx.x + gridDim.x, 1);
    }

    // this lane's places in its wave's partial-sum slots: c[unknown q][row m16]; M[pair m16 = (pj, pl)][rows 4 q ..] twice
    // (M is symmetric), a slot's M entries in ROTATED order -- slot (row, j) entry r is M[j][(j + r) % NU], the order in
    // which phase B's quad rotations deliver the iterate; rows 4 q + rr at immediate offsets (slot set 0; set 1 follows)
    double* __restrict__ const mine_c = red + (size_t)wave * NV * 16 + (m16 * NU + q) * SLOT;
    double* __restrict__ const mine_m1 = red + (size_t)wave * NV * 16 + (4 * q * NU + pl) * SLOT + 1 + (pj - pl + NU) % NU;
    double* __restrict__ const mine_m2 = red + (size_t)wave * NV * 16 + (4 * q * NU + pj) * SLOT + 1 + (pl - pj) % NU;

    // ---- tile store of staging set `set` into the wave's tile of that set (waits for the prefetched loads)
    auto tile_store = [&](int set, int rslot) {
        const BlockTile T = block_tile(set);
        if constexpr (BYTES) {
            // the images as they arrived: piece `lane` of ring slot rslot and of the count tile
            *reinterpret_cast<v4u*>(ring + rslot * (kRingBlockBytes / 4) + 4 * lane) = px[set][0];
#ifndef DMF_ABLATE_DSTORE
            *reinterpret_cast<v4u*>(dtile8(set) + 4 * lane) = pd[set][0];
#endif
        } else if constexpr (DEFER_C) {
            // x as bytes (the low byte of each u16: every x <= 255) into ring slot rslot: two dwords of row 8 i + d_row
#pragma unroll
            for (int i = 0; i < 2; ++i)
                *reinterpret_cast<v2u*>(ring_at(rslot, 8 * i + d_row, 2 * (lane & 7))) =
                    v2u{__builtin_amdgcn_perm(px[set][i].y, px[set][i].x, 0x06040200u),
                        __builtin_amdgcn_perm(px[set][i].w, px[set][i].z, 0x06040200u)};
        } else if constexpr (XS) {
#pragma unroll
            for (int i = 0; i < 2; ++i) *reinterpret_cast<v4u*>(T.X + (8 * i + d_row) * kRowD + d_col) = px[set][i];
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                *reinterpret_cast<v2d*>(T.V + (2 * i + ld_row) * kRowV + ((i >= 2 && i < 6) ? ld_col_sw : ld_col)) = pv[set][i];
        }
#ifndef DMF_ABLATE_DSTORE
        if constexpr (!BYTES) {
#pragma unroll
            for (int i = 0; i < 2; ++i) *reinterpret_cast<v4u*>(T.D + (8 * i + d_row) * kRowD + d_col) = pd[set][i];
        }
#endif
    };

    // ---- phase A of the block in tile set `set` (R_trunc rows: staging set `set`) -> partial sums in slot set `set`
    auto phase_a = [&](int set, int rslot, int st_a, int st_p) {
        const BlockTile T = block_tile(set);
        const double* __restrict__ const tileV = T.V;
        unsigned short* __restrict__ const tileD = T.D;
        unsigned short* __restrict__ const tileX = T.X;
        const double (&rtop)[NKC > 0 ? NKC : 1] = nrt[set];  // B operand of the first product: Rt^T[k = 4 kc + q][n = row]
        // strips of 16 samples; the LDS reads of strip t + 1 are issued before the MFMAs of strip t, and the E chain of
        // strip t + 1 is slotted between the c / M MFMAs of strip t (a dependent FP64 MFMA stalls behind its producer)
        struct StripV {
            v2d v01, v23;
            v2u dw;  // the four counts of the piece, u16
        };
        struct StripX {
            v2u dw, xw;  // the four counts and the four x = d v of the piece, u16
        };
        using Strip = std::conditional_t<XS, StripX, StripV>;
        auto load_strip = [&](int t, Strip& R) {
            if constexpr (DEFER_C) {
                R.xw.x = *ring_at(rslot, m16, 4 * t + q);  // the piece's four x as bytes
            } else if constexpr (XS) {
                R.xw = *reinterpret_cast<const v2u*>(tileX + m16 * kRowD + t * 16 + 4 * q);
            } else {
                const double* __restrict__ tv = tileV + m16 * kRowV + t * 16 + 4 * qs;
                R.v01 = *reinterpret_cast<const v2d*>(tv);
                R.v23 = *reinterpret_cast<const v2d*>(tv + 2);
            }
            if constexpr (BYTES) R.dw.x = dtile8(set)[rowpass_image_dword(m16, 4 * t + q)];  // the piece's four counts as bytes
            else R.dw = *reinterpret_cast<const v2u*>(tileD + m16 * kRowD + t * 16 + 4 * q);
        };
        double csm0 = 0.0, csm1 = 0.0;  // c[unknown q][row m16], one double per lane
        // E = V - Rt a_known; XS: E = -Rt a_known, and V enters through x below
        auto e_init = [&](const Strip& R) {
            if constexpr (XS) return v4d{0.0, 0.0, 0.0, 0.0};
            else return v4d{R.v01.x, R.v01.y, R.v23.x, R.v23.y};
        };
        auto run_strip = [&](const Strip& R, v4d e, const Strip& Rn, const double (&a1n)[NKC > 0 ? NKC : 1],
                             const double (&a2)[4], bool has_next) {
            const v4d d = BYTES ? v4d{(double)(R.dw.x & 0xFFu), (double)((R.dw.x >> 8) & 0xFFu), (double)((R.dw.x >> 16) & 0xFFu), (double)(R.dw.x >> 24)}
                                : v4d{(double)(R.dw.x & 0xFFFFu), (double)(R.dw.x >> 16), (double)(R.dw.y & 0xFFFFu), (double)(R.dw.y >> 16)};
            v4d w;
            if constexpr (XS) {  // w = d (v - Rt a1) = fma(d, -Rt a1, x)
                const v4d x = DEFER_C ? v4d{(double)(R.xw.x & 0xFFu), (double)((R.xw.x >> 8) & 0xFFu), (double)((R.xw.x >> 16) & 0xFFu), (double)(R.xw.x >> 24)}
                                      : v4d{(double)(R.xw.x & 0xFFFFu), (double)(R.xw.x >> 16), (double)(R.xw.y & 0xFFFFu), (double)(R.xw.y >> 16)};
#pragma unroll
                for (int r = 0; r < 4; ++r) w[r] = fma(d[r], e[r], x[r]);
            } else {
                w = d * e;
            }
            v4d en = e_init(Rn);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (r & 1) csm1 = __builtin_amdgcn_mfma_f64_4x4x4f64(a2[r], w[r], csm1, 0, 0, 0);
                else csm0 = __builtin_amdgcn_mfma_f64_4x4x4f64(a2[r], w[r], csm0, 0, 0, 0);
                if (has_next && r < NKC) en = __builtin_amdgcn_mfma_f64_16x16x4f64(a1n[r], rtop[r], en, 0, 0, 0);
            }
            return en;
        };
#ifdef DMF_ABLATE_E
        const double csm = XS ? (double)tileX[m16 * kRowD + 4 * q] : tileV[m16 * kRowV + 4 * qs];
#else
        Strip sa, sb;
        load_strip(0, sa);
        load_strip(1, sb);
        __builtin_amdgcn_sched_barrier(0);
        v4d e0 = e_init(sa);
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc) e0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1r[0][kc], rtop[kc], e0, 0, 0, 0);
        const v4d e1 = run_strip(sa, e0, sb, a1r[1], a2r[0], true);
        load_strip(2, sa);
        __builtin_amdgcn_sched_barrier(0);
        const v4d e2 = run_strip(sb, e1, sa, a1r[2], a2r[1], true);
        load_strip(3, sb);
        __builtin_amdgcn_sched_barrier(0);
        const v4d e3 = run_strip(sa, e2, sb, a1r[3], a2r[2], true);
        (void)run_strip(sb, e3, sb, a1r[3], a2r[3], false);
        const double csm = csm0 + csm1;
#endif
        // M on the integer matrix cores: digit weights 256^0 .. 256^7 (count digit d + P digit t -> weight t + d)
        v4i mw[8];
#pragma unroll
        for (int w8 = 0; w8 < 8; ++w8) mw[w8] = v4i{0, 0, 0, 0};
#ifndef DMF_ABLATE_M  // (diagnostic builds of tools/rowpass2_probe.hip leave pieces out to see what they cost)
        if constexpr (BYTES) {
            // A from bytes: d + 128 = b0 + 256 b1 with b0 = d ^ 0x80, so digit 0 = b0 - 128 is the byte d itself read as i8, and
            // digit 1 = b1 is its top bit -- the same digits as below
            const v4u wd = *reinterpret_cast<const v4u*>(dtile8(set) + rowpass_image_dword(m16, 4 * q));
            const v4i c0 = {(int)wd.x, (int)wd.y, (int)wd.z, (int)wd.w};
#pragma unroll
            for (int t = 0; t < 7; ++t) mw[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(c0, pdg[t], mw[t], 0, 0, 0);
            if (nd == 2) {
                const v4i c1 = {(int)((wd.x >> 7) & 0x01010101u), (int)((wd.y >> 7) & 0x01010101u),
                                (int)((wd.z >> 7) & 0x01010101u), (int)((wd.w >> 7) & 0x01010101u)};
#pragma unroll
                for (int t = 0; t < 7; ++t) mw[t + 1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(c1, pdg[t], mw[t + 1], 0, 0, 0);
            }
        } else {
            // A: counts [row m16][samples 16 q .. 16 q + 15] as balanced digits: d + 128 = b0 + 256 b1, digit 0 = b0 - 128
            // (b0 ^ 0x80 as i8), digit 1 = b1
            const v4u wa = *reinterpret_cast<const v4u*>(tileD + m16 * kRowD + 16 * q);
            const v4u wb = *reinterpret_cast<const v4u*>(tileD + m16 * kRowD + 16 * q + 8);
            const unsigned int e0 = wa.x + 0x00800080u, e1 = wa.y + 0x00800080u, e2 = wa.z + 0x00800080u, e3 = wa.w + 0x00800080u;
            const unsigned int e4 = wb.x + 0x00800080u, e5 = wb.y + 0x00800080u, e6 = wb.z + 0x00800080u, e7 = wb.w + 0x00800080u;
            const v4i c0 = {(int)(__builtin_amdgcn_perm(e1, e0, 0x06040200u) ^ 0x80808080u),
                            (int)(__builtin_amdgcn_perm(e3, e2, 0x06040200u) ^ 0x80808080u),
                            (int)(__builtin_amdgcn_perm(e5, e4, 0x06040200u) ^ 0x80808080u),
                            (int)(__builtin_amdgcn_perm(e7, e6, 0x06040200u) ^ 0x80808080u)};
#pragma unroll
            for (int t = 0; t < 7; ++t) mw[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(c0, pdg[t], mw[t], 0, 0, 0);
            if (nd == 2) {
                const v4i c1 = {(int)__builtin_amdgcn_perm(e1, e0, 0x07050301u), (int)__builtin_amdgcn_perm(e3, e2, 0x07050301u),
                                (int)__builtin_amdgcn_perm(e5, e4, 0x07050301u), (int)__builtin_amdgcn_perm(e7, e6, 0x07050301u)};
#pragma unroll
                for (int t = 0; t < 7; ++t) mw[t + 1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(c1, pdg[t], mw[t + 1], 0, 0, 0);
            }
        }
#endif
        // lane (pair m16, q) holds rows 4 q + reg: the exact integer sum_w 256^w mw[w] in two halves that fit a double
        // without rounding (|mw| < 2^21 per digit product sum), one rounding when they are joined.  The digit pairs
        // mw[2k] + 256 mw[2k+1] (< 2^30) are joined in i32 first: four conversions and three FMAs per value on the FP64
        // pipe instead of eight and seven, every intermediate exact either way.
        double mrow[4];
#ifdef DMF_ABLATE_M
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) mrow[rr] = 0.25 * (rr == (m16 & 3));
#else
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
#ifndef DMF_CHAIN_NO_I32
            const double lo = fma((double)(mw[3][rr] * 256 + mw[2][rr]), 65536.0, (double)(mw[1][rr] * 256 + mw[0][rr]));
            const double hi = fma((double)(mw[7][rr] * 256 + mw[6][rr]), 65536.0, (double)(mw[5][rr] * 256 + mw[4][rr]));
#else
            const double lo = fma(fma(fma((double)mw[3][rr], 256.0, (double)mw[2][rr]), 256.0, (double)mw[1][rr]), 256.0, (double)mw[0][rr]);
            const double hi = fma(fma(fma((double)mw[7][rr], 256.0, (double)mw[6][rr]), 256.0, (double)mw[5][rr]), 256.0, (double)mw[4][rr]);
#endif
            mrow[rr] = fma(hi, 0x1p32, lo) * m_scale;
        }
#endif
        DMF2_STAMP(st_a)  // phase A
        {
            const size_t so = (size_t)set * MAXW * NV * 16;  // this block's slot set
            if (q < NU) mine_c[so] = csm;  // c[unknown q][row m16]
            if (m16 < NP) {  // C layout of the 16x16x64 tile: col = pair m16 = (pj, pl), rows 4 q + reg; M is symmetric
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) mine_m1[so + rr * NU * SLOT] = mrow[rr];
                if (pj != pl) {
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) mine_m2[so + rr * NU * SLOT] = mrow[rr];
                }
            }
        }
        DMF2_STAMP(st_p)  // partials
    };

    // ---- phase B of the block at row0 (its partial sums in slot set `set`, its u into ubuf set `uset`): row-local inner
    // iterations, lane = (row, unknown j); c and M pre-scaled by 1 / l_w
    auto phase_b = [&](int uset, int set, int64_t row0, double uu0, double up0) {
        __builtin_amdgcn_s_setprio(3);  // a dependent chain on the workgroup's critical path
        DMF2_SUB_BEGIN
        const bool ok = b_lane && row0 + rl < N;
        const int lane0 = lane - jb;
        const int rlc = rl < 16 ? rl : 15;
        double cj = 0.0, Ms[NU];
#pragma unroll
        for (int l = 0; l < NU; ++l) Ms[l] = 0.0;
        {
            // this lane's slot of every column group, in column-group order (a fixed summation order); the values
            // are already c / l_w and -M / l_w
            const double* __restrict__ slot = red + (size_t)set * MAXW * NV * 16 + (rlc * NU + jb) * SLOT;
#pragma unroll 1
            for (int w0 = 0; w0 < MAXW; w0 += 4) {  // (batches of four column groups: registers)
                v2d part[4][SLOT / 2];
#pragma unroll
                for (int w = 0; w < 4; ++w)
#pragma unroll
                    for (int h = 0; h < SLOT / 2; ++h)
                        part[w][h] = *reinterpret_cast<const v2d*>(slot + (w0 + w) * NV * 16 + 2 * h);
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    cj += part[w][0].x;
#pragma unroll
                    for (int l = 0; l < NU; ++l) Ms[l] += (l & 1) ? part[w][(l + 1) / 2].x : part[w][l / 2].y;
                }
            }
        }
        double uu = uu0, up = up0;
        DMF2_SUB(8)
        // The momentum coefficients ride in a VGPR (lane t holds beta_t) and reach the steps through
        // v_readlane: an LDS read here would sit on the dependent chain every step.
#ifndef DMF_CHAIN_NO_UNROLL
        if (XS && MAXW == 4 && n_iter2 == kUnrolledSteps) {  // (X16 form, up to four waves: the written-out loop at its step count)
            const double bvec = beta_tab[lane < kUnrolledSteps ? lane : kUnrolledSteps - 1];  // (as below)
            const int b_lo = __double2loint(bvec), b_hi = __double2hiint(bvec);
            if (mode == 1) {
                inner_steps_unrolled<NU, true>(uu, up, cj, Ms, b_lo, b_hi, lane0);
            } else {
                Ms[0] += 1.0;
                inner_steps_unrolled<NU, false>(uu, up, cj, Ms, b_lo, b_hi, lane0);
            }
        } else
#endif
        for (int t0 = 0; t0 < n_iter2; t0 += 64) {
            const int tl = t0 + lane < n_iter2 ? t0 + lane : n_iter2 - 1;
            const double bvec = beta_tab[tl];  // (lane t: beta_t; the first read goes out with the partial-sum reads)
            const int b_lo = __double2loint(bvec), b_hi = __double2hiint(bvec);
            const int t_end = n_iter2 - t0 < 64 ? n_iter2 - t0 : 64;
            // (u, u_) swap roles every step: written out in pairs so that no register copies sit on the chain
            // (the loop holds v_readlane, a convergent operation the unroller will not split by itself)
            if (mode == 1) {
                inner_steps<NU, true>(uu, up, cj, Ms, b_lo, b_hi, t_end, lane0);
            } else {
                if (t0 == 0) Ms[0] += 1.0;  // the step's own "+ ut" (deconvolution.py:88), folded into the diagonal
                inner_steps<NU, false>(uu, up, cj, Ms, b_lo, b_hi, t_end, lane0);
            }
        }
        DMF2_SUB(9)
        if (b_lane) ubuf[uset * 16 * NU + rl * NU + jb] = ok ? uu : 0.0;  // rows beyond N: phase C multiplies them by zero counts
        if (ok) {
            // (buffer stores, like the loads: scalar base of the block + this lane's constant offset)
            const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc((void*)(u + row0 * NU), 0, span((N - row0) * NU * 8), 0x00020000);
            const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc((void*)(u_prev + row0 * NU), 0, span((N - row0) * NU * 8), 0x00020000);
            __builtin_amdgcn_raw_buffer_store_b64(v2u{(unsigned int)__double2loint(uu), (unsigned int)__double2hiint(uu)}, ru, u_off, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b64(v2u{(unsigned int)__double2loint(up), (unsigned int)__double2hiint(up)}, rp, u_off, 0, 0);
            u2_acc = fma(uu, uu, u2_acc);
        }
        DMF2_SUB(10)
        __builtin_amdgcn_s_setprio(0);
    };

    // ---- phase C of the block in tile set `set`, u from ubuf set `set`: b_u[j][s] += sum_rows u[row][j] (d v)[row][s] on
    // the 4x4x4 (4 blocks) FP64 MFMA: block = sample quad of a 16-sample strip, i = unknown, j = sample in the quad, k = row
    // in a quad of rows (A[b][i][k] sits at lane 16 k + 4 b + i, B[b][k][j] at lane 16 k + 4 b + j, the result D[b][i][j]
    // at lane 16 i + 4 b + j: tools/mfma_probe.hip).  k may number the rows of a quad in any order: lane (q, m16) reads
    // (d v) of row R + c_row(q), sample 16 t + m16 (at its swizzled place) and u of that row, unknown m16 & 3; the 32 tile
    // reads of the block are independent and go out in two batches (a lane = sample loop with per-row broadcast reads of
    // u spent ~1.6k cycles per block on LDS round trips).
    auto phase_c = [&](int set) {
#ifndef DMF_ABLATE_C
        const BlockTile T = block_tile(set);
        const double* __restrict__ const ub = ubuf + set * 16 * NU;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            double vv[2][4], ua[2];
            unsigned short dd[2][4];  // (XS: x)
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const int row = 2 * half + rr + c_row;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if constexpr (XS) {
                        dd[rr][t] = T.X[row * kRowD + 16 * t + m16];
                    } else {
                        vv[rr][t] = T.V[row * kRowV + 16 * t + mC];
                        dd[rr][t] = T.D[row * kRowD + 16 * t + m16];
                    }
                }
                ua[rr] = (m16 & 3) < NU ? ub[row * NU + (m16 & 3)] : 0.0;
            }
#pragma unroll
            for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    bu[t] = __builtin_amdgcn_mfma_f64_4x4x4f64(ua[rr], XS ? (double)dd[rr][t] : (double)dd[rr][t] * vv[rr][t], bu[t], 0, 0, 0);
        }
#endif
    };

    // ---- (DEFER_C) phase C of block `b01` of pair `pp`: x from the ring, u from the pair's ubuf sets.  The same products in
    // the same order as phase_c on every sample; lane (q, m16) reads ONE dword per row -- samples 4 m16 .. 4 m16 + 3 -- so
    // bu[t] is b_u[unknown q][sample 4 m16 + t] on this schedule (the slab write-out below knows), and a block takes four
    // tile reads instead of sixteen.
    auto phase_c_ring = [&](int pp, int b01) {
        const int rslot = 2 * (pp % 3) + b01;
        const double* __restrict__ const ub = ubuf + (2 * (pp % 3) + b01) * 16 * NU;
        unsigned int xw[4];
        double ua[4];
#pragma unroll
        for (int R = 0; R < 4; ++R) {
            xw[R] = *ring_at(rslot, R + c_row, m16);
            ua[R] = (m16 & 3) < NU ? ub[(R + c_row) * NU + (m16 & 3)] : 0.0;
        }
#pragma unroll
        for (int R = 0; R < 4; ++R)
#pragma unroll
            for (int t = 0; t < 4; ++t)
                bu[t] = __builtin_amdgcn_mfma_f64_4x4x4f64(ua[R], (double)((xw[R] >> (8 * t)) & 0xFFu), bu[t], 0, 0, 0);
    };

    // The block loop: NSET blocks per barrier cycle. One block (NSET = 1): its phase B runs on wave s % NW while the
    // other waves wait at barrier Y.  A pair (NSET = 2): blocks s and s + 1 run their phases A and C one after the other
    // on every wave, their phases B at the same time on waves s % NW and (s + 1) % NW (different waves for NW >= 2, so
    // different SIMDs).  Each block keeps its own tile, slot and ubuf set, the wave and the order of every sum stay those
    // of one block at a time (phase C adds block s before block s + 1), so the results are the same bit for bit.  A
    // workgroup with an odd number of blocks runs its last one alone.
    // Deferred C (DEFER_C, four waves): the phase-B waves of cycle p = s / 2 are {0, 1} for even p and {2, 3} for odd p.  The
    // OTHER two run, between barriers X and Y, phase C of the pairs p - 2 and p - 1 in block order -- both complete pairs,
    // whose phases B ended before an earlier barrier Y -- and nothing follows barrier Y.  Every wave so runs phase C in every
    // second cycle, for every pair once and in order, into the same accumulators: the same sums bit for bit.  Pair p's x
    // stands in ring slots 2 (p % 3), + 1 from its tile store (the slots' former pair p - 3 was last read in cycle p - 1, by
    // this wave itself); pair p's u stands in ubuf sets 2 (p % 3), + 1
    // from its phase B until phase B of pair p + 3, two barriers behind its last reader in cycle p + 2.  What is pending after
    // the last cycle -- its pair, and the one before on the waves that ran its phase B -- is drained behind the loop.
    // (tests/rowpass_schedule_model.py walks this schedule for every block count.)
    for (int s = 0; s < nk; s += NSET) {
        const bool has2 = PAIR && s + 1 < nk;
        const int64_t blk = blockIdx.x + (int64_t)s * gridDim.x;
        const int cyc = s >> 1;                                    // (DEFER_C)
        const bool b_role = !DEFER_C || (wave >> 1) == (cyc & 1);  // (DEFER_C) may run a phase B in this cycle
        __builtin_amdgcn_s_setprio(1);
        const int rs0 = 2 * (cyc % 3);  // (DEFER_C) ring slots = ubuf sets of this cycle's blocks: rs0, rs0 + 1
        tile_store(0, rs0);
        if (has2) tile_store(1, rs0 + 1);
        const int bset = pair_set(s);
        const bool my_turn = bset == 1 || wave == s % NW;
        // the u / u_ of this wave's own block arrived with the tiles (the next prefetch reuses pu / pup before phase B runs)
        const double uu0 = pu;
        const double up0 = pup;
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_setprio(0);
        DMF2_STAMP(0)  // tile stores (vmcnt wait for the prefetch)
        phase_a(0, rs0, 1, 2);
        if (has2) phase_a(1, rs0 + 1, 11, 12);
        // (a bare barrier behind an LDS-only wait: __syncthreads() would also drain vmcnt)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // ---- barrier X
        DMF2_STAMP(3)  // wait X
        // The next cycle's global loads (their staging registers were free during phase A).  42 KB of loads take the CU's
        // one address unit ~700 cycles when a workgroup's waves issue them together: the waves that run phase B go
        // first, the others -- who wait for phase B anyway -- a little later.  (ONE place for all waves: with the loads in
        // two branches the register allocator gave them different destinations and put copies -- and the waits for the
        // data -- behind one of them.)
#ifndef DMF_V2_NO_STAGGER
        if constexpr (!DEFER_C) {
            if (!my_turn) __builtin_amdgcn_s_sleep(DMF_V2_STAGGER);
        } else if (DMF_V2_STAGGER_DEFER > 0) {
            if (!b_role) __builtin_amdgcn_s_sleep(DMF_V2_STAGGER_DEFER);
        }
#endif
        if (s + NSET < nk) {
            const int64_t nb = blk + NSET * (int64_t)gridDim.x;
            prefetch_u(nb + (int64_t)pair_set(s + NSET) * gridDim.x);
            prefetch_tile(nb, 0);
            if (PAIR && s + 3 < nk) prefetch_tile(nb + gridDim.x, 1);
        }
        if (b_role) { DMF2_STAMP(7) } else { DMF2_STAMP(16) }  // prefetch issue (16: in a cycle whose window this wave spends on phase C)
        if (my_turn) phase_b((DEFER_C ? rs0 : 0) + bset, bset, (blk + (int64_t)bset * gridDim.x) * 16, uu0, up0);
        DMF2_STAMP(4)  // phase B (or nothing)
        if constexpr (DEFER_C) {
            if (!b_role) {  // (the window's critical chain: above the other workgroup's phase A, below phase B)
                if (DMF_V2_DEFER_PRIO > 0) __builtin_amdgcn_s_setprio(DMF_V2_DEFER_PRIO);
#pragma unroll 1
                for (int pp = cyc < 2 ? 0 : cyc - 2; pp < cyc; ++pp) {
                    phase_c_ring(pp, 0);
                    phase_c_ring(pp, 1);
                }
                if (DMF_V2_DEFER_PRIO > 0) __builtin_amdgcn_s_setprio(0);
            }
            DMF2_STAMP(6)  // deferred phase C in the window
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // ---- barrier Y
        if (b_role) { DMF2_STAMP(5) } else { DMF2_STAMP(17) }  // wait Y (17: behind phase C)
        if constexpr (!DEFER_C) {
            phase_c(0);
            DMF2_STAMP(6)  // phase C, block s
            if (has2) phase_c(1);
            __builtin_amdgcn_s_setprio(0);
            DMF2_STAMP(13)  // phase C, block s + 1
        }
        // (the next cycle's tile stores touch this wave's own tiles only; ubuf and red are rewritten behind the next
        // barrier X / by phase A after this wave's own phase C)
    }
    if constexpr (DEFER_C) {
        if (nk > 0) {
            // the drain: the last pair (a lone last block: its first half only) and, on the waves that ran the last
            // cycle's phase B, the pair before; their u stands behind the last barrier Y
            const int last = (nk - 1) >> 1;
            const bool lone = (nk & 1) != 0;
            const int first = ((wave >> 1) != (last & 1) || last == 0) ? last : last - 1;
#pragma unroll 1
            for (int pp = first; pp <= last; ++pp) {
                phase_c_ring(pp, 0);
                if (pp < last || !lone) phase_c_ring(pp, 1);
            }
        }
        DMF2_STAMP(13)  // the drain
    }

    DMF2_STAMP_FLUSH
    const double w2 = wave_sum(u2_acc);
    if (lane == 0) u2red[wave] = w2;
    __syncthreads();
    // ---- b_u slab of this workgroup [NU][S] and its share of ||u||_F^2
    if (q < NU) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int sC = wcol0 + (DEFER_C ? 4 * m16 + t : 16 * t + m16);  // (DEFER_C: phase_c_ring's sample order)
            if (sC < S) slab[((int64_t)blockIdx.x * NU + q) * S + sC] = bu[t];
        }
    }
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int w = 0; w < NW; ++w) tot += u2red[w];
        u2_partials[blockIdx.x] = tot;
    }
}

// The byte images of a problem (dmf_rowpass_image.h), once per problem: a thread gathers one 16-byte piece of an image of X8
// and of D8 -- 16 consecutive samples of one row, the low bytes of two 16-byte loads of X16 / D16 (every element <= 255).
// pieces = N16 * SD / 16: piece (block, column group, l) is thread (block * SD / 64 + group) * 64 + l.
__global__ __launch_bounds__(256) void k_build_rowpass_images(const unsigned short* __restrict__ X16, const unsigned short* __restrict__ D16,
                                                              int SD, int64_t pieces, unsigned char* __restrict__ X8,
                                                              unsigned char* __restrict__ D8) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pieces) return;
    const int l = (int)(i & 63), groups = SD >> 6;
    const int64_t img = i >> 6, blk = img / groups;
    const int g = (int)(img - blk * groups);
    const int64_t src = (blk * 16 + rowpass_image_piece_row(l)) * SD + g * 64 + 16 * rowpass_image_piece_col(l);
    auto pack = [&](const unsigned short* __restrict__ a) {
        const v4u lo = *reinterpret_cast<const v4u*>(a + src), hi = *reinterpret_cast<const v4u*>(a + src + 8);
        return v4u{__builtin_amdgcn_perm(lo.y, lo.x, 0x06040200u), __builtin_amdgcn_perm(lo.w, lo.z, 0x06040200u),
                   __builtin_amdgcn_perm(hi.y, hi.x, 0x06040200u), __builtin_amdgcn_perm(hi.w, hi.z, 0x06040200u)};
    };
    *reinterpret_cast<v4u*>(X8 + i * 16) = pack(X16);
    *reinterpret_cast<v4u*>(D8 + i * 16) = pack(D16);
}

hipError_t launch_build_rowpass_images(const unsigned short* X16, const unsigned short* D16, int64_t N16, int SD,
                                       unsigned char* X8, unsigned char* D8, hipStream_t st) {
    if (X16 == nullptr || D16 == nullptr || X8 == nullptr || D8 == nullptr || N16 < 16 || (N16 & 15) != 0 || SD < 64 || (SD & 63) != 0)
        return hipErrorInvalidValue;
    const int64_t pieces = N16 * SD / 16;
    const int64_t grid = (pieces + 255) / 256;
    if (grid > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_build_rowpass_images, dim3((unsigned)grid), dim3(256), 0, st, X16, D16, SD, pieces, X8, D8);
    return hipGetLastError();
}

// ---- the launch plan (dmf_internal.h: RowpassV2Plan): every rule about which instance runs, with what grid and LDS, is here
static size_t rowpass_v2_lds_bytes(int S, int n_u, int n_iter2, bool x16, bool pair = false, bool defer_c = false, bool bytes = false) {
    const int NW = (S + 63) / 64;
    const int maxw = NW <= 4 ? 4 : 8;
    const int nset = pair ? 2 : 1;
    const int nub = defer_c ? kDeferUbufSets : nset;
    const int nv = n_u * ((n_u + 2) & ~1);  // a row's partial-sum slots (k_rowpass_v2: NV)
    const size_t doubles = (size_t)((n_iter2 + 1) & ~1) + (size_t)nub * 16 * n_u + (size_t)nset * maxw * nv * 16 + maxw;
    // (deferred C: x stands in the ring only; its byte form: the counts as the 1 KB image)
    const int tile = bytes ? kTileDBytes8 : defer_c ? kTileDBytes2 : (x16 ? kTileBytesX : kTileBytes2);
    return doubles * sizeof(double) + (size_t)nset * NW * tile + (defer_c ? (size_t)NW * kRingBytes : 0);
}

// The instances <NKC = 4, NU = 3 or 4> (13..16 known types with three or four unknowns) would spill a register on the
// deferred-C schedule (tools/kernel_regs.sh --x16): they are not built and keep the pair schedule.
constexpr bool rowpass_v2_defer_instance(int nkc, int nu) { return !(nkc == 4 && nu >= 3); }
constexpr int kDeferWaves = 4;  // the deferred-C schedule is written for four waves: 193..256 samples

bool rowpass_v2_byte_images_wanted(int S, bool x16, double max_count) {
    return x16 && rowpass_v2_counts_fit_bytes(max_count) && (S + 63) / 64 == kDeferWaves;  // (one unknown fits at every step count)
}

RowpassV2Plan rowpass_v2_plan(const ShapeKey& k, int n_iter2) {
    RowpassV2Plan g;
    const int S = k.S, n_u = k.n_u, NW = (S + 63) / 64;
    g.N = k.N, g.S = S, g.n_c = k.n_c, g.SD = k.SD, g.nd = k.nd, g.n_iter2 = n_iter2;
    g.nkc = (k.n_c + 3) / 4, g.nu = n_u, g.xs = k.x16;
    if (k.N < 1 || S < 2 || S > 512 || k.n_c < 0 || k.n_c > 16 || n_u < 1 || n_u > 4 || n_iter2 < 0 || k.nd < 1 || k.nd > 2 ||
        k.SD < NW * 64 || (k.SD & 7) != 0)
        return g;
    // up to 256 samples: two workgroups per CU within 160 KB; beyond: one workgroup of up to eight waves
    g.nw = NW, g.maxw = NW <= 4 ? 4 : 8;
    const size_t wg_cap = (size_t)(g.maxw == 4 ? 80 : 160) * 1024, cu_lds = (size_t)160 * 1024;
    // (checked on the V form: the X16 form's tile is smaller)
    if (rowpass_v2_lds_bytes(S, n_u, n_iter2, false) > wg_cap) return g;
    // workgroups per CU the grid is sized for, two waves per SIMD: NW = 5..8 -> 1, 4 -> 2, 3 -> 2, 2 -> 4, 1 -> 8
    const int per_cu = per_cu_knob("DMF_V2_PER_CU", NW > 4 ? 1 : 8 / NW);
    // The pair schedule applies to the X16 form with two to four waves, when the grid's workgroups per CU still fit the
    // CU's 160 KB of LDS with two tile / slot / ubuf sets each: so at two waves (four workgroups per CU) up to three
    // unknowns -- four need 44 KB per workgroup, and only three such workgroups would fit a CU: the grid would run in two rounds.
    g.pair = k.rowpass_pair && k.x16 && NW >= 2 && NW <= 4 &&
             rowpass_v2_lds_bytes(S, n_u, n_iter2, true, true) * (size_t)per_cu <= cu_lds;
    // The deferred-C schedule applies to the pair schedule at four waves when every x fits a byte and two workgroups, each
    // with the x ring and six ubuf sets, still fit the CU's 160 KB (a workgroup's share counted in whole 2 KB pieces, the
    // coarsest the LDS is handed out in): 70 848 B at n_u = 4 and 20 inner steps -- the ring of three pairs costs 24 KB,
    // the x tiles it replaces 18 KB.
    g.defer_c = g.pair && k.rowpass_defer_c && k.x_byte && NW == kDeferWaves && rowpass_v2_defer_instance(g.nkc, n_u) &&
                ((rowpass_v2_lds_bytes(S, n_u, n_iter2, true, true, true) + 2047) & ~(size_t)2047) * (size_t)per_cu <= cu_lds;
    // The byte form is the same schedule with 1 KB count tiles instead of 2.25 KB (60 KB at that shape, so it fits wherever
    // the u16 form does), read from the images every such problem carries (rowpass_v2_byte_images_wanted).
    g.bytes = g.defer_c && k.rowpass_bytes;
    g.lds = rowpass_v2_lds_bytes(S, n_u, n_iter2, g.xs, g.pair, g.defer_c, g.bytes);
    g.raise = g.lds > 48 * 1024;
    const int64_t nblk = (k.N + 15) / 16, full = 256 * per_cu;
    g.grid = (int)(nblk < full ? nblk : full);
    g.blocks_per_wg = (nblk + g.grid - 1) / g.grid;
    g.supported = g.lds <= wg_cap;
    return g;
}

hipError_t launch_rowpass_v2(const ProblemView& p, const IterateView& it, int n_iter2, const UScratch& scratch,
                             const RowpassV2Plan& g, hipStream_t st) {
    if (!g.supported || g.N != p.N || g.S != p.S || g.n_c != p.n_c || g.nu != it.n_u || g.SD != p.SD || g.nd != p.ND ||
        g.n_iter2 != n_iter2 || g.xs != (p.X16 != nullptr) || (g.bytes && (p.X8 == nullptr || p.D8 == nullptr)))
        return hipErrorInvalidValue;
    return dispatch_int<0, 4>(g.nkc, [&](auto nkc) {
        return dispatch_bool(g.xs, [&](auto xs) {
            return dispatch_int<1, 4>(g.nu, [&](auto nu) {
                const auto launch = [&](auto maxw, auto pair_t, auto defer_t, auto bytes_t) {
                    constexpr int MAXW = decltype(maxw)::value;
                    constexpr bool PAIR = decltype(pair_t)::value, DEFER_C = decltype(defer_t)::value, BYTES = decltype(bytes_t)::value;
                    constexpr auto kernel = k_rowpass_v2<decltype(nkc)::value, decltype(nu)::value, MAXW, decltype(xs)::value, PAIR, DEFER_C, BYTES>;
                    // (a plan that names an instance that is not built ends up here on another one)
                    if (g.maxw != MAXW || g.pair != PAIR || g.defer_c != DEFER_C || g.bytes != BYTES) return hipErrorInvalidValue;
                    if (g.raise) {
                        const hipError_t e = raise_dynamic_lds<kernel>((size_t)(MAXW == 4 ? 80 : 160) * 1024);
                        if (e != hipSuccess) return e;
                    }
                    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(g.nw * 64), g.lds, st, p.V, BYTES ? reinterpret_cast<const unsigned short*>(p.D8) : p.D16,
                                       BYTES ? reinterpret_cast<const unsigned short*>(p.X8) : p.X16, p.SD, p.Rtp, it.alpha,
                                       it.u, it.u_prev, it.state, p.N, p.S, p.n_c, n_iter2, it.mode, p.ND, scratch.slab,
                                       scratch.u2_partials
#ifdef DMF_STAMPS
                                       , (unsigned long long*)nullptr
#endif
                                       );
                    return hipGetLastError();
                };
                // The instances that exist: eight waves run one block at a time; the pair schedule is an X16 form; its
                // deferred-C forms are built where rowpass_v2_defer_instance says so.
                constexpr std::integral_constant<int, 4> w4{};
                constexpr std::true_type yes{};
                constexpr std::false_type no{};
                if (g.maxw == 8) return launch(std::integral_constant<int, 8>{}, no, no, no);
                if constexpr (decltype(xs)::value) {
                    if constexpr (rowpass_v2_defer_instance(decltype(nkc)::value, decltype(nu)::value)) {
                        if (g.bytes) return launch(w4, yes, yes, yes);
                        if (g.defer_c) return launch(w4, yes, yes, no);
                    }
                    if (g.pair) return launch(w4, yes, no, no);
                }
                return launch(w4, no, no, no);
            });
        });
    });
}

}  // namespace dmf
