// Internal declarations shared by the kernel translation units and the C-ABI layer.
// gfx950 only; no portability macros on purpose.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dmf_select.h"

namespace dmf {

// Device-resident scalar state of one solve (demethify/deconvolution.py:192-204 and the
// scalars carried across outer iterations, :206-221).
struct SolverState {
    double a1;         // momentum scalar of the u phase (:192, :83-84)
    double a2;         // momentum scalar of the alpha phase (:193, :95-96)
    double l_w;        // ||alpha[-n_u:]||_F^2 * d (:198, :216)
    double l_w_prev;   // l_w_ (:199, :89)
    double l_h;        // ||R||_F^2 * d (:201, :212)
    double l_h_prev;   // l_h_ (:202, :101)
    double dsq;        // d = max(D)^2 (:197)
    double rt_norm2;   // ||R_trunc||_F^2 (constant part of ||R||_F^2)
    double u_norm2;    // ||u||_F^2 of the current u
    double cf;         // current cost (:204, :218)
    double cf_prev;    // cf_0 (:207)
    double tol;        // stop threshold of the running step() call (:220)
    long long iters;   // outer iterations completed
    double band;       // 1: |cf - cf_0| < tol stops; > 1: |cf - cf_0| < band x tol pauses for the host's confirmation
    int done;          // 1 once |cf - cf_0| < tol was met, 2 while paused: later launches are no-ops
    int arrive;        // workgroups of the alpha kernel that have finished this outer iteration (the last one closes it)
    // Momentum rows (dmf_solver_step).  The sequence a_t of deconvolution.py:83-84 / :95-96 does not depend on the data, so
    // the host runs it ahead for the iterations it enqueues and uploads one row per outer iteration:
    //   { a1 after the iteration, a2 after it, (a_{t-1} - 1) / a_t for the u phase [mom_n], the same for the alpha phase }
    // -- no kernel then spends its first microseconds on a chain of n_iter2 square roots and divisions (the row pass's
    // thread 0, every wave of the alpha kernel and the closing step each did).  Row mom_i is the current iteration's
    // (the closing step moves on); valid for launches with n_iter2 == mom_n only.
    const double* mom;
    int mom_stride, mom_rows, mom_i, mom_n;
};

// the row of momentum ratios of the current outer iteration, or nullptr (the kernel then runs the recurrence itself)
__device__ __forceinline__ const double* momentum_row(const SolverState* __restrict__ state, int n_iter2) {
    return (state->mom != nullptr && state->mom_n == n_iter2 && state->mom_i < state->mom_rows)
               ? state->mom + (int64_t)state->mom_i * state->mom_stride
               : nullptr;
}

// Packed upper triangle, column-major over (k <= l): independent of the matrix size.
__host__ __device__ inline int tri(int k, int l) { return l * (l + 1) / 2 + k; }

constexpr int kMaxK = 64;          // largest K = n_c + n_u the alpha kernels are built for
constexpr int kGramChunk = 16;     // accumulators per generic Gram job
constexpr int kRowsPerBlockU = 64; // rows handled by one block of the u-phase kernels

struct GramJobTable {              // device arrays, one entry per accumulator
    const short* k_idx;            // extended index (0..K; K means "the sample column v")
    const short* l_idx;
    const int* dst_row;            // destination row in the solver's packed Gram buffer
    int count;
};

// One percentile of numpy's "linear" method over n sorted values: lerp(sorted[k_prev], sorted[k_next], gamma)
struct PercentilePlan {
    long long k_prev, k_next;
    double gamma;
    int from_top;  // set by the launcher: which register tail of k_percentile_tails holds the two values
    int pad;
};

// ---- views: what the launch wrappers take instead of lists of pointers and sizes (plain structs, passed by const&)
// The device arrays of a problem as the kernels read them (dmf_problem::view()).  D16 / X16 / Dt8 null: no integer copies
// (counts as u16 [N16][SD], methylated read counts in the same layout, balanced 8-bit digit planes: see below).
struct ProblemView {
    const double* V = nullptr;
    const double* D = nullptr;
    const unsigned short* D16 = nullptr;
    const unsigned short* X16 = nullptr;
    const unsigned char* X8 = nullptr;  // byte images of X16 / D16 for the deferred-C row pass (dmf_rowpass_image.h); null: none
    const unsigned char* D8 = nullptr;
    const signed char* Dt8 = nullptr;
    int64_t plane_stride = 0;
    int SD = 0, ND = 0;
    const double* Rt = nullptr;
    const double* Rtp = nullptr;  // R_trunc with rows zero-padded to a multiple of 4 doubles
    int64_t N = 0;
    int S = 0, n_c = 0;
    unsigned v_align() const { return (unsigned)(reinterpret_cast<uintptr_t>(V) & 15); }
    // rows [first, first + count) through the f64 arrays alone (the integer copies are laid out in blocks of rows)
    ProblemView rows(int64_t first, int64_t count) const {
        ProblemView r;
        r.V = V + first * S;
        r.D = D + first * S;
        r.Rt = Rt ? Rt + first * n_c : nullptr;
        r.Rtp = Rtp ? Rtp + first * ((n_c + 3) / 4 * 4) : nullptr;
        r.N = count;
        r.S = S;
        r.n_c = n_c;
        return r;
    }
};

// The iterate of a solver and its device state (dmf_solver::iterate()).
struct IterateView {
    double* u = nullptr;
    double* u_prev = nullptr;
    const double* alpha = nullptr;
    SolverState* state = nullptr;
    int n_u = 0, mode = 0;
    IterateView rows(int64_t first) const {  // the same iterate from row `first` on
        IterateView r = *this;
        r.u = u + first * n_u;
        r.u_prev = u_prev + first * n_u;
        return r;
    }
};

// What the alpha phase of a solver works on (dmf_solver::alpha_view()): the packed Gram buffer gb[(K+1)(K+2)/2][S], the
// iterate, the per-sample known-block masses of a purity-constrained solve (null otherwise) and `partials`, which holds
// 2 * (ceil(S / 64) + S) doubles.
struct AlphaView {
    const double* gb = nullptr;
    double* alpha = nullptr;
    double* alpha_prev = nullptr;
    const double* purity = nullptr;
    SolverState* state = nullptr;
    double* partials = nullptr;
    int S = 0, n_c = 0, n_u = 0;
};

// Per-solver scratch that some u phases write: c_i / M_i per row and the momentum coefficients of the split u phase, the
// b_u slab and the per-workgroup ||u||^2 shares of the one-launch row passes.
struct UScratch {
    double* cm = nullptr;
    double* beta = nullptr;
    double* slab = nullptr;
    double* u2_partials = nullptr;
};

// ---- launch wrappers (dmf_kernels_*.hip) ---------------------------------------------------
// All wrappers enqueue on `st` and return the hipGetLastError() of their launches.  Where a wrapper takes (u, n_u) beside
// a ProblemView, they are the row features next to R_trunc: a solver's u, or none / R_trunc itself for the known block.

hipError_t launch_convert_counts(const long long* src, double* dst, int64_t n, hipStream_t st);
// max over a f64 array -> *out (device); scratch needs >= 1024 doubles
hipError_t launch_max_f64(const double* x, int64_t n, double* scratch, double* out, hipStream_t st);
// max |x - (double)(float)x| -> *out: 0 iff every element is exactly representable in f32
hipError_t launch_f32_residual_max(const double* x, int64_t n, double* scratch, double* out, hipStream_t st);
// max(x) if every element is a non-negative integer, +inf otherwise -> *out
hipError_t launch_int_count_max(const double* x, int64_t n, double* scratch, double* out, hipStream_t st);
// 0 if every element lies in [0, 1], 1 otherwise -> *out
hipError_t launch_unit_range_check(const double* x, int64_t n, double* scratch, double* out, hipStream_t st);
// sum of squares -> *out (device)
hipError_t launch_sumsq_f64(const double* x, int64_t n, double* scratch, double* out,
                            const int* done_flag, hipStream_t st);
hipError_t launch_pad_rows(const double* src, double* dst, int64_t n_rows, int width_src, int width_dst,
                           hipStream_t st);
hipError_t launch_index_range_check(const long long* idx, int64_t n_idx, int64_t n_src, unsigned int* flag, hipStream_t st);
hipError_t launch_gather_rows(const double* src, double* dst, const long long* idx, int64_t n_idx,
                              int64_t width, hipStream_t st);

// direct weighted cost: *out = sum d (v - [Rt|u] alpha)^2 by the kernel that `plan` names (dmf_select.h; the plan of
// cost_key(p, n_u, level), or hipErrorInvalidValue comes back); scratch: kCostPartials doubles.  The column-resident
// kernels keep the lane's alpha column in registers and read Rtp (the padded R_trunc copy) and, where the plan says so,
// D16 (u16 counts, row stride SD) instead of D.
inline CostKey cost_key(const ProblemView& p, int n_u, int level) {
    CostKey k;
    k.S = p.S, k.n_c = p.n_c, k.n_u = n_u;
    k.d16 = p.D16 != nullptr;
    k.SD = p.SD;
    k.v_align = p.v_align();
    k.rtp_present = p.Rtp != nullptr;
    k.level = level;
    return k;
}
hipError_t launch_cost_plan(const CostPlan& plan, const ProblemView& p, const double* u, const double* alpha, int n_u,
                            double* scratch, double* out, hipStream_t st);
int vdv_cols_grid(int64_t N);
hipError_t launch_vdv_cols(const ProblemView& p, double* slab, double* out, hipStream_t st);

// What a Gram launcher ran, as text: the kernel, its template arguments and the number of launches (dmf_solver_gram
// reports it).  Written by the launcher itself, next to the launch.
struct GramRan {
    char text[192] = "";
};

// generic weighted Gram accumulation over the extended row vector x = (Rt, u, v)
hipError_t launch_gram(const ProblemView& p, const double* u, int n_u, GramJobTable jobs, double* slab, int64_t slab_doubles,
                       double* gb, const int* done_flag, hipStream_t st, GramRan* ran = nullptr);
int64_t gram_slab_doubles(int64_t N, int S, int n_jobs);
hipError_t launch_gram_reduce(const double* slab, int ny, int n_jobs, int S, const int* dst_row,
                              double* gb, const int* done_flag, hipStream_t st);
// shape-specialised one-pass Gram of the u-dependent entries (n_u <= 8, n_c <= 16); slab in job order.
// Rtp = R_trunc with rows zero-padded to a multiple of 4 doubles (dmf_problem::Rtp).
bool gram_u_supported(int n_c, int n_u);
int64_t gram_u_slab_doubles(int64_t N, int S, int n_c, int n_u);
hipError_t launch_gram_u(const ProblemView& p, const double* u, int n_u, double* slab, const int* done_flag, int* ny_out,
                         hipStream_t st, GramRan* ran = nullptr);

// ---- what the first-generation FP64 row kernels launch for a shape.  Each launcher below computes ONE such plan and
// launches from it; describe_u_phase (dmf_select.h: dmf_u_phase_describe) prints the same plan, so the text cannot say
// anything else than what runs.  Pure host functions of the shape -- no pointers, no context.
struct RowLaunch {
    bool supported = false;     // false: the launcher answers hipErrorInvalidValue
    int nw = 0;                 // waves per workgroup (k_rowpass_fused: column groups; 3 nw waves run)
    int grid = 0;               // workgroups
    size_t lds = 0;             // dynamic LDS bytes
    bool raise = false;         // the launcher raises the kernel's dynamic-LDS limit first (more than 48 KB)
    int64_t blocks_per_wg = 0;  // the largest number of row blocks any workgroup takes (workgroup 0's)
};
struct UPhaseMfmaPlan : RowLaunch {  // k_u_phase_mfma<NKC,NU,VEC,D16T>; row block = 16 rows
    int nkc = 0, nu = 0;
    bool vec = false, d16 = false;
    bool split = false;  // cm_out given: c_i / M_i per row go out, k_u_inner_rows runs the inner steps
};
// has_d16 / SD: the problem carries the u16 copy of its counts, and its padded row length
UPhaseMfmaPlan u_phase_mfma_plan(int64_t N, int S, int n_c, int n_u, int n_iter2, bool has_d16, int SD, bool split);
struct RowpassFusedPlan : RowLaunch {  // k_rowpass_fused<NKC,NU>; N = the whole 16-row blocks (the caller runs the tail)
    int nkc = 0, nu = 0;
};
RowpassFusedPlan rowpass_fused_plan(int64_t N, int S, int n_c, int n_u, int n_iter2);
struct UPhaseBigPlan : RowLaunch {  // k_u_phase_big<NKC,GS>; row block = 16 rows
    int nkc = 0, gs = 16, n_u = 0;
};
UPhaseBigPlan u_phase_big_plan(int64_t N, int S, int n_c, int n_u, int n_iter2);
struct UPhaseGramPlan : RowLaunch {  // k_u_phase_gram<NU>; row block = kRowsPerBlockU rows, one per workgroup
    int nu = 0;
    bool alpha_in_lds = false;
};
UPhaseGramPlan u_phase_gram_plan(int64_t N, int S, int n_c, int n_u);
struct UStepDirectPlan : RowLaunch {  // k_u_step_direct, one launch per inner step; row block = 4 rows (one per wave)
    int n_u = 0;
};
UStepDirectPlan u_step_direct_plan(int64_t N, int S, int n_c, int n_u);
// The second-generation row pass (dmf_kernels_rowpass2.hip): the same contract, from the solver's ShapeKey -- the plan
// reads N, S, n_c, n_u, nd, SD, x16, x_byte and the three rowpass_* switches.  supported is checked on the V form's LDS
// (the X16 forms need less); lds is the launched form's.
enum class RowpassSchedule { One, Pair, Deferred, Bytes };  // one block per barrier cycle / two / phase C deferred / ... on bytes
constexpr int kRowpassSchedules = 4;
struct RowpassV2Plan : RowLaunch {  // k_rowpass_v2<NKC,NU,MAXW,XS,PAIR,DEFER_C,BYTES>; row block = 16 rows
    int nkc = 0, nu = 0, maxw = 4;
    bool xs = false, pair = false, defer_c = false, bytes = false;
    int64_t N = 0;  // the problem and step count it was made for (the launcher takes no other)
    int S = 0, n_c = 0, SD = 0, nd = 0, n_iter2 = 0;
    RowpassSchedule schedule() const { return RowpassSchedule(pair + defer_c + bytes); }  // (bytes implies defer_c implies pair)
};
RowpassV2Plan rowpass_v2_plan(const ShapeKey& k, int n_iter2);
// "k_u_phase_mfma<2,3,vec,d16> split nw=2 grid=512 lds=6912 raise=0 blocks/wg=3"; the row pass's plan goes behind its
// rowpass= text: "maxw=4 bytes nw=4 grid=512 lds=61440 raise=1 blocks/wg=123"
int describe_row_launch(const UPhaseMfmaPlan& g, char* buf, size_t cap);
int describe_row_launch(const RowpassFusedPlan& g, char* buf, size_t cap);
int describe_row_launch(const UPhaseBigPlan& g, char* buf, size_t cap);
int describe_row_launch(const UPhaseGramPlan& g, char* buf, size_t cap);
int describe_row_launch(const UStepDirectPlan& g, char* buf, size_t cap);
int describe_row_launch(const RowpassV2Plan& g, char* buf, size_t cap);

// u phase, Gram form (n_u <= 8): all n_iter2 inner iterations in one launch
hipError_t launch_u_phase_gram(const ProblemView& p, const IterateView& it, int n_iter2, hipStream_t st);
bool u_phase_gram_supported(int S, int n_c, int n_u);
// u phase on the FP64 matrix cores (n_u <= 8, n_c <= 16, S <= 512); reads the padded Rtp, and D16 where there is one
bool u_phase_mfma_supported(int S, int n_c, int n_u);
hipError_t launch_u_phase_mfma(const ProblemView& p, const IterateView& it, int n_iter2, hipStream_t st);
// the same kernel; cm_out: null, or where its split mode leaves the per-row c_i / M_i instead of running the inner steps
hipError_t launch_u_phase_mfma_impl(const ProblemView& p, const IterateView& it, int n_iter2, double* cm_out, hipStream_t st);
// fused row pass: u phase + u-dependent Gram slab + ||u||^2 / l_h in one read of V and D
// (S % 4 == 0, S <= 256, n_c <= 16, n_u <= 8, accumulators <= 80, counts exact in f32);
// grid_out = workgroups launched; the slab (scratch.slab, with scratch.u2_partials) holds 2 rows per workgroup
bool rowpass_fused_supported(int S, int n_c, int n_u);
int rowpass_fused_grid(int64_t N, int S);
int64_t rowpass_fused_slab_doubles(int64_t N, int S, int n_c, int n_u);
hipError_t launch_rowpass_fused(const ProblemView& p, const IterateView& it, int n_iter2, const UScratch& scratch,
                                int* grid_out, hipStream_t st);
// sum of the fused kernel's per-workgroup ||u||^2 shares -> state->u_norm2 and l_h (deconvolution.py:212)
hipError_t launch_finish_u_norm(const double* u2_partials, int n, SolverState* state, hipStream_t st);
// u phase, schedule-faithful fallback: ONE inner iteration (index t) per launch, from (it.u, it.u_prev) into u_next
hipError_t launch_u_step_direct(const ProblemView& p, const IterateView& it, double* u_next, int t, hipStream_t st);
bool u_step_direct_supported(int S, int n_c, int n_u);

// alpha phase: the n_iter2 inner steps (Frank-Wolfe steps for the two purity kinds) with the kernel the plan names
// (dmf_select.h), then the close of the outer iteration; hipErrorInvalidValue where `kind` does not take K = n_c + n_u
hipError_t launch_alpha(AlphaKind kind, const AlphaView& a, int n_iter2, hipStream_t st);
hipError_t launch_set_lh(SolverState* state, hipStream_t st);
hipError_t launch_project_simplex(const double* X, double* out, int K, int S, double z,
                                  hipStream_t st);
hipError_t launch_scatter_known_block(const double* gb_known, double* gb, int n_c, int K, int S,
                                      hipStream_t st);
hipError_t launch_init_state(SolverState* state, const double* consts, const double* alpha,
                             int S, int n_c, int n_u, hipStream_t st);

// the same u phase in two launches for many inner steps: c_i / M_i per row to `cm`, then inner iterations with
// every lane busy; scratch.cm holds u_phase_split_cm_doubles(N, n_u) doubles, scratch.beta n_iter2 doubles
int64_t u_phase_split_cm_doubles(int64_t N, int n_u);
hipError_t launch_u_phase_split(const ProblemView& p, const IterateView& it, int n_iter2, const UScratch& scratch,
                                hipStream_t st);

// split u phase whose producer runs M_i on the integer matrix cores (dmf_kernels_cm_i8.hip): n_u <= 16, 2 <= S <= 2048
// (panels of 256 samples), u16 counts with ND digit planes, alpha in [0, 1]; v_align = ProblemView::v_align()
bool cm_i8_supported(unsigned v_align, int S, int n_c, int n_u, int ND, int SD);
// What launch_cm_i8 launches for a shape: panels of up to 256 samples, per panel one or more launches that each hold
// `tpl` 16-pair tiles of M_i in the LDS (the last one what is left) and one 16-unknown tile of c.  The launcher dispatches
// on it and describe_cm_i8_plan prints it (dmf_u_phase_describe, dmf_solver_row_moments).  Pure host code.
struct CmI8Launch {  // launch li of a panel
    int mt0 = 0, mt1 = 0;         // pair tiles [mt0, mt1)
    int c_tile = 0, c_store = 0;  // the c tile it computes, and whether it stores it
    size_t lds = 0;               // dynamic LDS bytes
    int grid = 0;                 // workgroups of 8 waves, a wave per 32-row block at a time
    int64_t blocks_per_wave = 0;  // the largest number of 32-row blocks any wave takes
};
struct CmI8Panel {
    int col0 = 0, Sp = 0;  // samples col0 .. col0 + Sp - 1
    bool s4 = false;       // template argument S4: the plain 16-byte strip loads
    int ncgx = 2;          // template argument NCGX: 2 column groups of 64 samples, 4 beyond 128 samples
    int tpl = 0;           // pair tiles per launch
    int n_launch = 0;
    CmI8Launch first, last;  // the first and the last launch (the ones between equal the first but for their tiles)
};
constexpr int kCmMaxPanels = 8;  // 2048 samples
struct CmI8Plan {
    bool supported = false;
    int64_t N = 0;
    int S = 0, n_c = 0, n_u = 0;
    int nkc = 0, nd = 1;    // template arguments NKC (12 = kCmNkcWide: more than 16 known types) and ND
    int nmt = 0, n_ct = 0;  // 16-pair tiles of M_i, 16-unknown tiles of c
    int n_panels = 0;
    CmI8Panel panel[kCmMaxPanels];
};
CmI8Plan cm_i8_plan(int64_t N, int S, int n_c, int n_u, int ND);
CmI8Launch cm_i8_launch_of(const CmI8Plan& g, int panel, int li);
// "panels=2 tiles=10 | col0=0 sp=256 k_cm_i8<1,2,4,s4> tpl=5 launches=2 ctiles=2 lds=.. grid=.. blocks/wave=.. | col0=256 .."
int describe_cm_i8_plan(const CmI8Plan& g, char* buf, size_t cap);
struct CmRan {  // what a producer of the split u phase ran, as text (dmf_solver_row_moments)
    char text[2048] = "";
};
hipError_t launch_cm_i8(const ProblemView& p, const IterateView& it, double* cm, hipStream_t st, CmRan* ran = nullptr);
hipError_t launch_u_phase_split_i8(const ProblemView& p, const IterateView& it, int n_iter2, const UScratch& scratch,
                                   hipStream_t st);

// ... and with the inner iterations fused with the b_u stream of the integer Gram route (k_inner_bu): scratch.slab holds
// u_inner_bu_grid(N, S) x n_u x S doubles, scratch.u2_partials one double per workgroup (their count comes back in grid_out)
bool u_inner_bu_supported(unsigned v_align, int S, int SD, int n_u, int n_iter2);
int u_inner_bu_grid(int64_t N, int S);
hipError_t launch_u_phase_split_i8_bu(const ProblemView& p, const IterateView& it, int n_iter2, const UScratch& scratch,
                                      int* grid_out, hipStream_t st);

// u phase for 9 <= n_u <= 26 unknown types on the matrix cores (dmf_kernels_rowpass_big.hip); Rtp = padded R_trunc
bool u_phase_big_supported(int S, int n_c, int n_u, int n_iter2);
hipError_t launch_u_phase_big(const ProblemView& p, const IterateView& it, int n_iter2, hipStream_t st);

// any-shape Gram accumulation on the matrix cores (dmf_kernels_gram_mfma.hip): jobs [0, n_dense) have l < K,
// the rest are the "v" column; the slab ([ny][count][S]) is then summed by launch_gram_reduce
hipError_t launch_gram_mfma(const ProblemView& p, const double* u, int n_u, GramJobTable jobs, int n_dense, double* slab,
                            int64_t slab_doubles, const int* done_flag, int* ny_out, hipStream_t st, GramRan* ran = nullptr);
int64_t gram_mfma_slab_doubles(int64_t N, int S, int n_jobs);

// ---- second-generation row pass (dmf_kernels_rowpass2.hip) + integer-matrix-core Gram (dmf_kernels_gram_i8.hip)
// counts as u16 (D16[N16][SD], zero padded: N16 = N rounded up to 16, SD = S rounded up to 64) and as balanced 8-bit
// digit planes in the MFMA B layout (Dt8[ND][ceil(N/32)][SD/32][32][32]); ND = 1 (d <= 127) or 2 (d <= 32639)
// X16 (optional, D16's layout): the methylated read counts x = rint(v d), when every element is exact (see
// launch_build_counts_int); the gather carries it along (src_x16 / X16 null: no copy) and sums the gathered x into *xsum_out
hipError_t launch_gather_counts_int(const unsigned short* src16, const unsigned short* src_x16, const long long* idx,
                                    int64_t n_idx, int SD, int ND, unsigned short* D16, unsigned short* X16, int64_t N16,
                                    signed char* Dt8, int64_t plane_stride, unsigned int* max_out,
                                    unsigned long long* xsum_out, hipStream_t st);
// X16 != null: also x = rint(v d) per element, accepted when 0 <= x <= d and |fma(v, d, -x)| <= kX16MaxDev max(x, 1)
// (d = 0: x = 0 whatever v is); x_stats[3] (zeroed here) <- { elements that fail, bits of the largest |fma(v, d, -x)| /
// max(x, 1), sum of x }
constexpr double kX16MaxDev = 8.0 * 0x1p-53;
hipError_t launch_build_counts_int(const double* D, const double* V, int64_t N, int S, int ND, unsigned short* D16,
                                   unsigned short* X16, int64_t N16, int SD, signed char* Dt8, int64_t plane_stride,
                                   unsigned long long* x_stats, hipStream_t st);
// the digit planes alone, from a D16 that is already in place (the second half of the two launchers above)
hipError_t launch_build_dt8(const unsigned short* D16, int64_t N, int SD, int ND, signed char* Dt8, int64_t plane_stride,
                            hipStream_t st);
// hold-out masks (dmf_kernels_mask.hip).  bits: the N x S train mask, bit-packed row-major, ceil(S / 8) bytes per row,
// sample s = bit (s & 7) of byte (s >> 3), 1 = kept.  dst = src where kept, 0 where held out, for V and D and -- src16 not
// null -- D16 and X16 (srcX / dstX both or neither); W16 (D16's layout, zero padded) <- 1 where held out.  stats[3] (zeroed
// here) <- { bits of max(kept counts, 0) as a double, sum of the kept x, number of held-out elements }
hipError_t launch_mask_problem(const double* srcV, const double* srcD, const unsigned short* src16,
                               const unsigned short* srcX, const unsigned char* bits, double* dstV, double* dstD,
                               unsigned short* dst16, unsigned short* dstX, unsigned short* W16, int64_t N, int64_t N16, int S,
                               int SD, unsigned long long* stats, hipStream_t st);
// W[N][S] <- 1.0 where held out, 0.0 where kept
hipError_t launch_holdout_weights_f64(const unsigned char* bits, double* W, int64_t N, int S, hipStream_t st);
// the mask draw (dmf_kernels_rng.hip): bits <- `np.random.rand(N, S) < fraction` of the MT19937 state (key_io, pos), packed as
// above with every byte written and the padding bits zero; threshold = ceil(fraction 2^53) (0 .. 2^53).  key_io[624] (device)
// <- the key as of the last regeneration; result[2] <- { number of ones, position after the last word used }.  pos in
// [0, 624], 624 = regenerate first.  One persistent workgroup.
constexpr int64_t kMaskDrawMaxS = ((int64_t)1 << 31) - 1, kMaskDrawMaxElements = (int64_t)1 << 60;
hipError_t launch_mask_draw(unsigned int* key_io, int pos, int64_t N, int64_t S, unsigned long long threshold,
                            unsigned char* bits, unsigned long long* result, hipStream_t st);
// ... cut into segments of `c` 624-word blocks on numpy's grid, one workgroup each (block 0 = the caller's key, used from word
// pos).  The plan is a function of the shape alone: `segments` of `blocks_per_segment` blocks cover the 2 N S + 624 words a
// draw can reach; one segment means launch_mask_draw.  Measured (profiles/r14_mask_draw_segments.txt): segments of about 64
// blocks are the fastest cut while there are workgroups to give (shorter ones cost more in jumps than they save in
// regenerations), and a round of jumps costs what some 200 regenerations do, so a draw is cut from 512 blocks on.
constexpr int64_t kMaskDrawMaxSegments = 1024, kMaskDrawMinBlocks = 64, kMaskDrawCutFrom = 512;
inline int64_t mask_draw_blocks(int64_t N, int64_t S) { return (2 * N * S + 624 + 623) / 624; }
inline void mask_draw_plan(int64_t N, int64_t S, int64_t* segments, int64_t* blocks_per_segment) {
    const int64_t blocks = mask_draw_blocks(N, S), by_length = blocks / kMaskDrawMinBlocks;
    const int64_t w = blocks < kMaskDrawCutFrom ? 1 : by_length > kMaskDrawMaxSegments ? kMaskDrawMaxSegments : by_length;
    *segments = w, *blocks_per_segment = (blocks + w - 1) / w;
}
// keys[W][624] (device), W = (pos + 2 N S - 1) / 624 / c + 1 <= kMaskDrawMaxSegments: row 0 the caller's key, row s >= 1 the key
// of block c s - 1.  key_out[624] <- the key as of the last regeneration, result[1] <- the position after the last word used,
// counts[W] <- the ones per segment (result[0] is not written: the caller adds them up).  Every byte of bits is written, by
// the one workgroup whose segment holds the byte's first element.
hipError_t launch_mask_draw_segments(const unsigned int* keys, unsigned int* key_out, int pos, int64_t c, int64_t N, int64_t S,
                                     unsigned long long threshold, unsigned char* bits, unsigned long long* result,
                                     unsigned long long* counts, hipStream_t st);
// One jump per job, a workgroup each: row dst of keys[..][624] (device) <- row src carried forward by the jump polynomial with
// the non-zero terms terms[first .. first + n_terms) (dmf_mt_jump.h; exponents <= 19937).  The jobs of one launch write rows
// that none of them reads.
struct MtJumpJob {
    int src, dst, first, n_terms;
};
hipError_t launch_mt_jump(unsigned int* keys, const MtJumpJob* jobs, int64_t n_jobs, const unsigned short* terms,
                          hipStream_t st);
// u phase + b_u slab (scratch.slab: [plan.grid][n_u][S] doubles) + per-workgroup ||u||^2 shares in one read of V (f64)
// and D16 -- or, on the plan's X16 form, of X16 and D16 (V is not read) or of their byte images X8 / D8.  Every schedule of
// a shape gives the same results bit for bit.  `plan` is rowpass_v2_plan() of this problem, iterate and n_iter2, or
// hipErrorInvalidValue comes back: N, S, n_c, n_u, SD, ND and n_iter2 equal, X16 present iff plan.xs, X8 / D8 if plan.bytes.
hipError_t launch_rowpass_v2(const ProblemView& p, const IterateView& it, int n_iter2, const UScratch& scratch,
                             const RowpassV2Plan& plan, hipStream_t st);
// the byte images X8 / D8 ([N16 / 16][SD / 64][1024], dmf_rowpass_image.h) of X16 / D16 ([N16][SD], every element <= 255)
hipError_t launch_build_rowpass_images(const unsigned short* X16, const unsigned short* D16, int64_t N16, int SD,
                                       unsigned char* X8, unsigned char* D8, hipStream_t st);
// ShapeKey::x_byte: every count of the problem, so every x, fits a byte
inline bool rowpass_v2_counts_fit_bytes(double max_count) { return max_count <= 255.0; }
// a problem builds those images: true exactly where some plan of the problem (any n_c, n_u, n_iter2) can have `bytes` set
bool rowpass_v2_byte_images_wanted(int S, bool x16, double max_count);
bool gram_i8_supported(int n_c, int n_u, int ND, int64_t N, int SD);
// What launch_gram_i8 launches for a shape -- the one geometry result that the launcher dispatches on and that
// describe_gram_i8_plan prints (dmf_gram_i8_describe), so that the text cannot say anything else than what runs.
// n_u = 0: the known block (features = pairs of R_trunc columns).
struct GramI8Plan {
    bool supported = false;
    int xl = 1, nd = 1, ring = 8;  // template arguments of k_gram_i8_w8: DMA pieces of a block's row image, count digits, ring slots
    int nf = 0, launches = 0;      // features, launches of 64 features each
    int nsh = 0, ny = 0;           // workgroups per row range (128 samples each), row ranges: the grid is nsh * ny
    int64_t rows_per_wg = 0;       // rows of a range (a multiple of 32)
    int blocks = 0, last = 0;      // 32-row blocks of a full range, of the last range
    int tail = 0;                  // N % 32: rows of the ragged last block (0: none)
    bool xcd = false;              // ny % 8 == 0: the kernel maps the workgroups of a range onto one XCD
};
GramI8Plan gram_i8_plan(int64_t N, int SD, int n_c, int n_u, int ND);
// "k_gram_i8_w8<2,2,6> launches=3 nsh=16 ny=16 blocks=9 last=8 tail=27 xcd=1"
void describe_gram_i8_plan(const GramI8Plan& g, char* buf, size_t cap);
int64_t gram_i8_slab_words(int64_t N, int SD, int n_c, int n_u);  // i64 words of the slab
int64_t gram_i8_acc_words(int S, int n_c, int n_u);               // i64 words of the reduction scratch (zero-initialised)
// the known block of the packed Gram through the same kernels (features = pairs of R_trunc columns; n_u = 0)
bool gram_i8_known_supported(int n_c, int ND, int64_t N, int SD);
int64_t gram_i8_slab_words_nf(int64_t N, int SD, int nf);
int64_t gram_i8_acc_words_nf(int S, int nf, int n_bu);
// exact cross / uu Gram entries: features p = (feat_a[p], feat_b[p]) over x = (Rt, u), i64 slab [ny][2][slots][SD];
// Rtp = the padded R_trunc copy (rows of 4 ceil(n_c / 4) doubles); Rtp, u, Dt8 16-byte aligned, u allocated to a
// multiple of 16 bytes
hipError_t launch_gram_i8(const ProblemView& p, const double* u, int n_u, const short* feat_a, const short* feat_b, int NF,
                          long long* slab, int64_t slab_words, const int* done_flag, int* ny_out, hipStream_t st,
                          GramRan* ran = nullptr);
// b_u alone (for u phases that are kernels of their own): slab [n_slabs][n_u][S] doubles, n_u <= 20
int bu_cols_grid(int64_t N);
hipError_t launch_bu_cols(const ProblemView& p, const double* u, int n_u, double* slab, const int* done_flag,
                          int* n_slabs_out, hipStream_t st, bool* with_vdv = nullptr);
// gb rows of the u-dependent jobs from the i64 slab (jobs < NF) and the row pass's b_u slabs (jobs NF .. NF + n_u);
// acc_words: gram_i8_acc_words() i64 words, all zero before the first call (the kernels leave them zero again);
// u2_partials != null: the finish kernel also sums the row pass's ||u||^2 shares into state (u_norm2, l_h)
hipError_t launch_gram_v2_reduce(const long long* slab_i8, int ny, int NF, int SD, const double* slab_bu, int n_bu_slabs,
                                 int n_u, int S, long long* acc_words, const int* dst_row, double* gb, const int* done_flag,
                                 const double* u2_partials, int n_u2, SolverState* state, hipStream_t st);

// two percentiles over axis 0 of x[n][m] -> out0[m], out1[m] (out1 may be null); dmf_kernels_percentile.hip
hipError_t launch_percentile_pair(const double* x, int64_t n, int64_t m, PercentilePlan p0, PercentilePlan p1,
                                  double* out0, double* out1, hipStream_t st);
// the same with the NaNs of a column left out (np.nanpercentile): p0 / p1 are the plans for the full n, q0 / q1 the
// quantiles (percentile / 100) from which the kernels plan each column for its own count of numbers
hipError_t launch_nanpercentile_pair(const double* x, int64_t n, int64_t m, PercentilePlan p0, PercentilePlan p1, double q0,
                                     double q1, double* out0, double* out1, hipStream_t st);
int64_t percentile_max_replicates();

// wls_intercept for every sample at once (dmf_kernels_wls.hip).  launch_wls_moments: one pass over the rows for the first
// moments of R = [Rt | u] under the weights d and the target t = v (target_dv 0) or d v (1), read from (X16, D16) where the
// problem carries them, else from V and D; mom[2 K + 2][S] = { m_k, r_k, sw, st }, summed over wls_moments_grid(N) slabs in
// fixed order; slab holds wls_slab_doubles(N, S, K) doubles.  launch_nnls_intercept: Lawson-Hanson per sample on the dense
// part of a packed Gram gb and mom; out[K][S] for the samples with status 0 (1: not solved here, 2: weights sum to zero).
int wls_moments_grid(int64_t N);
int64_t wls_slab_doubles(int64_t N, int S, int K);
hipError_t launch_wls_moments(const ProblemView& p, const double* u, int n_u, int target_dv, double* slab, double* mom,
                              hipStream_t st);
hipError_t launch_nnls_intercept(const double* gb, const double* mom, int K, int S, double* out, int* status, hipStream_t st);

// The SVD initialiser (dmf_kernels_svd.hip; constrained_nndsvd / nndsvd_initialize, init_func.py:17-82) by the Gram route.
// Yres = max(V - Rt H1, 1e-8) (n_c = 0: V as it is) is formed on the fly from the f64 V, Rt and the device array H1[n_c][S].
// launch_svd_gram: C[S][S] = Yres^T Yres, exactly symmetric; slab holds svd_gram_slab_doubles(N, S) doubles, flags
// 2 svd_gram_grid(N, S) ints (per workgroup: negative, non-finite entries of V).  launch_svd_project: T[N][rank] = Yres Es
// with Es[S][rank] = the e_j / sigma_j columns, norms[2][rank] = per column sum max(t, 0)^2, sum max(-t, 0)^2; slab holds
// svd_project_slab_doubles(N, rank) doubles.  launch_svd_finish: T <- clip(cut(scale_j |t| or scale_j max(sign_j t, 0))),
// in place (sign 0: the absolute value).  Every result depends on the data and (N, S, rank) alone.
constexpr int kSvdMaxS = 512, kSvdMaxNc = 64, kSvdMaxRank = 64;
constexpr size_t kSvdMaxLds = 160 * 1024;  // k_svd_project's E / sigma columns, row tile and partial norms must fit a CU's LDS
size_t svd_project_lds_bytes(int S, int rank);
struct SvdColumns {
    double sign[kSvdMaxRank], scale[kSvdMaxRank];
};
bool svd_supported(int S, int n_c, int rank);
int svd_gram_grid(int64_t N, int S);
int64_t svd_gram_slab_doubles(int64_t N, int S);
hipError_t launch_svd_gram(const ProblemView& p, const double* H1, double* slab, int* flags, double* C, hipStream_t st);
int64_t svd_project_slab_doubles(int64_t N, int rank);
hipError_t launch_svd_project(const ProblemView& p, const double* H1, const double* Es, int rank, double* T, double* slab,
                              double* norms, hipStream_t st);
hipError_t launch_svd_finish(double* T, int64_t N, int rank, const SvdColumns& cols, hipStream_t st);

// Component matching (dmf_kernels_match.hip).  launch_match_gram: P[n_u][n_u] (device) = sum_j u[j][a] anchor[idx[j]][b] over
// the N rows of u, anchor n_anchor_rows x n_u, idx N int64 row indices or null (the identity); slab holds
// match_gram_slab_doubles(N, n_u) doubles, flags match_gram_grid(N, n_u) ints (per workgroup: indices outside
// [0, n_anchor_rows), which are not dereferenced -- P is then to be discarded).  P depends on the data and (N, n_u) alone.
// launch_copy_cols_permuted: dst[i][b] = u[i][cols.src[b]] (dst != u).  1 <= n_u <= kMaxK.
struct MatchColumns {
    int src[kMaxK];
};
int match_gram_grid(int64_t N, int n_u);
int64_t match_gram_slab_doubles(int64_t N, int n_u);
hipError_t launch_match_gram(const double* u, const double* anchor, const long long* idx, int64_t N, int64_t n_anchor_rows,
                             int n_u, double* slab, int* flags, double* P, hipStream_t st);
hipError_t launch_copy_cols_permuted(const double* u, double* dst, int64_t N, int n_u, const MatchColumns& cols,
                                     hipStream_t st);
// Profiles by CpG.  launch_first_occurrence: first[c] (n_dst_rows int64, device) = the lowest j < M with idx[j] == c, or
// kNotDrawn; *n_bad (device) = how many idx[j] lie outside [0, n_dst_rows) -- those are not dereferenced.  The table depends
// on idx alone.  launch_copy_rows_first: dst[c][b] = u[first[c]][cols.src[b]], or the quiet NaN where c was not drawn.
constexpr long long kNotDrawn = 0x7fffffffffffffffLL;
hipError_t launch_first_occurrence(const long long* idx, int64_t M, int64_t n_dst_rows, long long* first,
                                   unsigned long long* n_bad, hipStream_t st);
hipError_t launch_copy_rows_first(const double* u, const long long* first, double* dst, int64_t n_dst_rows, int n_u,
                                  const MatchColumns& cols, hipStream_t st);

}  // namespace dmf
