// Mid-size problems: B independent solves of one resident problem per launch, W >= 1 workgroups per solve
// (dmf_kernels_mid.hip, dmf_api_mid.hip).  Shared by the kernels' translation unit and the C-ABI
// layer; nothing else includes it.
#pragma once
#include "dmf_batch.h"

namespace dmf {

// the envelope of the mid-size batch (dmf_solve_mid_supported): the batch envelope with this bound on N S
constexpr int64_t kMidMaxElements = (int64_t)1 << 23;  // bounds the workspace, not a cross-over
constexpr int kMidFwMaxThreads = 1024;  // k_mid_alpha_fw: 64 ceil(S / 4) threads, a 16-lane row per sample
constexpr int kMidMaxW = 64;      // slabs (workgroups) per solve
constexpr int kMidSlabScalars = 4;  // per (solve, slab): ||u||^2, ||R_trunc||^2, max(D), spare

// The plan: a solve's N rows are cut into W slabs of `rows` rows (a multiple of kBatchThreads; the last slab may be ragged),
// and the host reads the stop flags every `check_every` outer iterations.  Defaults, functions of (N, S) alone:
//   rows         the smallest multiple of 256 that keeps W <= 64: as many workgroups per solve as the envelope allows,
//                a thread per row up to N = 16 384
//   check_every  2^22 / (N S), at least 4 and at most 16: a check drains the stream once, and the launches enqueued for
//                solves that have stopped return at their first instruction
// rows_per_workgroup = 0 asks for the default; any other value must be a positive multiple of 256 with W <= 64.
struct MidPlan {
    int64_t rows = 0;
    int W = 0;
    int check_every = 0;
};
bool mid_plan(int64_t N, int64_t S, int64_t rows_per_workgroup, MidPlan* out);

// rows of the slab workspace per (solve, slab): the set-up launch puts the known jobs there, every later one the u jobs
inline int mid_slab_jobs(int n_c, int n_u) {
    const int a = known_jobs(n_c), b = u_jobs(n_c, n_u);
    return a > b ? a : b;
}
size_t mid_alpha_lds_bytes(int S, int K);
size_t mid_alpha_fw_lds_bytes(int S, int K);  // k_mid_alpha_fw: G and b, alpha, 256 doubles, the job tables

// What the launches of one call work on; the workspace arrays are indexed by the solve b and, where it says so, the slab w.
// scal[kBsCf] is the cost BEFORE the one the cost partials hold.
struct MidArgs : BatchArgs {
    double tol = 0.0;
    int64_t rows = 0;  // rows per slab
    int W = 0;         // slabs per solve
    int n_pj = 0;      // mid_slab_jobs(n_c, n_u)
    double* u = nullptr;           // B x N x n_u
    double* u_prev = nullptr;      // B x N x n_u
    double* alpha = nullptr;       // B x K x S
    double* alpha_prev = nullptr;  // B x K x S
    double* gk = nullptr;          // B x known_jobs(n_c) x S: the known block of the per-sample Grams
    double* ratio = nullptr;       // B x 2 x n_iter2: (a_{t-1} - 1) / a_t of the next u phase and alpha phase
    double* scal = nullptr;        // B x kBatchScalars
    double* part_g = nullptr;      // B x W x n_pj x S: a slab's partial of the Gram jobs
    double* part_s = nullptr;      // B x W x kMidSlabScalars
    double* part_cf = nullptr;     // B x W: a slab's partial of the streaming cost of the current iterate
    double* cost = nullptr;        // B: the sum of part_cf (k_mid_finish)
    long long* iters = nullptr;    // B
    int* done = nullptr;           // B
    // B x N x ceil(S / 8) bytes or null.  Not null: solve b has its own train mask (a bi-cross-validation fold, ic.py:58-89) in
    // dmf_problem_mask's layout -- row-major, sample s in bit (s & 7) of byte (s >> 3), 1 = kept, padding bits ignored -- and
    // the MASK instances of the slab kernels run, which see the count of an element as 0 where its bit is 0.  Not together with
    // idx or purity.  The last field: every other one keeps its place (dmf_batch.h on why that matters).
    const uint8_t* mask = nullptr;
};
hipError_t launch_mid_setup(const MidArgs& a, int64_t B, hipStream_t st);      // set-up, then the first cost partials
// k_mid_rows, k_mid_alpha, k_mid_cost; with `purity` (S doubles on the device) k_mid_alpha_fw takes k_mid_alpha's place
hipError_t launch_mid_iteration(const MidArgs& a, int64_t B, hipStream_t st, const double* purity = nullptr);
hipError_t launch_mid_finish(const MidArgs& a, int64_t B, hipStream_t st);     // cost[b], done[b]
// the framing passes of a masked call, a workgroup per slab of the plan (rows, W):
// n_part[b W + w] = the set bits among the real positions of slab w's rows of mask b (integers: add them in any order)
hipError_t launch_mid_mask_count(const uint8_t* mask, int64_t B, int64_t N, int S, int64_t rows, int W, long long* n_part,
                                 hipStream_t st);
// part_h[b W + w] = slab w's partial of the sum over the held-out elements of (v - [Rt | u_b] alpha_b)^2 on the problem's full V
// with the workspace's iterate; a solve's hold-out sum is its W partials added in rising slab order
hipError_t launch_mid_holdout(const MidArgs& a, int64_t B, double* part_h, hipStream_t st);

}  // namespace dmf
