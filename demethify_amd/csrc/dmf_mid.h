// Mid-size problems: B independent solves of one resident problem per launch, W >= 1 workgroups per solve
// (dmf_kernels_mid.hip, dmf_api_mid.hip).  Shared by the kernels' translation unit and the C-ABI
// layer; nothing else includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dmf {

// the envelope of the mid-size batch (dmf_solve_mid_supported): k_solve_small's, with a larger bound on N S
constexpr int kMidMaxS = 64, kMidMaxK = 16, kMidMaxNu = 4;
constexpr int64_t kMidMaxElements = (int64_t)1 << 23;  // N S: bounds the workspace, not a cross-over
constexpr int kMidThreads = 256;
constexpr int kMidFwMaxThreads = 1024;  // k_mid_alpha_fw: 64 ceil(S / 4) threads, a 16-lane row per sample
constexpr int kMidChunk = 16;     // Gram accumulators per pass over a slab's rows
constexpr int kMidMaxW = 64;      // slabs (workgroups) per solve
constexpr int kMidSlabScalars = 4;  // per (solve, slab): ||u||^2, ||R_trunc||^2, max(D), spare
enum MidScalar { kMdA1, kMdA2, kMdLw, kMdLwPrev, kMdLh, kMdLhPrev, kMdDsq, kMdRtNorm2, kMdCf, kMidScalars = 16 };

bool mid_supported(int64_t N, int64_t S, int64_t n_c, int64_t n_u, int mode);

// The plan: a solve's N rows are cut into W slabs of `rows` rows (a multiple of kMidThreads; the last slab may be ragged),
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

// jobs per sample: the known block (pairs of R_trunc columns and their products with v) and what involves u
__host__ __device__ inline int mid_known_jobs(int n_c) { return n_c * (n_c + 1) / 2 + n_c; }
__host__ __device__ inline int mid_u_jobs(int n_c, int n_u) {
    const int K = n_c + n_u;
    return K * (K + 1) / 2 + K - mid_known_jobs(n_c);
}
// rows of the slab workspace per (solve, slab): the set-up launch puts the known jobs there, every later one the u jobs
inline int mid_slab_jobs(int n_c, int n_u) {
    const int a = mid_known_jobs(n_c), b = mid_u_jobs(n_c, n_u);
    return a > b ? a : b;
}
size_t mid_alpha_lds_bytes(int S, int K);
size_t mid_alpha_fw_lds_bytes(int S, int K);  // k_mid_alpha_fw: G and b, alpha, 256 doubles, the job tables

// What the launches of one call work on.  The problem's arrays and the caller's (idx, u0, alpha0) are read only; all
// per-solve state lives in the workspace arrays, indexed by the solve b and, where it says so, the slab w.
struct MidArgs {
    const double* V = nullptr;        // N_src x S
    const double* D = nullptr;        // N_src x S
    const double* Rt = nullptr;       // N_src x n_c
    const long long* idx = nullptr;   // B x N row indices into the problem, or null: the problem's own rows
    const double* u0 = nullptr;       // B x N x n_u
    const double* alpha0 = nullptr;   // B x K x S
    int64_t N = 0;
    int S = 0, n_c = 0, n_u = 0, mode = 0;
    int64_t n_iter2 = 0;
    double tol = 0.0;
    int64_t rows = 0;  // rows per slab
    int W = 0;         // slabs per solve
    int n_pj = 0;      // mid_slab_jobs(n_c, n_u)
    double* u = nullptr;           // B x N x n_u
    double* u_prev = nullptr;      // B x N x n_u
    double* alpha = nullptr;       // B x K x S
    double* alpha_prev = nullptr;  // B x K x S
    double* gk = nullptr;          // B x mid_known_jobs(n_c) x S: the known block of the per-sample Grams
    double* ratio = nullptr;       // B x 2 x n_iter2: (a_{t-1} - 1) / a_t of the next u phase and alpha phase
    double* scal = nullptr;        // B x kMidScalars; kMdCf is the cost BEFORE the one the cost partials hold
    double* part_g = nullptr;      // B x W x n_pj x S: a slab's partial of the Gram jobs
    double* part_s = nullptr;      // B x W x kMidSlabScalars
    double* part_cf = nullptr;     // B x W: a slab's partial of the streaming cost of the current iterate
    double* cost = nullptr;        // B: the sum of part_cf (k_mid_finish)
    long long* iters = nullptr;    // B
    int* done = nullptr;           // B
};
hipError_t launch_mid_setup(const MidArgs& a, int64_t B, hipStream_t st);      // set-up, then the first cost partials
// k_mid_rows, k_mid_alpha, k_mid_cost; with `purity` (S doubles on the device) k_mid_alpha_fw takes k_mid_alpha's place
hipError_t launch_mid_iteration(const MidArgs& a, int64_t B, hipStream_t st, const double* purity = nullptr);
hipError_t launch_mid_finish(const MidArgs& a, int64_t B, hipStream_t st);     // cost[b], done[b]

}  // namespace dmf
