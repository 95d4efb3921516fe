// Small problems: B independent solves of one resident problem per launch, one workgroup per solve
// (dmf_kernels_small.hip, dmf_api_small.hip).  Shared by the kernel's translation unit and the
// C-ABI layer; nothing else includes it.
#pragma once
#include "dmf_batch.h"

namespace dmf {

// the envelope of k_solve_small (dmf_solve_small_supported): the batch envelope with this bound on N S
constexpr int64_t kSmallMaxElements = (int64_t)1 << 20;  // bounds how long one launch can run, not a cross-over
// Outer iterations per launch when the caller passes 0: as many as keep (iterations x N S) within kSmallLaunchElements,
// at least kSmallMinItersPerLaunch and at most kSmallMaxItersPerLaunch.  Measured on an MI355X at the envelope's largest
// shapes (N S = 2^20, 12 + 4 types, 20 inner steps; tools/small_batch_bench.py envelope, profiles/small_batch_bench.txt): one
// outer iteration takes 33 ms at 16384 x 64 (36 ms with 256 solves resident) and 77 ms at 2^20 x 1 (85 ms with 16), so a
// default launch of 2 stays below 0.17 s there; the 350 x 10 example gets 64 iterations per launch.
constexpr int64_t kSmallLaunchElements = (int64_t)1 << 21;
constexpr int kSmallMinItersPerLaunch = 2, kSmallMaxItersPerLaunch = 64;
// The purity variant (dmf_solve_small_purity) is run with the command line's 500 inner steps, and there the row-local u phase
// is what a launch spends its time on: measured at the same shapes with 500 inner steps (same tool,
// profiles/small_batch_purity_bench.txt), one outer iteration takes 40 ms at 16384 x 64 (49 ms with 256 solves resident) and
// 533 ms at 2^20 x 1 (551 ms with 16) -- about 0.5 us per row, whatever S.  Its default is therefore counted in rows:
// kSmallPurityLaunchRows / N, at least 1: 2 iterations (0.10 s) at 16384 x 64, 64 for the 350 x 10 example, within 0.17 s per
// launch up to about 3e5 rows.  Beyond that ONE outer iteration is longer than 0.17 s (0.55 s at 2^20 x 1) and a launch is
// that one iteration: an outer iteration is not cut.
constexpr int64_t kSmallPurityLaunchRows = (int64_t)1 << 15;
inline int small_default_iters_per_launch(int64_t N, int64_t S, bool purity = false) {
    const int64_t q = purity ? kSmallPurityLaunchRows / N : kSmallLaunchElements / (N * S);
    const int64_t lo = purity ? 1 : kSmallMinItersPerLaunch;
    return (int)(q < lo ? lo : (q > kSmallMaxItersPerLaunch ? kSmallMaxItersPerLaunch : q));
}
size_t small_lds_bytes(int S, int K);

// What one launch of k_solve_small works on.  All per-solve state lives in the workspace arrays, indexed by the solve
// b = blockIdx.x.
struct SmallArgs : BatchArgs {
    int n_run = 0;    // outer iterations this launch may run per solve
    int first = 0;    // the launch that sets the solves up (deconvolution.py:192-204)
    double tol = 0.0;
    double* u = nullptr;           // B x N x n_u
    double* u_prev = nullptr;      // B x N x n_u
    double* alpha = nullptr;       // B x K x S
    double* alpha_prev = nullptr;  // B x K x S
    double* gk = nullptr;          // B x known_jobs(n_c) x S: the known block of the per-sample Grams
    double* ratio = nullptr;       // B x 2 x n_iter2: (a_{t-1} - 1) / a_t of the u phase and of the alpha phase
    double* scal = nullptr;        // B x kBatchScalars
    long long* iters = nullptr;    // B
    int* done = nullptr;           // B
    // S doubles or null.  Not null: the purity variant (mdwbssmf_deconv_p, deconvolution.py:306-337), whose alpha phase is
    // Frank-Wolfe with mass purity[s] on the known block of sample s; alpha_prev and the second half of ratio are unused.
    const double* purity = nullptr;
    // B x N x ceil(S / 8) bytes or null.  Not null: solve b has its own train mask (a bi-cross-validation fold, ic.py:58-89)
    // in dmf_problem_mask's layout -- row-major, sample s in bit (s & 7) of byte (s >> 3), 1 = kept, padding bits ignored --
    // and sees the count of an element as 0 where its bit is 0.  Not together with idx or purity.
    const uint8_t* mask = nullptr;
};
hipError_t launch_solve_small(const SmallArgs& a, int64_t B, hipStream_t st);
// n_train[b] = the set bits among the N x S real positions of mask b (grid B; an integer sum in a fixed tree)
hipError_t launch_small_mask_count(const uint8_t* mask, int64_t B, int64_t N, int S, long long* n_train, hipStream_t st);
// sum_sq[b] = sum over the elements whose bit is 0 of (v - [Rt | u_b] alpha_b)^2 on the problem's full V, with (u, alpha) the
// B x N x n_u and B x K x S iterates of the workspace (grid B; ic.py:80 before the division)
hipError_t launch_small_holdout(const double* V, const double* Rt, const double* u, const double* alpha, const uint8_t* mask,
                                int64_t B, int64_t N, int S, int n_c, int n_u, double* sum_sq, hipStream_t st);

}  // namespace dmf
