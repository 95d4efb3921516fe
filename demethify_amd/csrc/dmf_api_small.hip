// C-ABI of libdemethify_hip.so, part 7: many independent small solves of one resident problem per launch
// (dmf_solve_small, dmf_solve_small_purity, dmf_solve_small_masked; the kernels are in dmf_kernels_small.hip).
#include "dmf_api_batch.h"
#include "dmf_small.h"

using namespace dmf_api;

// The body of the three entries.  with_purity: `purity` (S doubles) selects the purity variant of the kernel.  with_mask:
// `train_bits` (B x N x ceil(S / 8) bytes) gives every solve a train mask, and the hold-out error of every final iterate goes
// to out_holdout_sum_sq / out_n_test.
static int solve_small(dmf_context* ctx, const dmf_problem* p, int64_t B, const int64_t* idx, const double* u0, const double* alpha0,
                       int64_t n_u, int mode, int64_t n_iter1, int64_t n_iter2, double tol, int64_t iters_per_launch, int flags,
                       bool with_purity, const double* purity, double* out_u, double* out_alpha, double* out_cost,
                       int64_t* out_iters, bool with_mask = false, const uint8_t* train_bits = nullptr,
                       double* out_holdout_sum_sq = nullptr, int64_t* out_n_test = nullptr) {
    if (ctx == nullptr || p == nullptr || B < 1 || B > 0x7fffffff || u0 == nullptr || alpha0 == nullptr || out_u == nullptr ||
        out_alpha == nullptr || out_cost == nullptr || out_iters == nullptr || n_iter1 < 0 || n_iter2 < 0 || iters_per_launch < 0)
        return DMF_ERR_BAD_ARG;
    if (p->ctx != ctx || p->mask_bits != nullptr) return DMF_ERR_BAD_ARG;  // (a masked problem's held-out zeros are not data)
    if (with_mask && (train_bits == nullptr || out_holdout_sum_sq == nullptr || out_n_test == nullptr || idx != nullptr))
        return DMF_ERR_BAD_ARG;
    if (with_purity && (purity == nullptr || p->n_c < 1)) return DMF_ERR_BAD_ARG;  // (no known block to hold at that mass)
    if (with_purity && mode != DMF_MODE_PARTIAL) return DMF_ERR_UNSUPPORTED;
    if (!dmf::batch_supported(p->N, p->S, p->n_c, n_u, mode, dmf::kSmallMaxElements)) return DMF_ERR_UNSUPPORTED;
    DMF_TRY(check_ctx(ctx));
    const int64_t N = p->N, S = p->S, K = p->n_c + n_u;
    const size_t un = (size_t)B * N * n_u, an = (size_t)B * K * S;

    BatchInputs in;
    DMF_TRY(in.import_idx(ctx, idx, B, N, flags));
    BatchMasks masks;
    if (with_mask)  // (a mask that keeps nothing is refused here, while no solve has started)
        DMF_TRY(masks.import_counted(ctx, train_bits, B, N, S, flags, 1, [&](const uint8_t* bits, long long* n_train) {
            return dmf::launch_small_mask_count(bits, B, N, (int)S, n_train, ctx->stream);
        }));
    DMF_TRY(in.import_starts(ctx, u0, alpha0, with_purity ? purity : nullptr, S, un, an, flags));
    BatchWorkspace w;
    DMF_TRY(w.alloc(ctx, B, un, an, p->n_c, S, n_iter2, flags, out_u));
    dmf::SmallArgs a;
    w.fill(a, p, in, n_u, mode, n_iter2, tol);
    if (with_purity) a.purity = in.purity;
    if (with_mask) a.mask = masks.bits;

    const int64_t per_launch = iters_per_launch > 0 ? std::min<int64_t>(iters_per_launch, 1 << 20)
                                                      : dmf::small_default_iters_per_launch(N, S, with_purity);
    int64_t ran = 0;  // outer iterations every unfinished solve has run
    for (bool first = true;; first = false) {
        a.first = first ? 1 : 0;
        a.n_run = (int)std::min<int64_t>(per_launch, n_iter1 - ran);
        HIP_TRY(dmf::launch_solve_small(a, B, ctx->stream));
        ran += a.n_run;
        if (ran >= n_iter1) break;
        bool all = false;
        DMF_TRY(w.all_done(ctx, B, &all));
        if (all) break;
    }

    // the hold-out error of every final iterate, taken where it lives (ic.py:80 before the division)
    DevBuf<double> d_hold;
    std::vector<double> h_hold;
    if (with_mask) {
        h_hold.assign((size_t)B, 0.0);
        HIP_TRY(d_hold.alloc(ctx, (size_t)B));
        HIP_TRY(dmf::launch_small_holdout(p->V, p->Rt, w.u, w.alpha, masks.bits, B, N, (int)S, (int)p->n_c, (int)n_u, d_hold, ctx->stream));
        HIP_TRY(hipMemcpyAsync(h_hold.data(), d_hold, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }

    // out_cost[b] = cost_f_w of the final iterate (the loop's own streaming cost), out_iters[b] = its outer iterations
    std::vector<double> h_scal((size_t)B * dmf::kBatchScalars);
    HIP_TRY(hipMemcpyAsync(h_scal.data(), w.scal, h_scal.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    DMF_TRY(w.copy_out(ctx, B, un, an, flags, out_u, out_alpha, out_iters));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int64_t b = 0; b < B; ++b) out_cost[b] = h_scal[(size_t)b * dmf::kBatchScalars + dmf::kBsCf];
    if (with_mask)
        for (int64_t b = 0; b < B; ++b) out_holdout_sum_sq[b] = h_hold[(size_t)b], out_n_test[b] = N * S - masks.n_train[(size_t)b];
    return DMF_OK;
}

extern "C" {

int dmf_solve_small_supported(int64_t N, int64_t S, int64_t n_c, int64_t n_u, int mode) {
    return dmf::batch_supported(N, S, n_c, n_u, mode, dmf::kSmallMaxElements) ? 1 : 0;
}

int dmf_solve_small(dmf_context* ctx, const dmf_problem* p, int64_t B, const int64_t* idx, const double* u0, const double* alpha0,
                    int64_t n_u, int mode, int64_t n_iter1, int64_t n_iter2, double tol, int64_t iters_per_launch, int flags,
                    double* out_u, double* out_alpha, double* out_cost, int64_t* out_iters) {
    return solve_small(ctx, p, B, idx, u0, alpha0, n_u, mode, n_iter1, n_iter2, tol, iters_per_launch, flags, false, nullptr, out_u,
                       out_alpha, out_cost, out_iters);
}

int dmf_solve_small_purity(dmf_context* ctx, const dmf_problem* p, int64_t B, const int64_t* idx, const double* u0,
                           const double* alpha0, const double* purity, int64_t n_u, int mode, int64_t n_iter1, int64_t n_iter2,
                           double tol, int64_t iters_per_launch, int flags, double* out_u, double* out_alpha, double* out_cost,
                           int64_t* out_iters) {
    return solve_small(ctx, p, B, idx, u0, alpha0, n_u, mode, n_iter1, n_iter2, tol, iters_per_launch, flags, true, purity, out_u,
                       out_alpha, out_cost, out_iters);
}

int dmf_solve_small_masked(dmf_context* ctx, const dmf_problem* p, int64_t B, const uint8_t* train_bits, const double* u0,
                           const double* alpha0, int64_t n_u, int mode, int64_t n_iter1, int64_t n_iter2, double tol,
                           int64_t iters_per_launch, int flags, double* out_u, double* out_alpha, double* out_cost,
                           int64_t* out_iters, double* out_holdout_sum_sq, int64_t* out_n_test) {
    return solve_small(ctx, p, B, nullptr, u0, alpha0, n_u, mode, n_iter1, n_iter2, tol, iters_per_launch, flags, false, nullptr,
                       out_u, out_alpha, out_cost, out_iters, true, train_bits, out_holdout_sum_sq, out_n_test);
}

}  // extern "C"
