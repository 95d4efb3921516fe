// C-ABI of libdemethify_hip.so, part 8: many independent mid-size solves of one resident problem, several workgroups per
// solve (dmf_solve_mid, dmf_solve_mid_purity, dmf_solve_mid_masked, dmf_solve_mid_plan, dmf_solve_mid_supported; the kernels
// are in dmf_kernels_mid.hip).
#include "dmf_api_batch.h"
#include "dmf_mid.h"

using namespace dmf_api;

// The body of the three solve entries.  with_purity: `purity` (S doubles) selects the Frank-Wolfe alpha launch.  with_mask:
// `train_bits` (B x N x ceil(S / 8) bytes) gives every solve a train mask, the MASK instances of the slab kernels run, and the
// hold-out error of every final iterate goes to out_holdout_sum_sq / out_n_test.
static int solve_mid(dmf_context* ctx, const dmf_problem* p, int64_t B, const int64_t* idx, const double* u0, const double* alpha0,
                     int64_t n_u, int mode, int64_t n_iter1, int64_t n_iter2, double tol, int64_t rows_per_workgroup,
                     int64_t check_every, int flags, bool with_purity, const double* purity, double* out_u, double* out_alpha,
                     double* out_cost, int64_t* out_iters, bool with_mask = false, const uint8_t* train_bits = nullptr,
                     double* out_holdout_sum_sq = nullptr, int64_t* out_n_test = nullptr) {
    if (ctx == nullptr || p == nullptr || B < 1 || B > 0x7fffffff || u0 == nullptr || alpha0 == nullptr || out_u == nullptr ||
        out_alpha == nullptr || out_cost == nullptr || out_iters == nullptr || n_iter1 < 0 || n_iter2 < 0 ||
        rows_per_workgroup < 0 || check_every < 0)
        return DMF_ERR_BAD_ARG;
    if (p->ctx != ctx || p->mask_bits != nullptr) return DMF_ERR_BAD_ARG;  // (a masked problem's held-out zeros are not data)
    if (with_mask && (train_bits == nullptr || out_holdout_sum_sq == nullptr || out_n_test == nullptr || idx != nullptr ||
                      with_purity))
        return DMF_ERR_BAD_ARG;
    if (with_purity && (purity == nullptr || p->n_c < 1)) return DMF_ERR_BAD_ARG;  // (no known block to hold at that mass)
    if (with_purity && mode != DMF_MODE_PARTIAL) return DMF_ERR_UNSUPPORTED;
    if (!dmf::batch_supported(p->N, p->S, p->n_c, n_u, mode, dmf::kMidMaxElements)) return DMF_ERR_UNSUPPORTED;
    dmf::MidPlan plan;
    if (!dmf::mid_plan(p->N, p->S, rows_per_workgroup, &plan) || B > 0x7fffffff / plan.W) return DMF_ERR_BAD_ARG;
    DMF_TRY(check_ctx(ctx));
    const int64_t N = p->N, S = p->S, K = p->n_c + n_u, W = plan.W;
    const size_t un = (size_t)B * N * n_u, an = (size_t)B * K * S;

    BatchInputs in;
    DMF_TRY(in.import_idx(ctx, idx, B, N, flags));
    BatchMasks masks;
    if (with_mask)  // (counted per slab; a mask that keeps nothing is refused here, while no solve has started)
        DMF_TRY(masks.import_counted(ctx, train_bits, B, N, S, flags, W, [&](const uint8_t* bits, long long* n_part) {
            return dmf::launch_mid_mask_count(bits, B, N, (int)S, plan.rows, plan.W, n_part, ctx->stream);
        }));
    DMF_TRY(in.import_starts(ctx, u0, alpha0, with_purity ? purity : nullptr, S, un, an, flags));
    const double* fw_purity = with_purity ? (const double*)in.purity : nullptr;

    // the workspace: all per-solve state and the slab partials (the purity variant uses the same, less alpha_, a2 and l_h)
    const int n_pj = dmf::mid_slab_jobs((int)p->n_c, (int)n_u);
    BatchWorkspace w;
    DevBuf<double> w_pg, w_ps, w_pc, w_cost;
    DMF_TRY(w.alloc(ctx, B, un, an, p->n_c, S, n_iter2, flags, out_u));
    HIP_TRY(w_pg.alloc(ctx, (size_t)B * W * n_pj * S));
    HIP_TRY(w_ps.alloc(ctx, (size_t)B * W * dmf::kMidSlabScalars));
    HIP_TRY(w_pc.alloc(ctx, (size_t)B * W));
    HIP_TRY(w_cost.alloc(ctx, (size_t)B));

    dmf::MidArgs a;
    w.fill(a, p, in, n_u, mode, n_iter2, tol);
    a.rows = plan.rows, a.W = plan.W, a.n_pj = n_pj;
    a.part_g = w_pg, a.part_s = w_ps, a.part_cf = w_pc, a.cost = w_cost;
    if (with_mask) a.mask = masks.bits;

    HIP_TRY(dmf::launch_mid_setup(a, B, ctx->stream));
    const int64_t every = check_every > 0 ? std::min<int64_t>(check_every, 1 << 20) : plan.check_every;
    for (int64_t ran = 0; ran < n_iter1;) {
        const int64_t n_run = std::min<int64_t>(every, n_iter1 - ran);
        for (int64_t it = 0; it < n_run; ++it) HIP_TRY(dmf::launch_mid_iteration(a, B, ctx->stream, fw_purity));
        ran += n_run;
        if (ran >= n_iter1) break;
        HIP_TRY(dmf::launch_mid_finish(a, B, ctx->stream));
        bool all = false;
        DMF_TRY(w.all_done(ctx, B, &all));
        if (all) break;
    }

    // the slab partials of the hold-out error of every final iterate, taken where it lives (ic.py:80 before the division)
    DevBuf<double> d_hold;
    std::vector<double> h_hold;
    if (with_mask) {
        h_hold.assign((size_t)(B * W), 0.0);
        HIP_TRY(d_hold.alloc(ctx, h_hold.size()));
        HIP_TRY(dmf::launch_mid_holdout(a, B, d_hold, ctx->stream));
        HIP_TRY(hipMemcpyAsync(h_hold.data(), d_hold, h_hold.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }

    // out_cost[b] = cost_f_w of the final iterate (the loop's own streaming cost), out_iters[b] = its outer iterations
    HIP_TRY(dmf::launch_mid_finish(a, B, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out_cost, w_cost, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    DMF_TRY(w.copy_out(ctx, B, un, an, flags, out_u, out_alpha, out_iters));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (with_mask)
        for (int64_t b = 0; b < B; ++b) {
            double sum = 0.0;  // rising slab order
            for (int64_t sl = 0; sl < W; ++sl) sum += h_hold[(size_t)(b * W + sl)];
            out_holdout_sum_sq[b] = sum, out_n_test[b] = N * S - masks.n_train[(size_t)b];
        }
    return DMF_OK;
}

extern "C" {

int dmf_solve_mid_supported(int64_t N, int64_t S, int64_t n_c, int64_t n_u, int mode) {
    return dmf::batch_supported(N, S, n_c, n_u, mode, dmf::kMidMaxElements) ? 1 : 0;
}

int dmf_solve_mid_plan(int64_t N, int64_t S, int64_t rows_per_workgroup, int64_t* out_rows, int64_t* out_W,
                       int64_t* out_check_every) {
    dmf::MidPlan plan;
    if (out_rows == nullptr || out_W == nullptr || out_check_every == nullptr || N > ((int64_t)1 << 40) ||
        !dmf::mid_plan(N, S, rows_per_workgroup, &plan))
        return DMF_ERR_BAD_ARG;
    *out_rows = plan.rows, *out_W = plan.W, *out_check_every = plan.check_every;
    return DMF_OK;
}

int dmf_solve_mid(dmf_context* ctx, const dmf_problem* p, int64_t B, const int64_t* idx, const double* u0, const double* alpha0,
                  int64_t n_u, int mode, int64_t n_iter1, int64_t n_iter2, double tol, int64_t rows_per_workgroup,
                  int64_t check_every, int flags, double* out_u, double* out_alpha, double* out_cost, int64_t* out_iters) {
    return solve_mid(ctx, p, B, idx, u0, alpha0, n_u, mode, n_iter1, n_iter2, tol, rows_per_workgroup, check_every, flags, false,
                     nullptr, out_u, out_alpha, out_cost, out_iters);
}

int dmf_solve_mid_purity(dmf_context* ctx, const dmf_problem* p, int64_t B, const int64_t* idx, const double* u0,
                         const double* alpha0, const double* purity, int64_t n_u, int mode, int64_t n_iter1, int64_t n_iter2,
                         double tol, int64_t rows_per_workgroup, int64_t check_every, int flags, double* out_u, double* out_alpha,
                         double* out_cost, int64_t* out_iters) {
    return solve_mid(ctx, p, B, idx, u0, alpha0, n_u, mode, n_iter1, n_iter2, tol, rows_per_workgroup, check_every, flags, true,
                     purity, out_u, out_alpha, out_cost, out_iters);
}

int dmf_solve_mid_masked(dmf_context* ctx, const dmf_problem* p, int64_t B, const uint8_t* train_bits, const double* u0,
                         const double* alpha0, int64_t n_u, int mode, int64_t n_iter1, int64_t n_iter2, double tol,
                         int64_t rows_per_workgroup, int64_t check_every, int flags, double* out_u, double* out_alpha,
                         double* out_cost, int64_t* out_iters, double* out_holdout_sum_sq, int64_t* out_n_test) {
    return solve_mid(ctx, p, B, nullptr, u0, alpha0, n_u, mode, n_iter1, n_iter2, tol, rows_per_workgroup, check_every, flags, false,
                     nullptr, out_u, out_alpha, out_cost, out_iters, true, train_bits, out_holdout_sum_sq, out_n_test);
}

}  // extern "C"
