// C-ABI of libdemethify_hip.so, part 5: the reference-based regression (wls_intercept) of every sample at once.
#include "dmf_api.h"

using namespace dmf_api;

extern "C" {

int dmf_wls_intercept(dmf_context* ctx, const dmf_problem* p, const double* u, int64_t n_u, int target, int flags,
                      double* out_alpha, int* out_status) {
    DMF_TRY(check_ctx(ctx));
    if (p == nullptr || out_alpha == nullptr || out_status == nullptr || n_u < 0) return DMF_ERR_BAD_ARG;
    if (n_u > 0 && u == nullptr) return DMF_ERR_BAD_ARG;
    if (target != DMF_WLS_TARGET_V && target != DMF_WLS_TARGET_DV) return DMF_ERR_BAD_ARG;
    const int64_t K = p->n_c + n_u, S = p->S;
    if (K < 1) return DMF_ERR_BAD_ARG;
    if (K > dmf::kMaxK) return DMF_ERR_UNSUPPORTED;
    // G: the known block as the problem keeps it (rebuilt by every gather and mask), or -- with a u -- the packed Gram of a
    // temporary solver on the caller's u, by the FP64 kernels, as dmf_update_alpha builds it
    SolverPtr tmp;
    DevBuf<double> zeros;
    const double* gb = p->gb_known;
    const double* du = nullptr;
    if (n_u > 0) {
        const size_t an = (size_t)K * S;
        std::vector<double> h_zeros;
        const double* alpha0 = nullptr;
        if (flags & DMF_PTR_DEVICE) {
            HIP_TRY(zeros.alloc(ctx, an));
            HIP_TRY(hipMemsetAsync(zeros, 0, an * sizeof(double), ctx->stream));
            alpha0 = zeros;
        } else {
            h_zeros.assign(an, 0.0);
            alpha0 = h_zeros.data();
        }
        dmf_solver* raw = nullptr;
        DMF_TRY(dmf_solver_create(ctx, p, u, alpha0, n_u, DMF_MODE_PARTIAL,
                                  (flags & DMF_PTR_DEVICE) | DMF_INIT_IN_UNIT_RANGE, &raw));
        tmp.reset(raw);
        DMF_TRY(enqueue_gram(raw, fp64_gram_kind(raw)));
        gb = raw->gb;
        du = raw->u;
    }
    DevBuf<double> slab, mom, d_alpha;
    DevBuf<int> d_status;
    HIP_TRY(slab.alloc(ctx, (size_t)dmf::wls_slab_doubles(p->N, (int)S, (int)K)));
    HIP_TRY(mom.alloc(ctx, (size_t)(2 * K + 2) * S));
    HIP_TRY(d_alpha.alloc(ctx, (size_t)K * S));
    HIP_TRY(d_status.alloc(ctx, (size_t)S));
    // DMF_WLS_F64_ARRAYS: weights and target from V and the f64 counts even where the problem carries (X16, D16), so that
    // the result does not depend on whether it does (the SVD initialiser, whose residual is formed from the f64 V)
    dmf::ProblemView pv = p->view();
    if (flags & DMF_WLS_F64_ARRAYS) pv.X16 = nullptr, pv.D16 = nullptr;
    HIP_TRY(dmf::launch_wls_moments(pv, du, (int)n_u, target == DMF_WLS_TARGET_DV, slab, mom, ctx->stream));
    HIP_TRY(dmf::launch_nnls_intercept(gb, mom, (int)K, (int)S, d_alpha, d_status, ctx->stream));
    std::vector<double> h_alpha((size_t)K * S);
    HIP_TRY(hipMemcpyAsync(out_status, d_status, (size_t)S * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(h_alpha.data(), d_alpha, h_alpha.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int64_t s = 0; s < S; ++s)
        if (out_status[s] == 0)
            for (int64_t k = 0; k < K; ++k) out_alpha[k * S + s] = h_alpha[(size_t)(k * S + s)];
    return DMF_OK;
}

}  // extern "C"
