// C-ABI of libdemethify_hip.so, part 5: the reference-based regression (wls_intercept) of every sample at once.
#include "dmf_api.h"

using namespace dmf_api;

namespace {

// What dmf_wls_intercept and dmf_wls_moments share: the argument checks, the Gram and the device copy of u, and the first
// moments on the stream.
struct WlsWork {
    SolverPtr tmp;
    DevBuf<double> zeros;
    const double* gb = nullptr;  // the packed Gram the solve reads
    DevBuf<double> slab, mom;    // mom: (2 K + 2) x S, enqueued
    int64_t K = 0, S = 0;
};

int wls_enqueue_moments(dmf_context* ctx, const dmf_problem* p, const double* u, int64_t n_u, int target, int flags,
                        WlsWork& w) {
    DMF_TRY(check_ctx(ctx));
    if (p == nullptr || n_u < 0) return DMF_ERR_BAD_ARG;
    if (n_u > 0 && u == nullptr) return DMF_ERR_BAD_ARG;
    if (target != DMF_WLS_TARGET_V && target != DMF_WLS_TARGET_DV) return DMF_ERR_BAD_ARG;
    const int64_t K = p->n_c + n_u, S = p->S;
    if (K < 1) return DMF_ERR_BAD_ARG;
    if (K > dmf::kMaxK) return DMF_ERR_UNSUPPORTED;
    w.K = K, w.S = S;
    // G: the known block as the problem keeps it (rebuilt by every gather and mask), or -- with a u -- the packed Gram of a
    // temporary solver on the caller's u, by the FP64 kernels, as dmf_update_alpha builds it
    w.gb = p->gb_known;
    const double* du = nullptr;
    if (n_u > 0) {
        const size_t an = (size_t)K * S;
        std::vector<double> h_zeros;
        const double* alpha0 = nullptr;
        if (flags & DMF_PTR_DEVICE) {
            HIP_TRY(w.zeros.alloc(ctx, an));
            HIP_TRY(hipMemsetAsync(w.zeros, 0, an * sizeof(double), ctx->stream));
            alpha0 = w.zeros;
        } else {
            h_zeros.assign(an, 0.0);
            alpha0 = h_zeros.data();
        }
        dmf_solver* raw = nullptr;
        DMF_TRY(dmf_solver_create(ctx, p, u, alpha0, n_u, DMF_MODE_PARTIAL,
                                  (flags & DMF_PTR_DEVICE) | DMF_INIT_IN_UNIT_RANGE, &raw));
        w.tmp.reset(raw);
        DMF_TRY(enqueue_gram(raw, fp64_gram_kind(raw)));
        w.gb = raw->gb;
        du = raw->u;
    }
    HIP_TRY(w.slab.alloc(ctx, (size_t)dmf::wls_slab_doubles(p->N, (int)S, (int)K)));
    HIP_TRY(w.mom.alloc(ctx, (size_t)(2 * K + 2) * S));
    // DMF_WLS_F64_ARRAYS: weights and target from V and the f64 counts even where the problem carries (X16, D16), so that
    // the result does not depend on whether it does (the SVD initialiser, whose residual is formed from the f64 V)
    dmf::ProblemView pv = p->view();
    if (flags & DMF_WLS_F64_ARRAYS) pv.X16 = nullptr, pv.D16 = nullptr;
    HIP_TRY(dmf::launch_wls_moments(pv, du, (int)n_u, target == DMF_WLS_TARGET_DV, w.slab, w.mom, ctx->stream));
    return DMF_OK;
}

// k_nnls_intercept on (gb, mom), both on the device, and its results on the host: out_status always, out_alpha for the
// samples with status 0 alone
int nnls_to_host(dmf_context* ctx, const double* gb, const double* mom, int64_t K, int64_t S, double* out_alpha,
                 int* out_status) {
    DevBuf<double> d_alpha;
    DevBuf<int> d_status;
    HIP_TRY(d_alpha.alloc(ctx, (size_t)K * S));
    HIP_TRY(d_status.alloc(ctx, (size_t)S));
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

}  // namespace

extern "C" {

int dmf_wls_intercept(dmf_context* ctx, const dmf_problem* p, const double* u, int64_t n_u, int target, int flags,
                      double* out_alpha, int* out_status) {
    if (out_alpha == nullptr || out_status == nullptr) return DMF_ERR_BAD_ARG;
    WlsWork w;
    DMF_TRY(wls_enqueue_moments(ctx, p, u, n_u, target, flags, w));
    return nnls_to_host(ctx, w.gb, w.mom, w.K, w.S, out_alpha, out_status);
}

int dmf_wls_moments(dmf_context* ctx, const dmf_problem* p, const double* u, int64_t n_u, int target, int flags,
                    double* out_mom) {
    if (out_mom == nullptr) return DMF_ERR_BAD_ARG;
    WlsWork w;
    DMF_TRY(wls_enqueue_moments(ctx, p, u, n_u, target, flags, w));
    HIP_TRY(hipMemcpyAsync(out_mom, w.mom, (size_t)(2 * w.K + 2) * w.S * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DMF_OK;
}

int dmf_nnls_normal(dmf_context* ctx, const double* gb, const double* mom, int64_t K, int64_t S, double* out_alpha,
                    int* out_status) {
    if (gb == nullptr || mom == nullptr || out_alpha == nullptr || out_status == nullptr) return DMF_ERR_BAD_ARG;
    if (K < 1 || S < 1 || S > INT32_MAX) return DMF_ERR_BAD_ARG;
    if (K > dmf::kMaxK) return DMF_ERR_UNSUPPORTED;
    DMF_TRY(check_ctx(ctx));
    DevBuf<double> d_gb, d_mom;
    DMF_TRY(import_array(ctx, gb, (size_t)(K * (K + 1) / 2) * S, 0, d_gb));
    DMF_TRY(import_array(ctx, mom, (size_t)(2 * K + 2) * S, 0, d_mom));
    return nnls_to_host(ctx, d_gb, d_mom, K, S, out_alpha, out_status);
}

}  // extern "C"
