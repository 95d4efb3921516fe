// C-ABI of libdemethify_hip.so, part 6: the SVD initialiser by the Gram route (dmf_kernels_svd.hip).  The symmetric
// eigendecomposition of the S x S Gram stays with the caller, between dmf_svd_gram and dmf_svd_factor: no LAPACK here.
#include "dmf_api.h"

using namespace dmf_api;

namespace {

// what the three entry points check alike: the problem, its shape, H1's presence
int svd_check(dmf_context* ctx, const dmf_problem* p, const double* H1, int64_t rank) {
    if (p == nullptr || p->ctx != ctx || rank < 0) return DMF_ERR_BAD_ARG;
    if (p->mask_bits != nullptr) return DMF_ERR_BAD_ARG;  // (held-out elements are zeros in V: not the matrix the caller means)
    if (p->n_c > 0 && H1 == nullptr) return DMF_ERR_BAD_ARG;
    if (p->S > dmf::kSvdMaxS || p->n_c > dmf::kSvdMaxNc || rank > dmf::kSvdMaxRank) return DMF_ERR_UNSUPPORTED;
    if (!dmf::svd_supported((int)p->S, (int)p->n_c, (int)rank)) return DMF_ERR_UNSUPPORTED;
    return DMF_OK;
}

}  // namespace

extern "C" {

int dmf_svd_gram(dmf_context* ctx, const dmf_problem* p, const double* H1, int flags, double* out_C, int64_t* out_flags) {
    DMF_TRY(check_ctx(ctx));
    if (out_C == nullptr || out_flags == nullptr) return DMF_ERR_BAD_ARG;
    DMF_TRY(svd_check(ctx, p, H1, 0));
    const int64_t S = p->S;
    const int nbx = dmf::svd_gram_grid(p->N, (int)S);
    DevBuf<double> d_h1, slab, d_c;
    DevBuf<int> d_flags;
    DMF_TRY(import_array(ctx, H1, (size_t)(p->n_c * S), flags, d_h1));
    HIP_TRY(slab.alloc(ctx, (size_t)dmf::svd_gram_slab_doubles(p->N, (int)S)));
    HIP_TRY(d_c.alloc(ctx, (size_t)(S * S)));
    HIP_TRY(d_flags.alloc(ctx, (size_t)2 * nbx));
    {
        FamilyScope scope(ctx, DMF_KERNEL_GRAM);  // (k_svd_gram and its reduce, for tools/svd_init_bench.py)
        HIP_TRY(dmf::launch_svd_gram(p->view(), d_h1, slab, d_flags, d_c, ctx->stream));
    }
    std::vector<int> h_flags((size_t)2 * nbx);
    HIP_TRY(hipMemcpyAsync(h_flags.data(), d_flags, h_flags.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out_C, d_c, (size_t)(S * S) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    out_flags[0] = out_flags[1] = 0;
    for (int b = 0; b < nbx; ++b) {
        out_flags[0] += h_flags[(size_t)2 * b];
        out_flags[1] += h_flags[(size_t)2 * b + 1];
    }
    for (int64_t x = 0; x < S * S; ++x)
        if (!std::isfinite(out_C[x])) return DMF_ERR_NONFINITE;
    return DMF_OK;
}

int dmf_svd_factor(dmf_context* ctx, const dmf_problem* p, const double* H1, const double* E_over_sigma, int64_t rank,
                   int flags, double* out_norms, void** out_T) {
    DMF_TRY(check_ctx(ctx));
    if (E_over_sigma == nullptr || out_norms == nullptr || out_T == nullptr || rank < 1) return DMF_ERR_BAD_ARG;
    *out_T = nullptr;
    DMF_TRY(svd_check(ctx, p, H1, rank));
    const int64_t S = p->S;
    DevBuf<double> d_h1, d_es, slab, d_norms;
    DMF_TRY(import_array(ctx, H1, (size_t)(p->n_c * S), flags, d_h1));
    DMF_TRY(import_array(ctx, E_over_sigma, (size_t)(S * rank), 0, d_es));
    HIP_TRY(slab.alloc(ctx, (size_t)dmf::svd_project_slab_doubles(p->N, (int)rank)));
    HIP_TRY(d_norms.alloc(ctx, (size_t)(2 * rank)));
    // T leaves as the caller's: a block of the context's pool, released with dmf_stage_free
    void* t = nullptr;
    HIP_TRY(pool_alloc(ctx, &t, (size_t)(p->N * rank) * sizeof(double)));
    const hipError_t e = dmf::launch_svd_project(p->view(), d_h1, d_es, (int)rank, static_cast<double*>(t), slab, d_norms,
                                                 ctx->stream);
    const int rc = e != hipSuccess ? hip_fail(e, "launch_svd_project", __FILE_NAME__, __LINE__)
                                   : export_array(ctx, d_norms, (size_t)(2 * rank) * sizeof(double), 0, out_norms);
    if (rc != DMF_OK) {
        pool_free(ctx, t);
        return rc;
    }
    *out_T = t;
    return DMF_OK;
}

int dmf_svd_finish(dmf_context* ctx, void* T, int64_t N, int64_t rank, const double* sign, const double* scale, int flags,
                   double* out_u) {
    DMF_TRY(check_ctx(ctx));
    if (T == nullptr || sign == nullptr || scale == nullptr || N < 1 || rank < 1) return DMF_ERR_BAD_ARG;
    if (rank > dmf::kSvdMaxRank) return DMF_ERR_UNSUPPORTED;
    if (!(flags & DMF_PTR_DEVICE) && out_u == nullptr) return DMF_ERR_BAD_ARG;
    dmf::SvdColumns cols = {};
    for (int64_t j = 0; j < rank; ++j) cols.sign[j] = sign[j], cols.scale[j] = scale[j];
    HIP_TRY(dmf::launch_svd_finish(static_cast<double*>(T), N, (int)rank, cols, ctx->stream));
    if (flags & DMF_PTR_DEVICE) {  // u0 stays where it is, or goes to another device array
        if (out_u != nullptr && out_u != T)
            HIP_TRY(hipMemcpyAsync(out_u, T, (size_t)(N * rank) * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        return DMF_OK;
    }
    return export_array(ctx, T, (size_t)(N * rank) * sizeof(double), 0, out_u);
}

}  // extern "C"
