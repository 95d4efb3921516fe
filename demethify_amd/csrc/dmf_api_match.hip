// C-ABI of libdemethify_hip.so, part 7: component matching for the bootstrap (dmf_kernels_match.hip) -- the inner products of
// a solver's profile columns with an anchor's, and the copy of the profiles out of the solver with the columns renamed.
#include "dmf_api.h"

using namespace dmf_api;

extern "C" {

int dmf_solver_match_components(dmf_solver* s, const void* anchor_dev, int64_t n_anchor_rows, const int64_t* idx_dev,
                                double* out_P) {
    if (s == nullptr || anchor_dev == nullptr || out_P == nullptr || n_anchor_rows < 1) return DMF_ERR_BAD_ARG;
    dmf_context* ctx = s->ctx;
    DMF_TRY(check_ctx(ctx));
    const int64_t N = s->p->N;
    const int n_u = (int)s->n_u;
    if (idx_dev == nullptr && n_anchor_rows != N) return DMF_ERR_BAD_SHAPE;
    const int grid = dmf::match_gram_grid(N, n_u);
    const size_t np = (size_t)n_u * n_u;
    DevBuf<double> slab, d_p;
    DevBuf<int> d_flags;
    HIP_TRY(slab.alloc(ctx, (size_t)dmf::match_gram_slab_doubles(N, n_u)));
    HIP_TRY(d_p.alloc(ctx, np));
    HIP_TRY(d_flags.alloc(ctx, (size_t)grid));
    {
        FamilyScope scope(ctx, DMF_KERNEL_GRAM);  // (k_match_gram and its reduce, for tools/component_match_bench.py)
        HIP_TRY(dmf::launch_match_gram(s->u, static_cast<const double*>(anchor_dev), reinterpret_cast<const long long*>(idx_dev),
                                       N, n_anchor_rows, n_u, slab, d_flags, d_p, ctx->stream));
    }
    std::vector<int> h_flags((size_t)grid);
    std::vector<double> h_p(np);
    HIP_TRY(hipMemcpyAsync(h_flags.data(), d_flags, h_flags.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(h_p.data(), d_p, np * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int b = 0; b < grid; ++b)
        if (h_flags[(size_t)b] != 0) return DMF_ERR_BAD_ARG;  // (an index outside the anchor's rows: out_P stays as it was)
    std::memcpy(out_P, h_p.data(), np * sizeof(double));
    return DMF_OK;
}

// src_col as the copy kernels take it: a permutation of 0 .. n_u - 1 (DMF_ERR_BAD_ARG otherwise)
static int permutation_columns(const int32_t* src_col, int n_u, dmf::MatchColumns& cols) {
    bool seen[dmf::kMaxK] = {};
    for (int b = 0; b < n_u; ++b) {
        const int32_t c = src_col[b];
        if (c < 0 || c >= n_u || seen[c]) return DMF_ERR_BAD_ARG;
        seen[c] = true;
        cols.src[b] = c;
    }
    return DMF_OK;
}

int dmf_solver_get_u_by_row(dmf_solver* s, const int64_t* idx_dev, int64_t n_dst_rows, const int32_t* src_col, void* dst_dev) {
    if (s == nullptr || idx_dev == nullptr || dst_dev == nullptr || n_dst_rows < 1 || s->n_u < 1) return DMF_ERR_BAD_ARG;
    dmf_context* ctx = s->ctx;
    DMF_TRY(check_ctx(ctx));
    const int n_u = (int)s->n_u;
    if (dst_dev == (void*)s->u.get()) return DMF_ERR_BAD_ARG;
    dmf::MatchColumns cols = {};
    if (src_col != nullptr) DMF_TRY(permutation_columns(src_col, n_u, cols));
    else
        for (int b = 0; b < n_u; ++b) cols.src[b] = b;
    // (pool blocks: the next replicate's call gets the same ones back)
    DevBuf<long long> first;
    DevBuf<unsigned long long> d_bad;
    HIP_TRY(first.alloc(ctx, (size_t)n_dst_rows));
    HIP_TRY(d_bad.alloc(ctx, 1));
    {
        FamilyScope scope(ctx, DMF_KERNEL_GRAM);
        HIP_TRY(dmf::launch_first_occurrence(reinterpret_cast<const long long*>(idx_dev), s->p->N, n_dst_rows, first, d_bad,
                                             ctx->stream));
    }
    unsigned long long h_bad = 0;
    HIP_TRY(hipMemcpyAsync(&h_bad, d_bad, sizeof(h_bad), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (h_bad != 0) return DMF_ERR_BAD_ARG;  // (an index outside the destination's rows: dst_dev stays as it was)
    {
        FamilyScope scope(ctx, DMF_KERNEL_GRAM);
        HIP_TRY(dmf::launch_copy_rows_first(s->u, first, static_cast<double*>(dst_dev), n_dst_rows, n_u, cols, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // (like dmf_solver_get_u_permuted: dst is complete when this returns)
    return DMF_OK;
}

int dmf_solver_get_u_permuted(dmf_solver* s, const int32_t* src_col, void* dst_dev) {
    if (s == nullptr || src_col == nullptr || dst_dev == nullptr) return DMF_ERR_BAD_ARG;
    dmf_context* ctx = s->ctx;
    DMF_TRY(check_ctx(ctx));
    const int n_u = (int)s->n_u;
    if (dst_dev == (void*)s->u.get()) return DMF_ERR_BAD_ARG;
    dmf::MatchColumns cols = {};
    DMF_TRY(permutation_columns(src_col, n_u, cols));
    {
        FamilyScope scope(ctx, DMF_KERNEL_GRAM);
        HIP_TRY(dmf::launch_copy_cols_permuted(s->u, static_cast<double*>(dst_dev), s->p->N, n_u, cols, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // (like dmf_solver_get: dst is complete when this returns)
    return DMF_OK;
}

}  // extern "C"
