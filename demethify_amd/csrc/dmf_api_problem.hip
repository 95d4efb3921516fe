// C-ABI of libdemethify_hip.so, part 2: problems -- creation from the caller's arrays, the row-gathered and the masked
// copies of a resident problem, their constants and integer count copies, and the streaming cost on a problem's data.
#include "dmf_api.h"

namespace dmf_api {

// The integer copies of the counts: sets ND / SD / N16 / plane_stride from (N, S, ND) and allocates D16 and Dt8, plus
// X16 and W16 on request (their contents are the caller's to write).
static int alloc_count_copies(dmf_problem* p, int ND, bool x16, bool w16) {
    dmf_context* ctx = p->ctx;
    p->ND = ND;
    p->SD = (int)((p->S + 63) / 64 * 64);
    p->N16 = (p->N + 15) / 16 * 16;
    p->plane_stride = ((p->N + 31) / 32) * (p->SD / 32) * 1024;
    const size_t u16_elems = (size_t)p->N16 * p->SD;
    HIP_TRY(p->D16.alloc(ctx, u16_elems));
    HIP_TRY(p->Dt8.alloc(ctx, (size_t)p->plane_stride * ND));
    if (x16) HIP_TRY(p->X16.alloc(ctx, u16_elems));
    if (w16) HIP_TRY(p->W16.alloc(ctx, u16_elems));
    return DMF_OK;
}

// The byte images X8 / D8 of the problem's X16 / D16, where some launch plan of the row pass reads them
// (dmf::rowpass_v2_byte_images_wanted).  Called by
// problem_finalize once the integer copies and the largest count stand, so for every problem that is created, gathered or
// masked -- a masked problem's X16 / D16 carry the masked counts, and so do its images.
static int build_rowpass_images(dmf_problem* p) {
    dmf_context* ctx = p->ctx;
    const bool x16 = p->X16 != nullptr && p->D16 != nullptr;
    if (!dmf::rowpass_v2_byte_images_wanted((int)p->S, x16, p->h_consts[kIntCountMax])) return DMF_OK;
    const size_t bytes = (size_t)p->N16 * p->SD;
    HIP_TRY(p->X8.alloc(ctx, bytes));
    HIP_TRY(p->D8.alloc(ctx, bytes));
    HIP_TRY(dmf::launch_build_rowpass_images(p->X16, p->D16, p->N16, p->SD, p->X8, p->D8, ctx->stream));
    return DMF_OK;
}

// one more piece of dmf_problem::known_ran, the text of dmf_problem_gram_known: "int_known" / "fp64" (without either: fp64),
// then every launcher that contributed rows, in launch order, separated by blanks
static void known_route(dmf_problem* p, const char* piece) {
    char* t = p->known_ran.text;
    const size_t have = std::strlen(t), cap = sizeof(p->known_ran.text);
    snprintf(t + have, cap - have, "%s%s", have > 0 ? " " : "", piece);
}

// Builds the per-problem constants: max(D)^2, ||Rt||_F^2 and the known block of the packed Gram.
// `counts_done`: a copy of a resident problem (dmf_problem_gather, dmf_problem_mask) whose integer count copies are
// already written from the source's and whose count constants -- max(D) in kDmax and kIntCountMax, the exactness flags
// copied -- are set by the caller: the three scans of D and the rebuild of the integer copies are skipped.
static int problem_finalize(dmf_problem* p, bool counts_done = false) {
    dmf_context* ctx = p->ctx;
    const int64_t N = p->N, S = p->S, n_c = p->n_c;
    double* const h = p->h_consts;
    HIP_TRY(p->consts.alloc(ctx, kProblemConsts));
    if (!counts_done) HIP_TRY(dmf::launch_max_f64(p->D, N * S, ctx->scratch, p->consts + kDmax, ctx->stream));
    if (n_c > 0) {
        HIP_TRY(dmf::launch_sumsq_f64(p->Rt, N * n_c, ctx->scratch + 1024, p->consts + kRtSumsq, nullptr, ctx->stream));
    } else {
        HIP_TRY(hipMemsetAsync(p->consts + kRtSumsq, 0, sizeof(double), ctx->stream));
    }
    if (!counts_done) {
        HIP_TRY(dmf::launch_f32_residual_max(p->D, N * S, ctx->scratch + 2048, p->consts + kF32ResidualMax, ctx->stream));
        HIP_TRY(dmf::launch_int_count_max(p->D, N * S, ctx->scratch + 3072, p->consts + kIntCountMax, ctx->stream));
        if (n_c > 0) {
            HIP_TRY(dmf::launch_unit_range_check(p->Rt, N * n_c, ctx->scratch, p->consts + kRtOutsideUnit, ctx->stream));
        } else {
            HIP_TRY(hipMemsetAsync(p->consts + kRtOutsideUnit, 0, sizeof(double), ctx->stream));
        }
    }
    {
        double got[kProblemConsts];
        HIP_TRY(hipMemcpyAsync(got, p->consts, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        h[kRtSumsq] = got[kRtSumsq];
        if (!counts_done)
            for (int i = kDmax; i < kProblemConsts; ++i) h[i] = got[i];
    }
    h[kDsq] = h[kDmax] * h[kDmax];  // d = max(D)**2, deconvolution.py:197
    p->d_f32_exact = h[kF32ResidualMax] == 0.0;
    HIP_TRY(hipMemcpyAsync(p->consts, h, kProblemConsts * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (!std::isfinite(h[kDmax]) || !std::isfinite(h[kRtSumsq])) return DMF_ERR_NONFINITE;

    // integer copies of the counts (u16 row-major for the row pass, 8-bit digit planes for the integer-MFMA Gram)
    // (S <= 2048: the row pass itself stops at 512 samples; the panel producer, the integer Gram, b_u and cost kernels do not)
    if (!counts_done && ctx->generic_level == 0 && h[kIntCountMax] <= 32639.0 && h[kRtOutsideUnit] == 0.0 && S >= 2 &&
        S <= 2048 && n_c <= 48) {
        DMF_TRY(alloc_count_copies(p, h[kIntCountMax] <= 127.0 ? 1 : 2, ctx->x16, false));
        DevBuf<unsigned long long> x_stats;
        if (ctx->x16) HIP_TRY(x_stats.alloc(ctx, 3));
        HIP_TRY(dmf::launch_build_counts_int(p->D, p->V, N, (int)S, p->ND, p->D16, p->X16, p->N16, p->SD, p->Dt8,
                                             p->plane_stride, x_stats, ctx->stream));
        if (p->X16 != nullptr) {
            unsigned long long got[3] = {1, 0, 0};
            HIP_TRY(hipMemcpyAsync(got, x_stats, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            if (got[0] != 0) {  // some element is not an exact x / d: every kernel reads V
                p->X16.reset();
            } else {
                std::memcpy(&p->x16_dev, &got[1], sizeof(double));
                p->x16_sum = (double)got[2];
            }
        }
    }

    DMF_TRY(build_rowpass_images(p));

    // padded copy of R_trunc for the shape-specialised kernels (aligned, branch-free row loads)
    if (n_c > 0 && n_c <= 48) {  // (<= 16: every shape-specialised kernel; beyond: the wide-row-group producer, the integer Gram)
        const int nct = (int)((n_c + 3) / 4 * 4);
        if (nct == n_c) {
            p->Rtp.borrow(p->Rt);
        } else {
            HIP_TRY(p->Rtp.alloc(ctx, (size_t)N * nct));
            HIP_TRY(dmf::launch_pad_rows(p->Rt, p->Rtp, N, (int)n_c, nct, ctx->stream));
        }
    }

    // known block: packed triangle over the extended indices (Rt_0..Rt_{n_c-1}, v)
    const dmf::ProblemView pv = p->view();
    JobTable jobs;
    jobs.build(0, (int)n_c, [](int, int) { return true; });
    const int n_jobs = jobs.n;
    // all but the last job (v, v) are sums of row-feature products against D or D * V: the matrix-core Gram
    // kernel takes them (n_c <= 16 here: 136 + 16 jobs at most); v^T D v goes through the generic kernel alone
    const bool mfma = n_c >= 1 && ctx->generic_level != 1 && ctx->generic_level != 2;
    const int n_fast = mfma ? n_jobs - 1 : 0, n_dense = (int)(n_c * (n_c + 1) / 2);
    // With integer copies of the counts the known block takes the solver's own integer route: the dense pairs on the integer
    // matrix cores from the 8-bit planes (exact sums of fixed-point products), the right-hand sides sum_i Rt_ik d_is v_is
    // from the u16 stream kernel -- 0.26 + 2.6 GB instead of the 4.5 GB of V and the f64 counts that the FP64 matrix-core
    // kernel reads (1.5 ms at 1e6 x 256 x 12; every bootstrap replicate builds a problem).
    const bool int_known = mfma && ctx->generic_level == 0 && p->Dt8 != nullptr && p->D16 != nullptr && p->Rtp != nullptr &&
                           (reinterpret_cast<uintptr_t>(p->Rtp.get()) & 15) == 0 &&
                           dmf::gram_i8_known_supported((int)n_c, p->ND, N, p->SD);
    int64_t slab_doubles = dmf::gram_slab_doubles(N, (int)S, mfma ? 1 : n_jobs);
    if (mfma && !int_known) {
        const int64_t need = dmf::gram_mfma_slab_doubles(N, (int)S, n_fast);
        if (need > slab_doubles) slab_doubles = need;
    }
    DevBuf<double> slab, slab_bu;  // (the temporaries live until the wait at the bottom)
    DevBuf<long long> slab_i8, acc;
    HIP_TRY(p->gb_known.alloc(ctx, (size_t)n_jobs * S));
    DMF_TRY(jobs.upload(ctx));
    HIP_TRY(slab.alloc(ctx, (size_t)slab_doubles));
    bool vdv_done = true;  // (in: asked for; out: delivered)
    if (int_known) {
        const int64_t slab_words = dmf::gram_i8_slab_words_nf(N, p->SD, n_dense);
        const int64_t acc_words = dmf::gram_i8_acc_words_nf((int)S, n_dense, (int)n_c + 1);
        HIP_TRY(slab_i8.alloc(ctx, (size_t)slab_words));
        HIP_TRY(acc.alloc(ctx, (size_t)acc_words));
        HIP_TRY(slab_bu.alloc(ctx, (size_t)dmf::bu_cols_grid(N) * (n_c + 1) * S));
        HIP_TRY(hipMemsetAsync(acc, 0, (size_t)acc_words * sizeof(long long), ctx->stream));
        int ny = 0, n_slabs = 0;
        dmf::GramRan ran;
        HIP_TRY(dmf::launch_gram_i8(pv, nullptr, 0, jobs.k, jobs.l, n_dense, slab_i8, slab_words, nullptr, &ny, ctx->stream, &ran));
        known_route(p, "int_known");
        known_route(p, ran.text);
        // (v^T D v rides along where the two-samples-per-lane form of the stream kernel runs)
        HIP_TRY(dmf::launch_bu_cols(pv, p->Rt, (int)n_c, slab_bu, nullptr, &n_slabs, ctx->stream, &vdv_done));
        known_route(p, vdv_done ? "+ k_bu_cols2 with vDv" : "+ k_bu_cols");
        // (dst lists the dense pairs first, then the n_c right-hand sides, then (v, v): the order of the reduce's jobs)
        HIP_TRY(dmf::launch_gram_v2_reduce(slab_i8, ny, n_dense, p->SD, slab_bu, n_slabs, (int)n_c + (vdv_done ? 1 : 0), (int)S,
                                           acc, jobs.dst, p->gb_known, nullptr, nullptr, 0, nullptr, ctx->stream));
    } else if (mfma) {
        dmf::GramJobTable fast{jobs.k, jobs.l, jobs.dst, n_fast};
        int ny = 0;
        dmf::GramRan ran;
        HIP_TRY(dmf::launch_gram_mfma(pv, nullptr, 0, fast, n_dense, slab, slab_doubles, nullptr, &ny, ctx->stream, &ran));
        known_route(p, "fp64");
        known_route(p, ran.text);
        HIP_TRY(dmf::launch_gram_reduce(slab, ny, n_fast, (int)S, jobs.dst, p->gb_known, nullptr, ctx->stream));
    }
    if (int_known && vdv_done) {
        // (nothing left)
    } else if (n_jobs - n_fast == 1 && ctx->generic_level != 1 && ctx->generic_level != 2 &&
               (int64_t)dmf::vdv_cols_grid(N) * S <= slab_doubles) {
        // what is left is v^T D v alone: a stream kernel of its own (the generic kernel took 2.7 ms for it at 1e6 x 256)
        HIP_TRY(dmf::launch_vdv_cols(pv, slab, p->gb_known + (int64_t)jobs.h_dst[n_jobs - 1] * S, ctx->stream));
        known_route(p, p->known_ran.text[0] == 0 ? "fp64 k_vdv_cols" : "+ k_vdv_cols");
    } else {
        dmf::GramJobTable rest{jobs.k + n_fast, jobs.l + n_fast, jobs.dst + n_fast, n_jobs - n_fast};
        dmf::GramRan ran;
        if (p->known_ran.text[0] == 0) known_route(p, "fp64");
        else known_route(p, "+");
        HIP_TRY(dmf::launch_gram(pv, nullptr, 0, rest, slab, slab_doubles, p->gb_known, nullptr, ctx->stream, &ran));
        known_route(p, ran.text);
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // (the uploads of the job table read host memory of this frame)
    return DMF_OK;
}

// which kernel computes cost_f_w on this problem's data: the plan (dmf_kernels_stream.hip) of its key at the context's level
static dmf::CostPlan cost_plan_of(dmf_context* ctx, const dmf::ProblemView& p, int n_u) {
    return dmf::cost_plan(dmf::cost_key(p, n_u, ctx->generic_level));
}

hipError_t enqueue_cost(dmf_context* ctx, const dmf::ProblemView& p, const double* u, const double* alpha, int n_u,
                        double* scratch, double* out) {
    return dmf::launch_cost_plan(cost_plan_of(ctx, p, n_u), p, u, alpha, n_u, scratch, out, ctx->stream);
}

// Does enqueue_cost read the counts of this problem from D16 alone (never from the f64 D)?
bool cost_reads_u16_only(dmf_context* ctx, const dmf::ProblemView& p, int n_u) { return cost_plan_of(ctx, p, n_u).d16; }

// The streaming cost (deconvolution.py:15-17) of (u, alpha) on the problem's data into a host slot; without `wait` the
// copy is only enqueued (a page-locked slot, and the caller's event behind it).
int cost_to_host(dmf_context* ctx, const dmf::ProblemView& p, const double* u, const double* alpha, int n_u,
                 double* host_slot, bool wait) {
    {
        FamilyScope scope(ctx, DMF_KERNEL_COST);
        HIP_TRY(enqueue_cost(ctx, p, u, alpha, n_u, ctx->scratch + 1024, ctx->scratch + 3072));
    }
    HIP_TRY(hipMemcpyAsync(host_slot, ctx->scratch + 3072, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (wait) HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DMF_OK;
}

// the row gather behind both entry points; idx_dev: the index array is the caller's device array (range-checked here, on the
// device), else a host array (checked by the caller of this function; uploaded here)
static int problem_gather(dmf_context* ctx, const dmf_problem* src, const int64_t* idx, int64_t n_idx, bool idx_dev,
                          dmf_problem** out) {
    DevBuf<long long> d_idx;
    if (idx_dev) {
        DevBuf<unsigned int> d_bad;
        unsigned int h_bad = 1;
        HIP_TRY(d_bad.alloc(ctx, 1));
        HIP_TRY(dmf::launch_index_range_check(reinterpret_cast<const long long*>(idx), n_idx, src->N, d_bad, ctx->stream));
        HIP_TRY(hipMemcpyAsync(&h_bad, d_bad, sizeof(h_bad), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (h_bad != 0) return DMF_ERR_BAD_ARG;
        d_idx.borrow(reinterpret_cast<const long long*>(idx));
    } else {
        HIP_TRY(d_idx.alloc(ctx, (size_t)n_idx));
        HIP_TRY(hipMemcpyAsync(d_idx, idx, (size_t)n_idx * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    }
    ProblemPtr p(new (std::nothrow) dmf_problem());
    if (p == nullptr) return DMF_ERR_BAD_ARG;
    p->ctx = ctx;
    p->N = n_idx;
    p->S = src->S;
    p->n_c = src->n_c;
    HIP_TRY(p->V.alloc(ctx, (size_t)n_idx * p->S));
    HIP_TRY(p->D.alloc(ctx, (size_t)n_idx * p->S));
    if (p->n_c > 0) HIP_TRY(p->Rt.alloc(ctx, (size_t)n_idx * p->n_c));
    HIP_TRY(dmf::launch_gather_rows(src->V, p->V, d_idx, n_idx, p->S, ctx->stream));
    HIP_TRY(dmf::launch_gather_rows(src->D, p->D, d_idx, n_idx, p->S, ctx->stream));
    if (p->n_c > 0) HIP_TRY(dmf::launch_gather_rows(src->Rt, p->Rt, d_idx, n_idx, p->n_c, ctx->stream));
    // integer counts: the source's u16 copy is gathered too (0.5 GB instead of a rebuild from the 2 GB f64 copy) and the
    // resampled maximum comes out of the same pass; integrality / range of the counts and of R_trunc carry over from the
    // source, so none of the scans of problem_finalize has to run again
    bool counts_done = false;
    if (src->D16 != nullptr && src->ND > 0 && ctx->generic_level == 0) {
        const bool x16 = src->X16 != nullptr && ctx->x16;
        DevBuf<unsigned int> d_max;
        DevBuf<unsigned long long> d_xsum;
        DMF_TRY(alloc_count_copies(p.get(), src->ND, x16, false));
        HIP_TRY(d_max.alloc(ctx, 1));
        if (x16) HIP_TRY(d_xsum.alloc(ctx, 1));
        HIP_TRY(dmf::launch_gather_counts_int(src->D16, x16 ? src->X16.get() : nullptr, d_idx, n_idx, p->SD, p->ND, p->D16,
                                              p->X16, p->N16, p->Dt8, p->plane_stride, d_max, d_xsum, ctx->stream));
        unsigned int h_max = 0;
        unsigned long long h_xsum = 0;
        HIP_TRY(hipMemcpyAsync(&h_max, d_max, sizeof(h_max), hipMemcpyDeviceToHost, ctx->stream));
        if (x16) HIP_TRY(hipMemcpyAsync(&h_xsum, d_xsum, sizeof(h_xsum), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        p->h_consts[kDmax] = p->h_consts[kIntCountMax] = (double)h_max;
        p->h_consts[kF32ResidualMax] = src->h_consts[kF32ResidualMax];
        p->h_consts[kRtOutsideUnit] = src->h_consts[kRtOutsideUnit];
        p->x16_dev = x16 ? src->x16_dev : 0.0;  // (a bound over the source's elements: holds for any subset)
        p->x16_sum = (double)h_xsum;
        counts_done = true;
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // (a host index array belongs to the caller again from here on)
    d_idx.reset();
    DMF_TRY(problem_finalize(p.get(), counts_done));
    *out = p.release();
    return DMF_OK;
}

}  // namespace dmf_api

using namespace dmf_api;

extern "C" {

int dmf_problem_create(dmf_context* ctx, int64_t N, int64_t S, int64_t n_c, const double* V,
                       const void* counts, const double* Rt, int flags, dmf_problem** out) {
    DMF_TRY(check_ctx(ctx));
    if (out == nullptr) return DMF_ERR_BAD_ARG;
    *out = nullptr;
    if (N <= 0 || S <= 0 || n_c < 0 || V == nullptr || counts == nullptr) return DMF_ERR_BAD_ARG;
    if (n_c > 0 && Rt == nullptr) return DMF_ERR_BAD_ARG;
    if (n_c > dmf::kMaxK || S > (1 << 24)) return DMF_ERR_UNSUPPORTED;
    ProblemPtr p(new (std::nothrow) dmf_problem());
    if (p == nullptr) return DMF_ERR_BAD_ARG;
    p->ctx = ctx;
    p->N = N;
    p->S = S;
    p->n_c = n_c;
    DMF_TRY(import_array(ctx, V, (size_t)N * S, flags, p->V));
    if (flags & DMF_COUNTS_F64) {
        DMF_TRY(import_array(ctx, counts, (size_t)N * S, flags, p->D));
    } else {
        DevBuf<long long> raw;
        DMF_TRY(import_array(ctx, counts, (size_t)N * S, flags, raw));
        HIP_TRY(p->D.alloc(ctx, (size_t)N * S));
        HIP_TRY(dmf::launch_convert_counts(raw, p->D, N * S, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    DMF_TRY(import_array(ctx, Rt, (size_t)N * n_c, flags, p->Rt));
    DMF_TRY(problem_finalize(p.get()));
    *out = p.release();
    return DMF_OK;
}

int dmf_problem_gather(dmf_context* ctx, const dmf_problem* src, const int64_t* idx, int64_t n_idx,
                       dmf_problem** out) {
    DMF_TRY(check_ctx(ctx));
    if (src == nullptr || idx == nullptr || out == nullptr || n_idx <= 0) return DMF_ERR_BAD_ARG;
    *out = nullptr;
    if (src->mask_bits != nullptr) return DMF_ERR_BAD_ARG;  // (the mask is not carried through a row gather)
    for (int64_t r = 0; r < n_idx; ++r)
        if (idx[r] < 0 || idx[r] >= src->N) return DMF_ERR_BAD_ARG;
    return problem_gather(ctx, src, idx, n_idx, false, out);
}

int dmf_problem_gather_device(dmf_context* ctx, const dmf_problem* src, const int64_t* idx_dev, int64_t n_idx,
                              dmf_problem** out) {
    DMF_TRY(check_ctx(ctx));
    if (src == nullptr || idx_dev == nullptr || out == nullptr || n_idx <= 0) return DMF_ERR_BAD_ARG;
    *out = nullptr;
    if (src->mask_bits != nullptr) return DMF_ERR_BAD_ARG;
    return problem_gather(ctx, src, idx_dev, n_idx, true, out);
}

// The masked copy of a resident problem, modelled on problem_gather: one pass over the rows writes the masked V, D, D16 and
// X16 and the hold-out weights and returns max(kept counts), the sum of the kept x and the number of held-out elements; the
// digit planes are rebuilt from the new D16; integrality / range of the counts and of R_trunc carry over from the source,
// so none of the scans of problem_finalize runs again.
int dmf_problem_mask(dmf_context* ctx, const dmf_problem* src, const uint8_t* train_bits, int flags, dmf_problem** out) {
    DMF_TRY(check_ctx(ctx));
    if (src == nullptr || train_bits == nullptr || out == nullptr) return DMF_ERR_BAD_ARG;
    *out = nullptr;
    if (src->ctx != ctx || src->mask_bits != nullptr) return DMF_ERR_BAD_ARG;
    ProblemPtr p(new (std::nothrow) dmf_problem());
    if (p == nullptr) return DMF_ERR_BAD_ARG;
    const int64_t N = src->N, S = src->S, n_c = src->n_c;
    p->ctx = ctx;
    p->N = N;
    p->S = S;
    p->n_c = n_c;
    const size_t bit_bytes = (size_t)N * (size_t)((S + 7) / 8), elems = (size_t)N * S;
    HIP_TRY(p->mask_bits.alloc(ctx, bit_bytes));
    HIP_TRY(hipMemcpyAsync(p->mask_bits, train_bits, bit_bytes,
                           (flags & DMF_PTR_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(p->V.alloc(ctx, elems));
    HIP_TRY(p->D.alloc(ctx, elems));
    if (n_c > 0) {
        HIP_TRY(p->Rt.alloc(ctx, (size_t)N * n_c));
        HIP_TRY(hipMemcpyAsync(p->Rt, src->Rt, (size_t)N * n_c * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    }
    const bool ints = src->D16 != nullptr && src->ND > 0 && ctx->generic_level == 0;
    const bool x16 = ints && src->X16 != nullptr && ctx->x16;
    if (ints) DMF_TRY(alloc_count_copies(p.get(), src->ND, x16, true));
    DevBuf<unsigned long long> d_stats;
    HIP_TRY(d_stats.alloc(ctx, 3));
    HIP_TRY(dmf::launch_mask_problem(src->V, src->D, ints ? src->D16.get() : nullptr, x16 ? src->X16.get() : nullptr,
                                     p->mask_bits, p->V, p->D, p->D16, p->X16, p->W16, N, p->N16, (int)S, p->SD, d_stats,
                                     ctx->stream));
    if (ints) HIP_TRY(dmf::launch_build_dt8(p->D16, N, p->SD, p->ND, p->Dt8, p->plane_stride, ctx->stream));
    unsigned long long h_stats[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h_stats, d_stats, sizeof(h_stats), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // (a host mask belongs to the caller again from here on)
    d_stats.reset();
    double dmax;
    std::memcpy(&dmax, &h_stats[0], sizeof(dmax));
    p->h_consts[kDmax] = dmax;
    p->h_consts[kF32ResidualMax] = src->h_consts[kF32ResidualMax];
    p->h_consts[kIntCountMax] = std::isfinite(src->h_consts[kIntCountMax]) ? dmax : src->h_consts[kIntCountMax];
    p->h_consts[kRtOutsideUnit] = src->h_consts[kRtOutsideUnit];
    p->x16_dev = x16 ? src->x16_dev : 0.0;  // (a bound over the source's elements: holds for any subset)
    p->x16_sum = (double)h_stats[1];
    p->n_test = (int64_t)h_stats[2];
    DMF_TRY(problem_finalize(p.get(), true));
    *out = p.release();
    return DMF_OK;
}

// (the buffers go back to the context's pool with the members that own them)
int dmf_problem_destroy(dmf_problem* p) {
    if (p == nullptr) return DMF_OK;
    hipSetDevice(p->ctx->device);
    delete p;
    return DMF_OK;
}

int dmf_problem_cost_describe(dmf_context* ctx, const dmf_problem* p, int64_t n_u, char* buf, int64_t cap) {
    if (ctx == nullptr || p == nullptr || buf == nullptr || cap < 1 || n_u < 0 || p->ctx != ctx) return DMF_ERR_BAD_ARG;
    if (p->n_c + n_u < 1 || p->n_c + n_u > dmf::kMaxK) return DMF_ERR_BAD_ARG;
    dmf::describe_cost_plan(cost_plan_of(ctx, p->view(), (int)n_u), buf, (size_t)cap);
    return DMF_OK;
}

int dmf_problem_gram_known(const dmf_problem* p, double* out, char* out_text, int64_t cap) {
    if (p == nullptr || out == nullptr || (out_text != nullptr && cap < 1)) return DMF_ERR_BAD_ARG;
    dmf_context* ctx = p->ctx;
    DMF_TRY(check_ctx(ctx));
    const size_t n = (size_t)(p->n_c + 1) * (p->n_c + 2) / 2 * p->S;
    HIP_TRY(hipMemcpyAsync(out, p->gb_known, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (out_text != nullptr) snprintf(out_text, (size_t)cap, "%s", p->known_ran.text);
    return DMF_OK;
}

int dmf_problem_report(const dmf_problem* p, int64_t* out_ints, double* out_dbls) {
    if (p == nullptr || out_ints == nullptr || out_dbls == nullptr) return DMF_ERR_BAD_ARG;
    const int64_t rtp_width = p->Rtp != nullptr ? (p->n_c + 3) / 4 * 4 : 0;
    const int64_t ints[DMF_REPORT_INTS] = {p->N, p->S, p->n_c, p->ND, p->SD, p->N16, p->plane_stride,
                                           p->D16 != nullptr, p->X16 != nullptr, p->W16 != nullptr, p->Dt8 != nullptr,
                                           p->mask_bits != nullptr, rtp_width,
                                           p->Rtp != nullptr && p->Rtp.get() == p->Rt.get(), p->n_test, p->d_f32_exact};
    std::memcpy(out_ints, ints, sizeof(ints));
    for (int i = 0; i < kProblemConsts; ++i) out_dbls[i] = p->h_consts[i];
    out_dbls[kProblemConsts] = p->x16_dev;
    out_dbls[kProblemConsts + 1] = p->x16_sum;
    return DMF_OK;
}

int dmf_problem_copy_out(const dmf_problem* p, int which, void* out, int64_t bytes) {
    if (p == nullptr || out == nullptr) return DMF_ERR_BAD_ARG;
    dmf_context* ctx = p->ctx;
    DMF_TRY(check_ctx(ctx));
    const size_t elems = (size_t)p->N * p->S, u16_bytes = (size_t)p->N16 * p->SD * sizeof(unsigned short);
    const void* src = nullptr;
    size_t size = 0;
    switch (which) {
        case DMF_ARRAY_V: src = p->V, size = elems * sizeof(double); break;
        case DMF_ARRAY_D: src = p->D, size = elems * sizeof(double); break;
        case DMF_ARRAY_RT: src = p->Rt, size = (size_t)p->N * p->n_c * sizeof(double); break;
        case DMF_ARRAY_RTP: src = p->Rtp, size = (size_t)p->N * ((p->n_c + 3) / 4 * 4) * sizeof(double); break;
        case DMF_ARRAY_D16: src = p->D16, size = u16_bytes; break;
        case DMF_ARRAY_X16: src = p->X16, size = u16_bytes; break;
        case DMF_ARRAY_W16: src = p->W16, size = u16_bytes; break;
        case DMF_ARRAY_DT8: src = p->Dt8, size = (size_t)p->plane_stride * p->ND; break;
        case DMF_ARRAY_MASK_BITS: src = p->mask_bits, size = (size_t)p->N * (size_t)((p->S + 7) / 8); break;
        case DMF_ARRAY_CONSTS: src = p->consts, size = kProblemConsts * sizeof(double); break;
        case DMF_ARRAY_X8: src = p->X8, size = (size_t)p->N16 * p->SD; break;
        case DMF_ARRAY_D8: src = p->D8, size = (size_t)p->N16 * p->SD; break;
        default: return DMF_ERR_BAD_ARG;
    }
    if (src == nullptr || size == 0) return DMF_ERR_BAD_ARG;
    if (bytes < 0 || (size_t)bytes != size) return DMF_ERR_BAD_SHAPE;
    return export_array(ctx, src, size, 0, out);
}

int dmf_problem_has_byte_images(const dmf_problem* p, int* out) {
    if (p == nullptr || out == nullptr) return DMF_ERR_BAD_ARG;
    *out = p->X8 != nullptr && p->D8 != nullptr;
    return DMF_OK;
}

int dmf_rowpass_image_offset(int row, int sample) {
    if (row < 0 || row > 15 || sample < 0 || sample > 63) return -1;
    return dmf::rowpass_image_byte(row, sample);
}

int dmf_problem_shape(const dmf_problem* p, int64_t* N, int64_t* S, int64_t* n_c) {
    if (p == nullptr) return DMF_ERR_BAD_ARG;
    if (N) *N = p->N;
    if (S) *S = p->S;
    if (n_c) *n_c = p->n_c;
    return DMF_OK;
}

}  // extern "C"
