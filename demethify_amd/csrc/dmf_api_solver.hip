// C-ABI of libdemethify_hip.so, part 3: solvers -- set-up, the outer-loop driver with its stop test, and dmf_solve.
#include "dmf_api.h"

namespace dmf_api {

using dmf::kSplitInnerSteps;

// scratch of the split u phase: per-row c_i / M_i and the momentum coefficients of the inner steps (allocated on first use)
static int ensure_split_scratch(dmf_solver* s, int n_iter2) {
    dmf_context* ctx = s->ctx;
    if (s->cm == nullptr) HIP_TRY(s->cm.alloc(ctx, (size_t)dmf::u_phase_split_cm_doubles(s->p->N, (int)s->n_u)));
    if (s->beta_cap < n_iter2 || s->beta_tab == nullptr) {
        s->beta_cap = n_iter2 > 0 ? n_iter2 : 1;
        HIP_TRY(s->beta_tab.alloc(ctx, (size_t)s->beta_cap));
    }
    return DMF_OK;
}

int enqueue_u_phase(dmf_solver* s, int n_iter2, dmf::RowKind row) {
    dmf_context* ctx = s->ctx;
    const dmf::ProblemView pv = s->p->view();
    FamilyScope scope(ctx, DMF_KERNEL_ROWPASS);
    switch (row) {
        case dmf::RowKind::CmI8InnerRows:
            // wide row groups on u16 counts: per-row c_i / M_i with M_i on the integer matrix cores, then the inner
            // iterations chip-wide (dmf_kernels_cm_i8.hip)
            DMF_TRY(ensure_split_scratch(s, n_iter2));
            HIP_TRY(dmf::launch_u_phase_split_i8(pv, s->iterate(), n_iter2, s->scratch(), ctx->stream));
            return DMF_OK;
        case dmf::RowKind::UPhaseBig:
            HIP_TRY(dmf::launch_u_phase_big(pv, s->iterate(), n_iter2, ctx->stream));
            return DMF_OK;
        case dmf::RowKind::UPhaseMfmaSplit:
            // many inner steps or wide row groups: one wave per workgroup running the inner steps is the bottleneck
            DMF_TRY(ensure_split_scratch(s, n_iter2));
            HIP_TRY(dmf::launch_u_phase_split(pv, s->iterate(), n_iter2, s->scratch(), ctx->stream));
            return DMF_OK;
        case dmf::RowKind::UPhaseMfma:
            HIP_TRY(dmf::launch_u_phase_mfma(pv, s->iterate(), n_iter2, ctx->stream));
            return DMF_OK;
        case dmf::RowKind::UPhaseGram:
            HIP_TRY(dmf::launch_u_phase_gram(pv, s->iterate(), n_iter2, ctx->stream));
            return DMF_OK;
        case dmf::RowKind::UStepDirect:
            for (int t = 0; t < n_iter2; ++t) {
                HIP_TRY(dmf::launch_u_step_direct(pv, s->iterate(), s->u_next, t, ctx->stream));
                std::swap(s->u_prev, s->u);   // (u_prev <- u, u <- u_next, u_next <- the old u_prev)
                std::swap(s->u, s->u_next);
            }
            return DMF_OK;
        default: return DMF_ERR_BAD_ARG;  // (the one-launch row passes are enqueue_outer_iteration's)
    }
}

// the row kind of a u phase that runs as a kernel of its own (the single-function entry points: dmf_update_u)
dmf::RowKind standalone_row_kind(const dmf_solver* s, int n_iter2) {
    return dmf::plan_iteration(s->key, dmf::standalone_spec(s->spec), n_iter2, false).row;
}

// What the integer Gram route of a solver writes and works in: the solver's own buffers in the loop, temporaries of the
// same sizes for dmf_solver_gram on a solver whose path never allocated them.
struct GramI8Buffers {
    double* slab_bu = nullptr;     // b_u slabs: bu_cols_grid(N) x n_u x S doubles (or what the row kernel left there)
    long long* slab_i8 = nullptr;  // gram_i8_slab_words() i64 words
    int64_t slab_i8_words = 0;
    long long* acc = nullptr;      // gram_i8_acc_words() i64 words, zero (the kernels leave them zero again)
    double* gb = nullptr;          // the packed Gram the rows go to
    const int* done = nullptr;     // the solver's done flag, or null: compute whatever the flag says
};

static GramI8Buffers solver_i8_buffers(dmf_solver* s) {
    GramI8Buffers b;
    b.slab_bu = s->slab, b.slab_i8 = s->slab_i8, b.slab_i8_words = s->slab_i8_words, b.acc = s->acc_i8, b.gb = s->gb;
    b.done = &s->state->done;
    return b;
}

// The integer Gram of the u-dependent entries on the 8-bit count planes and its reduce, which also folds in the b_u
// slabs (`n_slabs` of them in b.slab_bu) and, where the row kernel left them, `n_u2` shares of ||u||^2.
static int gram_i8_and_reduce(dmf_solver* s, const GramI8Buffers& b, int n_slabs, const double* u2_partials, int n_u2,
                              dmf::GramRan* ran = nullptr) {
    dmf_context* ctx = s->ctx;
    const dmf_problem* p = s->p;
    const int S = (int)p->S, n_c = (int)p->n_c, n_u = (int)s->n_u, nf = n_c * n_u + n_u * (n_u + 1) / 2;
    int ny = 0;
    HIP_TRY(dmf::launch_gram_i8(p->view(), s->u, n_u, s->jobs.k, s->jobs.l, nf, b.slab_i8, b.slab_i8_words, b.done, &ny,
                                ctx->stream, ran));
    HIP_TRY(dmf::launch_gram_v2_reduce(b.slab_i8, ny, nf, p->SD, b.slab_bu, n_slabs, n_u, S, b.acc, s->jobs.dst, b.gb, b.done,
                                       u2_partials, n_u2, s->state, ctx->stream));
    return DMF_OK;
}

// b_u by the stream kernel, then the integer Gram and its reduce: GramKind::BuColsI8
static int gram_bu_cols_i8(dmf_solver* s, const GramI8Buffers& b, dmf::GramRan* ran = nullptr) {
    int n_slabs = 0;
    HIP_TRY(dmf::launch_bu_cols(s->p->view(), s->u, (int)s->n_u, b.slab_bu, b.done, &n_slabs, s->ctx->stream));
    return gram_i8_and_reduce(s, b, n_slabs, nullptr, 0, ran);
}

// kind: GramKind::BuColsI8 only behind a u phase with at least one inner step (its clip puts u inside [0, 1], which the
// fixed-point features need); the dmf_update_alpha entry point hands over the caller's u and passes an FP64 kind
int enqueue_gram(dmf_solver* s, dmf::GramKind kind, bool heed_done, dmf::GramRan* ran) {
    dmf_context* ctx = s->ctx;
    const dmf::ProblemView pv = s->p->view();
    const int S = pv.S, n_u = (int)s->n_u;
    const int* done = heed_done ? &s->state->done : nullptr;
    FamilyScope scope(ctx, DMF_KERNEL_GRAM);
    if (kind == dmf::GramKind::BuColsI8) {
        GramI8Buffers b = solver_i8_buffers(s);
        b.done = done;
        return gram_bu_cols_i8(s, b, ran);
    }
    if (kind == dmf::GramKind::GramU) {
        int ny = 0;
        HIP_TRY(dmf::launch_gram_u(pv, s->u, n_u, s->slab, done, &ny, ctx->stream, ran));
        HIP_TRY(dmf::launch_gram_reduce(s->slab, ny, s->jobs.n, S, s->jobs.dst, s->gb, done, ctx->stream));
        return DMF_OK;
    }
    dmf::GramJobTable jobs{s->jobs.k, s->jobs.l, s->jobs.dst, s->jobs.n};
    if (kind == dmf::GramKind::GramMfma) {
        int ny = 0;
        HIP_TRY(dmf::launch_gram_mfma(pv, s->u, n_u, jobs, s->jobs.n - n_u, s->slab, s->slab_doubles, done, &ny, ctx->stream, ran));
        HIP_TRY(dmf::launch_gram_reduce(s->slab, ny, s->jobs.n, S, s->jobs.dst, s->gb, done, ctx->stream));
        return DMF_OK;
    }
    HIP_TRY(dmf::launch_gram(pv, s->u, n_u, jobs, s->slab, s->slab_doubles, s->gb, done, ctx->stream, ran));
    return DMF_OK;
}

dmf::GramKind fp64_gram_kind(const dmf_solver* s) {
    return s->spec.use_gram_spec ? dmf::GramKind::GramU : s->spec.use_gram_mfma ? dmf::GramKind::GramMfma : dmf::GramKind::Gram;
}

int enqueue_alpha_phase(dmf_solver* s, dmf::AlphaKind kind, int n_iter2) {
    FamilyScope scope(s->ctx, DMF_KERNEL_ALPHA);
    HIP_TRY(dmf::launch_alpha(kind, s->alpha_view(), n_iter2, s->ctx->stream));
    return DMF_OK;
}

// Where the loop records what wrote its Gram (dmf_solver::last_gram, for DMF_GRAM_LAST) -- or null while the source is
// the one already recorded: on one solver the text of a source does not change, and the loop formats nothing per iteration.
constexpr int kLastGramI8Tail = 100, kLastGramFused = 101;  // (other sources: the GramKind of enqueue_gram)
static dmf::GramRan* last_gram_slot(dmf_solver* s, int source) {
    if (s->last_gram_source == source) return nullptr;
    s->last_gram_source = source;
    return &s->last_gram;
}

// what follows a row kernel that left `grid` b_u slabs and ||u||^2 shares: the integer Gram, its reduce, the alpha phase
static int enqueue_gram_i8_tail(dmf_solver* s, dmf::AlphaKind alpha, int n_iter2, int grid) {
    {
        FamilyScope scope(s->ctx, DMF_KERNEL_GRAM);
        DMF_TRY(gram_i8_and_reduce(s, solver_i8_buffers(s), grid, s->u2_partials, grid, last_gram_slot(s, kLastGramI8Tail)));
    }
    return enqueue_alpha_phase(s, alpha, n_iter2);
}

static int enqueue_outer_iteration(dmf_solver* s, int n_iter2) {
    dmf_context* ctx = s->ctx;
    s->in_flight = true;
    const dmf_problem* p = s->p;
    const int S = (int)p->S;
    // which kernels: dmf_select.hip (one table for create / enqueue / describe)
    const dmf::IterationPlan plan = dmf::plan_iteration(s->key, s->spec, n_iter2, s->purity != nullptr);
    if (plan.row == dmf::RowKind::RowpassV2) {
        // Second generation: one read of V (f64) -- or of the u16 methylated read counts X16 -- and of the u16 counts for
        // the u phase and b_u, then the exact
        // integer-matrix-core GEMM for the u-dependent Gram entries on the 8-bit count planes.
        const dmf::RowpassV2Plan rp = dmf::rowpass_v2_plan(s->key, n_iter2);
        {
            FamilyScope scope(ctx, DMF_KERNEL_ROWPASS);
            HIP_TRY(dmf::launch_rowpass_v2(p->view(), s->iterate(), n_iter2, s->scratch(), rp, ctx->stream));
            for (int i = 0; i <= (int)rp.schedule(); ++i) ++s->n_rowpass[i];  // (each schedule is a form of the one before)
        }
        return enqueue_gram_i8_tail(s, plan.alpha, n_iter2, rp.grid);
    }
    if (plan.row == dmf::RowKind::CmI8InnerBu) {
        // Wide row groups on u16 counts: c_i / M_i (M_i on the integer matrix cores), then the inner iterations fused with
        // the b_u stream and the ||u||^2 shares, then the integer Gram and its reduce -- four launches + the momentum table.
        int grid = 0;
        DMF_TRY(ensure_split_scratch(s, n_iter2));
        {
            FamilyScope scope(ctx, DMF_KERNEL_ROWPASS);
            HIP_TRY(dmf::launch_u_phase_split_i8_bu(p->view(), s->iterate(), n_iter2, s->scratch(), &grid, ctx->stream));
        }
        return enqueue_gram_i8_tail(s, plan.alpha, n_iter2, grid);
    }
    if (plan.row == dmf::RowKind::RowpassFused) {
        // The fused kernel takes whole 16-row blocks; a ragged tail (< 16 rows) goes through the unfused
        // pair on the rows' own views and contributes extra slab rows and one more ||u||^2 share.
        const int64_t n_full = p->N - (p->N & 15), n_tail = p->N - n_full;
        const dmf::ProblemView pv = p->view();
        int grid = 0, ny_tail = 0;
        {
            FamilyScope scope(ctx, DMF_KERNEL_ROWPASS);
            HIP_TRY(dmf::launch_rowpass_fused(pv.rows(0, n_full), s->iterate(), n_iter2, s->scratch(), &grid, ctx->stream));
        }
        if (n_tail > 0) {
            const dmf::ProblemView tail = pv.rows(n_full, n_tail);
            const dmf::IterateView it_tail = s->iterate().rows(n_full);
            HIP_TRY(dmf::launch_u_phase_mfma(tail, it_tail, n_iter2, ctx->stream));
            HIP_TRY(dmf::launch_sumsq_f64(it_tail.u, n_tail * s->n_u, ctx->scratch, s->u2_partials + grid, &s->state->done,
                                          ctx->stream));
            HIP_TRY(dmf::launch_gram_u(tail, it_tail.u, it_tail.n_u, s->slab + (int64_t)2 * grid * s->jobs.n * S,
                                       &s->state->done, &ny_tail, ctx->stream));
        }
        if (dmf::GramRan* ran = last_gram_slot(s, kLastGramFused))
            snprintf(ran->text, sizeof(ran->text), "k_rowpass_fused<%d,%d> phase C slabs=%d%s", (int)(p->n_c + 3) / 4, (int)s->n_u,
                     2 * grid, n_tail > 0 ? " + k_gram_u tail" : "");
        HIP_TRY(dmf::launch_finish_u_norm(s->u2_partials, grid + (n_tail > 0 ? 1 : 0), s->state, ctx->stream));
        {
            FamilyScope scope(ctx, DMF_KERNEL_GRAM);
            HIP_TRY(dmf::launch_gram_reduce(s->slab, 2 * grid + ny_tail, s->jobs.n, S, s->jobs.dst, s->gb,
                                            &s->state->done, ctx->stream));
        }
        return enqueue_alpha_phase(s, plan.alpha, n_iter2);
    }
    DMF_TRY(enqueue_u_phase(s, n_iter2, plan.row));
    HIP_TRY(dmf::launch_sumsq_f64(s->u, p->N * s->n_u, ctx->scratch, &s->state->u_norm2, &s->state->done,
                                  ctx->stream));
    HIP_TRY(dmf::launch_set_lh(s->state, ctx->stream));
    DMF_TRY(enqueue_gram(s, plan.gram, true, last_gram_slot(s, (int)plan.gram)));
    return enqueue_alpha_phase(s, plan.alpha, n_iter2);
}

int fetch_state(dmf_solver* s) {
    HIP_TRY(hipMemcpyAsync(s->h_state, s->state, sizeof(SolverState), hipMemcpyDeviceToHost, s->ctx->stream));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    s->in_flight = false;
    return DMF_OK;
}

int push_state(dmf_solver* s) {
    HIP_TRY(hipMemcpyAsync(s->state, s->h_state, sizeof(SolverState), hipMemcpyHostToDevice, s->ctx->stream));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    return DMF_OK;
}

constexpr int kMomRows = 64, kMomSteps = 64;  // momentum rows per upload (= the largest batch), inner steps a row can hold

__global__ void k_set_momentum(SolverState* state, const double* mom, int stride, int rows, int n) {
    state->mom = mom;
    state->mom_stride = stride;
    state->mom_rows = rows;
    state->mom_i = 0;
    state->mom_n = n;
}

// Runs the momentum recurrence (deconvolution.py:83-84 / :95-96: a <- (1 + sqrt(1 + 4 a^2)) / 2, and the ratio
// (a_old - 1) / a that beta is the minimum of) ahead for `rows` outer iterations of n inner steps each, from the
// solver's current (a1, a2), and uploads the rows; the kernels of those iterations read them instead of running the
// recurrence themselves.  Plain IEEE double arithmetic, as numpy's in the reference (no contraction on the host).
static double momentum_advance(double& a) {  // a <- next a; returns (a_old - 1) / a_new
#pragma clang fp contract(off)
    const double a0 = a;
    const double sq = 4.0 * a0 * a0;
    a = (1.0 + std::sqrt(1.0 + sq)) / 2.0;
    return (a0 - 1.0) / a;
}

static int upload_momentum_rows(dmf_solver* s, int rows, int n) {
    dmf_context* ctx = s->ctx;
    const int stride = 2 + 2 * n;
    if (s->mom_host == nullptr) {
        if (!ctx->pinned_moms.empty()) {
            s->mom_host = ctx->pinned_moms.back();
            ctx->pinned_moms.pop_back();
        } else {
            HIP_TRY(hipHostMalloc((void**)&s->mom_host, (size_t)kMomRows * (2 + 2 * kMomSteps) * sizeof(double)));
        }
        HIP_TRY(s->mom_dev.alloc(ctx, (size_t)kMomRows * (2 + 2 * kMomSteps)));
    }
    double a1 = s->h_state->a1, a2 = s->h_state->a2;
    for (int r = 0; r < rows; ++r) {
        double* row = s->mom_host + (size_t)r * stride;
        for (int t = 0; t < n; ++t) {
            row[2 + t] = momentum_advance(a1);
            row[2 + n + t] = momentum_advance(a2);
        }
        row[0] = a1;
        row[1] = a2;
    }
    HIP_TRY(hipMemcpyAsync(s->mom_dev, s->mom_host, (size_t)rows * stride * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_set_momentum, dim3(1), dim3(1), 0, ctx->stream, s->state.get(), (const double*)s->mom_dev.get(), stride,
                       rows, n);
    HIP_TRY(hipGetLastError());
    return DMF_OK;
}

// tol and the band factor of this step() call: the closing kernel pauses (done = 2) when |cf - cf_0| < band x tol
// with band > 1, and stops (done = 1) when band == 1
__global__ void k_set_tol(SolverState* state, double tol, double band) {
    state->tol = tol;
    state->band = band;
}

constexpr double kConfirmBand = 10.0;       // Gram-form differences below this multiple of tol are decided on streaming costs
// Bound of the Gram-form cost's absolute error per unit of N S max(D).  Measured at 1e6 x 256, 12 + 4 against the streaming
// cost of the same iterate (tests/test_gpu_stop_test.py): 1.4e-6 at depth 120, 9e-6 at depth 1000, 4e-6 at depth 2500,
// i.e. at most 3.2e-17 N S max(D); thirty times that is the bound.
constexpr double kGramCostRelErr = 1e-15;

// the page-locked slot behind h_state that dmf_solver_cost_begin's result arrives in
static double* cost_slot(const dmf_solver* s) {
    return reinterpret_cast<double*>(reinterpret_cast<char*>(s->h_state) + kPinnedStateBytes - 16);
}

// The set-up of dmf_solver_create once the solver exists: whatever fails here, the caller's owner destroys the solver.
static int solver_setup(dmf_solver* s, const double* u0, const double* alpha0, int flags) {
    dmf_context* ctx = s->ctx;
    const dmf_problem* p = s->p;
    const int64_t N = p->N, S = p->S, n_c = p->n_c, n_u = s->n_u, K = n_c + n_u;
    // ---- kernel selection: a pure function of this key (dmf_select.hip)
    dmf::ShapeKey& key = s->key;
    key.N = N;
    key.S = (int)S;
    key.n_c = (int)n_c;
    key.n_u = (int)n_u;
    key.nd = (p->ND > 0 && p->D16 != nullptr) ? p->ND : 0;
    key.SD = p->SD;
    key.x16 = key.nd > 0 && p->X16 != nullptr;
    key.rowpass_pair = ctx->rowpass_pair;
    key.rowpass_defer_c = ctx->rowpass_defer_c;
    key.rowpass_bytes = ctx->rowpass_bytes;
    key.x_byte = key.x16 && dmf::rowpass_v2_counts_fit_bytes(p->h_consts[kIntCountMax]);  // (0 <= x <= d for every element of X16)
    key.level = ctx->generic_level;
    key.d_f32_exact = p->d_f32_exact;
    key.rtp_present = n_c == 0 || p->Rtp != nullptr;
    key.v_align = (unsigned)(reinterpret_cast<uintptr_t>(p->V.get()) & 15);
    key.rtp_align = (unsigned)(reinterpret_cast<uintptr_t>(p->Rtp.get()) & 15);
    key.alpha_unit = true;
    s->spec = dmf::select_path(key);
    if ((s->spec.use_v2 || s->spec.use_cm_i8) && !(flags & DMF_INIT_IN_UNIT_RANGE)) {
        // the integer row kernels write alpha_j alpha_l in fixed point on [0, 1]: true of every iterate (columns on the
        // simplex), checked for the caller's starting point -- in place for a host array, by a kernel for a device array
        // (callers that know where their alpha0 comes from say so with DMF_INIT_IN_UNIT_RANGE and skip the round trip)
        bool in_unit = true;
        if (flags & DMF_PTR_DEVICE) {
            double outside = 0.0;
            HIP_TRY(dmf::launch_unit_range_check(alpha0, K * S, ctx->scratch, ctx->scratch + 2048, ctx->stream));
            HIP_TRY(hipMemcpyAsync(&outside, ctx->scratch + 2048, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            in_unit = outside == 0.0;
        } else {
            for (int64_t i = 0; i < K * S; ++i)
                if (!(alpha0[i] >= 0.0 && alpha0[i] <= 1.0)) {
                    in_unit = false;
                    break;
                }
        }
        if (!in_unit) {
            key.alpha_unit = false;
            s->spec = dmf::select_path(key);
        }
    }
    if (!s->spec.supported) return DMF_ERR_UNSUPPORTED;
    s->in_flight = true;  // (from here on the solver has work on the stream)
    s->jobs.build((int)n_c, (int)K, [n_c, K](int k, int l) {
        if (l == (int)K && k < (int)n_c) return false;  // b of the known types is constant
        return !(l == (int)K && k == (int)K);           // v^T D v is constant
    });
    const int n_jobs = s->jobs.n;
    s->slab_doubles = dmf::gram_slab_doubles(N, (int)S, n_jobs);
    if (s->spec.use_gram_spec) {
        const int64_t spec = dmf::gram_u_slab_doubles(N, (int)S, (int)n_c, (int)n_u);
        if (spec > s->slab_doubles) s->slab_doubles = spec;
    }
    if (s->spec.use_gram_mfma) {
        const int64_t need = dmf::gram_mfma_slab_doubles(N, (int)S, n_jobs);
        if (need > s->slab_doubles) s->slab_doubles = need;
    }
    if (s->spec.use_fused) {
        const int64_t spec = dmf::rowpass_fused_slab_doubles(N - (N & 15), (int)S, (int)n_c, (int)n_u) +
                             dmf::gram_u_slab_doubles(16, (int)S, (int)n_c, (int)n_u);  // + ragged tail rows
        if (spec > s->slab_doubles) s->slab_doubles = spec;
    }
    if (s->spec.use_v2) {
        const int64_t bu = (int64_t)dmf::rowpass_v2_plan(key, dmf::kSizingInnerSteps).grid * n_u * S;  // (the same at every step count)
        if (bu > s->slab_doubles) s->slab_doubles = bu;
    }
    if (s->spec.use_gram_i8) {
        const int64_t bu = (int64_t)dmf::bu_cols_grid(N) * n_u * S;
        if (bu > s->slab_doubles) s->slab_doubles = bu;
        if (s->spec.use_cm_i8) {  // k_inner_bu writes one slab per workgroup
            const int64_t bu2 = (int64_t)dmf::u_inner_bu_grid(N, (int)S) * n_u * S;
            if (bu2 > s->slab_doubles) s->slab_doubles = bu2;
        }
    }
    const size_t un = (size_t)N * n_u, an = (size_t)K * S;  // (elements)
    const size_t un_alloc = (un + 1) & ~(size_t)1;  // the integer Gram kernel fetches u in 16-byte pieces
    const size_t gbn = (size_t)(K + 1) * (K + 2) / 2 * S;
    const int nb_alpha = (int)((S + 63) / 64);
    HIP_TRY(s->u.alloc(ctx, un_alloc));
    HIP_TRY(s->u_prev.alloc(ctx, un_alloc));
    if (s->spec.u_path == 2) HIP_TRY(s->u_next.alloc(ctx, un_alloc));
    HIP_TRY(s->alpha.alloc(ctx, an));
    HIP_TRY(s->alpha_prev.alloc(ctx, an));
    HIP_TRY(s->gb.alloc(ctx, gbn));
    HIP_TRY(s->slab.alloc(ctx, (size_t)s->slab_doubles));
    HIP_TRY(s->partials.alloc(ctx, (size_t)2 * (nb_alpha + S)));
    HIP_TRY(s->u2_partials.alloc(ctx, 4096));
    if (s->spec.use_v2 || s->spec.use_gram_i8) {
        s->slab_i8_words = dmf::gram_i8_slab_words(N, p->SD, (int)n_c, (int)n_u);
        HIP_TRY(s->slab_i8.alloc(ctx, (size_t)s->slab_i8_words));
        const size_t acc_words = (size_t)dmf::gram_i8_acc_words((int)S, (int)n_c, (int)n_u);
        HIP_TRY(s->acc_i8.alloc(ctx, acc_words));
        HIP_TRY(hipMemsetAsync(s->acc_i8, 0, acc_words * sizeof(long long), ctx->stream));
    }
    HIP_TRY(s->state.alloc(ctx, 1));
    if (!ctx->pinned_states.empty()) {
        s->h_state = (SolverState*)ctx->pinned_states.back();
        ctx->pinned_states.pop_back();
    } else {
        HIP_TRY(hipHostMalloc((void**)&s->h_state, kPinnedStateBytes));  // (state mirror + the cost slot of cost_begin / cost_end)
    }
    const hipMemcpyKind in_kind = (flags & DMF_PTR_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIP_TRY(hipMemsetAsync(s->state, 0, sizeof(SolverState), ctx->stream));
    HIP_TRY(hipMemsetAsync(s->gb, 0, gbn * sizeof(double), ctx->stream));
    HIP_TRY(hipMemcpyAsync(s->u, u0, un * sizeof(double), in_kind, ctx->stream));
    HIP_TRY(hipMemcpyAsync(s->u_prev, s->u, un * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(s->alpha, alpha0, an * sizeof(double), in_kind, ctx->stream));
    HIP_TRY(hipMemcpyAsync(s->alpha_prev, s->alpha, an * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    DMF_TRY(s->jobs.upload(ctx));
    HIP_TRY(dmf::launch_scatter_known_block(p->gb_known, s->gb, (int)n_c, (int)K, (int)S, ctx->stream));
    HIP_TRY(dmf::launch_sumsq_f64(s->u, N * n_u, ctx->scratch, &s->state->u_norm2, nullptr, ctx->stream));
    // (the cost before the loop, deconvolution.py:204: when a stop test needs it -- dmf_solver_step)
    HIP_TRY(dmf::launch_init_state(s->state, p->consts, s->alpha, (int)S, (int)n_c, (int)n_u, ctx->stream));
    // Host arrays belong to the caller again when this returns: wait for the copies out of them.  (Device arrays -- the
    // restart loops' staged uploads -- are read in stream order; their release is stream-ordered too: dmf_stage_free.)
    if (!(flags & DMF_PTR_DEVICE)) HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DMF_OK;
}

}  // namespace dmf_api

using namespace dmf_api;

extern "C" {

int dmf_solver_create(dmf_context* ctx, const dmf_problem* p, const double* u0, const double* alpha0,
                      int64_t n_u, int mode, int flags, dmf_solver** out) {
    DMF_TRY(check_ctx(ctx));
    if (out == nullptr) return DMF_ERR_BAD_ARG;
    *out = nullptr;
    if (p == nullptr || u0 == nullptr || alpha0 == nullptr || n_u < 1) return DMF_ERR_BAD_ARG;
    if (mode != DMF_MODE_PARTIAL && mode != DMF_MODE_UNSUPERVISED) return DMF_ERR_BAD_ARG;
    if (p->n_c + n_u > dmf::kMaxK) return DMF_ERR_UNSUPPORTED;
    SolverPtr s(new (std::nothrow) dmf_solver());
    if (s == nullptr) return DMF_ERR_BAD_ARG;
    s->ctx = ctx;
    s->p = p;
    s->n_u = n_u;
    s->mode = mode;
    DMF_TRY(solver_setup(s.get(), u0, alpha0, flags));
    *out = s.release();
    return DMF_OK;
}

int dmf_solver_step(dmf_solver* s, int64_t n_outer, int64_t n_iter2, double tol,
                    int64_t* iters_done_total, int* converged) {
    if (s == nullptr || n_outer < 0 || n_iter2 < 0 || n_iter2 > (1 << 20)) return DMF_ERR_BAD_ARG;
    dmf_context* ctx = s->ctx;
    DMF_TRY(check_ctx(ctx));
    const dmf_problem* p = s->p;
    // Stops are confirmed with streaming costs where the Gram form's error bound is not far below the threshold.
    // (the row pass on X16 forms b_u from x instead of d v: |x - d v| <= x16_dev x per element, u and alpha in [0, 1])
    const double gram_err = kGramCostRelErr * (double)p->N * (double)p->S * p->h_consts[kDmax] +
                            (s->key.x16 ? p->x16_dev * p->x16_sum : 0.0);
    s->confirm_stops = tol > 0.0 && ctx->stop_confirmation != 2 && (ctx->stop_confirmation == 1 || gram_err >= tol / 20.0);
    hipLaunchKernelGGL(k_set_tol, dim3(1), dim3(1), 0, ctx->stream, s->state.get(), tol, s->confirm_stops ? kConfirmBand : 1.0);
    HIP_TRY(hipGetLastError());
    if (s->cf_pending && tol > 0.0 && n_outer > 0) {
        // deconvolution.py:204: the cost before the loop, read by the first stop test only (a threshold of zero never fires)
        FamilyScope scope(ctx, DMF_KERNEL_COST);
        HIP_TRY(enqueue_cost(ctx, p->view(), s->u, s->alpha, (int)s->n_u, ctx->scratch + 1024, &s->state->cf));
        s->cf_pending = false;
        s->cf_stream_iter = -2;  // (marks: state->cf of iteration 0 IS a streaming cost; resolved at the first fetch below)
    }
    DMF_TRY(fetch_state(s));
    if (s->cf_stream_iter == -2) {
        s->cf_stream = s->h_state->cf;
        s->cf_stream_iter = s->h_state->iters;
    }
    // The device freezes the iterate once the stop test fires (every kernel checks state->done),
    // so the host may run ahead by `check_every` enqueued iterations without overshooting.
    // The batches double (8, 16, 32, 64): a solve that runs for hundreds of iterations reads the state back a handful of
    // times, and what a late stop costs is a few dozen no-op launches.
    int64_t check_every = s->spec.u_path != 2 ? 8 : 1;
    // (a threshold of zero never fires -- |cf - cf_0| < 0 -- so a fixed-work run needs no look at the state in between)
    if (tol == 0.0 && s->spec.u_path != 2) check_every = kMomRows;
    const long long iters0 = s->h_state->iters;
    // momentum rows for the kernels that read them (the one-launch row pass and the DPP alpha kernel)
    const dmf::IterationPlan plan = dmf::plan_iteration(s->key, s->spec, (int)n_iter2, s->purity != nullptr);
    const bool use_mom = n_iter2 >= 1 && n_iter2 <= kMomSteps && plan.row == dmf::RowKind::RowpassV2 &&
                         plan.alpha == dmf::AlphaKind::PhaseRow16;
    if (!use_mom && s->h_state->mom_n >= 0) {  // (rows of an earlier call with another n_iter2 / another path: off)
        hipLaunchKernelGGL(k_set_momentum, dim3(1), dim3(1), 0, ctx->stream, s->state.get(), (const double*)nullptr, 0, 0, -1);
        HIP_TRY(hipGetLastError());
    }
    while (s->h_state->iters - iters0 < n_outer && s->h_state->done != 1) {
        const int64_t left = n_outer - (s->h_state->iters - iters0);
        const int64_t batch = left < check_every ? left : check_every;
        if (use_mom) DMF_TRY(upload_momentum_rows(s, (int)batch, (int)n_iter2));  // (from h_state's a1 / a2: just fetched)
        for (int64_t b = 0; b < batch; ++b) DMF_TRY(enqueue_outer_iteration(s, (int)n_iter2));
        DMF_TRY(fetch_state(s));
        if (s->h_state->iters > iters0) s->cf_pending = false;  // (state->cf is the loop's cost from now on)
        if (s->h_state->done == 2) {
            // Paused inside the band at iteration h_state->iters (launches enqueued behind it were no-ops): decide
            // |cf - cf_0| < tol on the streaming costs of this and the previous iterate -- the reference's own formula.
            // The previous one is known when that iteration paused too (or was the starting point); the first
            // iteration inside the band has only the Gram form to go by.
            double cs = 0.0;
            DMF_TRY(cost_to_host(ctx, p->view(), s->u, s->alpha, (int)s->n_u, &cs, true));
            bool stop;
            if (s->cf_stream_iter == s->h_state->iters - 1) {
                stop = std::fabs(cs - s->cf_stream) < tol;
                s->n_confirmed += 1;
            } else {
                stop = std::fabs(s->h_state->cf - s->h_state->cf_prev) < tol;
                s->n_unconfirmed += 1;
            }
            s->cf_stream = cs;
            s->cf_stream_iter = s->h_state->iters;
            s->h_state->done = stop ? 1 : 0;
            DMF_TRY(push_state(s));
            check_every = 1;  // (stay close: the next iterations are likely to pause again)
        } else if (s->spec.u_path != 2 && check_every < 64 && check_every > 1) {
            check_every *= 2;
        }
    }
    if (iters_done_total) *iters_done_total = s->h_state->iters;
    if (converged) *converged = s->h_state->done == 1;
    return DMF_OK;
}

int dmf_solver_set_purity(dmf_solver* s, const double* purity, int flags) {
    if (s == nullptr || purity == nullptr) return DMF_ERR_BAD_ARG;
    dmf_context* ctx = s->ctx;
    DMF_TRY(check_ctx(ctx));
    if (s->mode != DMF_MODE_PARTIAL) return DMF_ERR_BAD_ARG;
    const size_t bytes = (size_t)s->p->S * sizeof(double);
    if (s->purity == nullptr) HIP_TRY(s->purity.alloc(ctx, (size_t)s->p->S));
    const hipMemcpyKind kind = (flags & DMF_PTR_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIP_TRY(hipMemcpyAsync(s->purity, purity, bytes, kind, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DMF_OK;
}

int dmf_solver_get(dmf_solver* s, int flags, double* out_u, double* out_alpha, double* out_cost,
                   int64_t* out_iters) {
    if (s == nullptr) return DMF_ERR_BAD_ARG;
    dmf_context* ctx = s->ctx;
    DMF_TRY(check_ctx(ctx));
    const dmf_problem* p = s->p;
    DMF_TRY(export_array(ctx, s->u, (size_t)p->N * s->n_u * sizeof(double), flags, out_u));
    DMF_TRY(export_array(ctx, s->alpha, (size_t)(p->n_c + s->n_u) * p->S * sizeof(double), flags, out_alpha));
    if (s->cf_pending && out_cost != nullptr) {  // no iteration has run: the cost of the starting point, now
        FamilyScope scope(ctx, DMF_KERNEL_COST);
        HIP_TRY(enqueue_cost(ctx, p->view(), s->u, s->alpha, (int)s->n_u, ctx->scratch + 1024, &s->state->cf));
        s->cf_pending = false;
    }
    DMF_TRY(fetch_state(s));
    if (out_cost) *out_cost = s->h_state->cf;
    if (out_iters) *out_iters = s->h_state->iters;
    return DMF_OK;
}

int dmf_solver_cost(dmf_solver* s, double* out_cost) {
    if (s == nullptr || out_cost == nullptr) return DMF_ERR_BAD_ARG;
    DMF_TRY(check_ctx(s->ctx));
    return cost_to_host(s->ctx, s->p->view(), s->u, s->alpha, (int)s->n_u, out_cost, true);
}

int dmf_solver_cost_begin(dmf_solver* s) {
    if (s == nullptr) return DMF_ERR_BAD_ARG;
    dmf_context* ctx = s->ctx;
    DMF_TRY(check_ctx(ctx));
    if (s->cost_event == nullptr) {
        if (!ctx->events.empty()) {
            s->cost_event = ctx->events.back();
            ctx->events.pop_back();
        } else {
            HIP_TRY(hipEventCreateWithFlags(&s->cost_event, hipEventDisableTiming));
        }
    }
    DMF_TRY(cost_to_host(ctx, s->p->view(), s->u, s->alpha, (int)s->n_u, cost_slot(s), false));
    HIP_TRY(hipEventRecord(s->cost_event, ctx->stream));
    s->cost_pending = true;
    return DMF_OK;
}

int dmf_solver_cost_end(dmf_solver* s, double* out_cost) {
    if (s == nullptr || out_cost == nullptr || !s->cost_pending) return DMF_ERR_BAD_ARG;
    DMF_TRY(check_ctx(s->ctx));
    HIP_TRY(hipEventSynchronize(s->cost_event));
    s->cost_pending = false;
    *out_cost = *cost_slot(s);
    return DMF_OK;
}

// cost_f_w with 0 / 1 weights: the cost kernels run on a view of the problem whose counts are the hold-out weights -- W16
// in D16's place where the shape's cost kernel streams u16 counts, else f64 weights expanded from the mask into a pooled
// temporary -- and whose meth_frequency is the unmasked one of `full`.
int dmf_solver_holdout_error(dmf_solver* s, const dmf_problem* full, double* sum_sq, int64_t* n_test) {
    if (s == nullptr || full == nullptr || sum_sq == nullptr || n_test == nullptr) return DMF_ERR_BAD_ARG;
    dmf_context* ctx = s->ctx;
    DMF_TRY(check_ctx(ctx));
    const dmf_problem* p = s->p;
    // (a masked `full` holds zeros where the error is taken)
    if (p->mask_bits == nullptr || full->mask_bits != nullptr || full->ctx != ctx) return DMF_ERR_BAD_ARG;
    if (full->N != p->N || full->S != p->S || full->n_c != p->n_c) return DMF_ERR_BAD_SHAPE;
    *n_test = p->n_test;
    *sum_sq = 0.0;
    if (p->n_test == 0) return DMF_OK;
    dmf::ProblemView pv;
    pv.N = p->N, pv.S = (int)p->S, pv.n_c = (int)p->n_c;
    pv.V = full->V, pv.Rt = p->Rt, pv.Rtp = p->Rtp;
    pv.D16 = p->W16, pv.SD = p->SD;
    DevBuf<double> weights;  // (the f64 weights, where the cost kernel reads them: lives until the wait below)
    if (!cost_reads_u16_only(ctx, pv, (int)s->n_u)) {
        HIP_TRY(weights.alloc(ctx, (size_t)p->N * p->S));
        HIP_TRY(dmf::launch_holdout_weights_f64(p->mask_bits, weights, p->N, (int)p->S, ctx->stream));
        pv.D = weights, pv.D16 = nullptr, pv.SD = 0;
    }
    return cost_to_host(ctx, pv, s->u, s->alpha, (int)s->n_u, sum_sq, true);
}

// dmf_solver_gram once its arguments are checked: the work on the stream.  Whatever it returns, the caller waits for the
// stream before the temporaries of this frame have gone back to the pool for long and clears in_flight.
static int solver_gram_enqueue(dmf_solver* s, int kind, double* out_gb, dmf::GramRan* ran) {
    dmf_context* ctx = s->ctx;
    const dmf_problem* p = s->p;
    const int64_t N = p->N, S = p->S, n_c = p->n_c, n_u = s->n_u, K = n_c + n_u;
    const size_t gbn = (size_t)(K + 1) * (K + 2) / 2 * S;
    DevBuf<double> slab_bu;  // (the temporaries of the integer kind live until the wait at the bottom)
    DevBuf<long long> slab_i8, acc;
    if (kind == DMF_GRAM_LAST) {
        *ran = s->last_gram;  // nothing is computed: gb as the last outer iteration left it
    } else if (kind == DMF_GRAM_FP64) {
        DMF_TRY(enqueue_gram(s, fp64_gram_kind(s), false, ran));
    } else {
        // whatever select_path chose for the solver: temporaries of the sizes problem_finalize / solver_setup allocate
        GramI8Buffers b;
        b.slab_i8_words = dmf::gram_i8_slab_words(N, p->SD, (int)n_c, (int)n_u);
        const size_t acc_words = (size_t)dmf::gram_i8_acc_words((int)S, (int)n_c, (int)n_u);
        HIP_TRY(slab_bu.alloc(ctx, (size_t)dmf::bu_cols_grid(N) * n_u * S));
        HIP_TRY(slab_i8.alloc(ctx, (size_t)b.slab_i8_words));
        HIP_TRY(acc.alloc(ctx, acc_words));
        HIP_TRY(hipMemsetAsync(acc, 0, acc_words * sizeof(long long), ctx->stream));
        b.slab_bu = slab_bu, b.slab_i8 = slab_i8, b.acc = acc, b.gb = s->gb;
        FamilyScope scope(ctx, DMF_KERNEL_GRAM);
        DMF_TRY(gram_bu_cols_i8(s, b, ran));
    }
    HIP_TRY(hipMemcpyAsync(out_gb, s->gb, gbn * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DMF_OK;
}

int dmf_solver_gram(dmf_solver* s, int kind, double* out_gb, char* out_text, int64_t cap) {
    if (s == nullptr || out_gb == nullptr || (kind != DMF_GRAM_INTEGER && kind != DMF_GRAM_FP64 && kind != DMF_GRAM_LAST))
        return DMF_ERR_BAD_ARG;
    if (out_text != nullptr && cap < 1) return DMF_ERR_BAD_ARG;
    dmf_context* ctx = s->ctx;
    DMF_TRY(check_ctx(ctx));
    const dmf_problem* p = s->p;
    if (kind == DMF_GRAM_INTEGER &&
        (p->ND < 1 || p->D16 == nullptr || p->Dt8 == nullptr || (p->n_c > 0 && p->Rtp == nullptr) ||
         (reinterpret_cast<uintptr_t>(p->Rtp.get()) & 15) != 0 ||
         !dmf::gram_i8_supported((int)p->n_c, (int)s->n_u, p->ND, p->N, p->SD)))
        return DMF_ERR_UNSUPPORTED;
    dmf::GramRan ran;
    s->in_flight = true;
    const int status = solver_gram_enqueue(s, kind, out_gb, &ran);
    // on an error path too: nothing of this call stays on the stream behind its temporaries, and the flag is cleared
    if (status != DMF_OK) (void)hipStreamSynchronize(ctx->stream);
    s->in_flight = false;
    if (status == DMF_OK && out_text != nullptr) snprintf(out_text, (size_t)cap, "%s", ran.text);
    return status;
}

// The row kind whose producer dmf_solver_row_moments runs: the stand-alone u phase of this solver in its split form -- what
// it takes beyond kSplitInnerSteps inner steps (wide row groups take it at every count).
static dmf::RowKind row_moments_kind(const dmf_solver* s) { return standalone_row_kind(s, kSplitInnerSteps + 1); }

// dmf_solver_row_moments once its arguments are checked: the producer and the copy on the stream, and the wait for both
static int solver_row_moments_enqueue(dmf_solver* s, dmf::RowKind row, double* out_cm, dmf::CmRan* ran) {
    dmf_context* ctx = s->ctx;
    const dmf::ProblemView pv = s->p->view();
    const int n_iter2 = kSplitInnerSteps + 1;
    DMF_TRY(ensure_split_scratch(s, 1));
    {
        FamilyScope scope(ctx, DMF_KERNEL_ROWPASS);
        if (row == dmf::RowKind::UPhaseMfmaSplit) {
            HIP_TRY(dmf::launch_u_phase_mfma_impl(pv, s->iterate(), n_iter2, s->cm, ctx->stream));
            dmf::describe_row_launch(dmf::u_phase_mfma_plan(pv.N, pv.S, pv.n_c, (int)s->n_u, n_iter2, pv.D16 != nullptr, pv.SD, true),
                                     ran->text, sizeof(ran->text));
        } else {
            HIP_TRY(dmf::launch_cm_i8(pv, s->iterate(), s->cm, ctx->stream, ran));
        }
    }
    const size_t n = (size_t)dmf::u_phase_split_cm_doubles(pv.N, (int)s->n_u);
    HIP_TRY(hipMemcpyAsync(out_cm, s->cm, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DMF_OK;
}

int dmf_solver_row_moments(dmf_solver* s, double* out_cm, char* out_text, int64_t cap) {
    if (s == nullptr || out_cm == nullptr || (out_text != nullptr && cap < 1)) return DMF_ERR_BAD_ARG;
    dmf_context* ctx = s->ctx;
    DMF_TRY(check_ctx(ctx));
    const dmf::RowKind row = row_moments_kind(s);
    if (row != dmf::RowKind::CmI8InnerRows && row != dmf::RowKind::CmI8InnerBu && row != dmf::RowKind::UPhaseMfmaSplit)
        return DMF_ERR_UNSUPPORTED;  // (a u phase that keeps c_i / M_i in its registers or never forms them)
    // the producers return at once when the stop test has fired: what is in the scratch then is an earlier iteration's
    DMF_TRY(fetch_state(s));
    if (s->h_state->done != 0) return DMF_ERR_BAD_ARG;
    dmf::CmRan ran;
    s->in_flight = true;
    const int status = solver_row_moments_enqueue(s, row, out_cm, &ran);
    if (status != DMF_OK) (void)hipStreamSynchronize(ctx->stream);
    s->in_flight = false;
    if (status == DMF_OK && out_text != nullptr) snprintf(out_text, (size_t)cap, "%s", ran.text);
    return status;
}

int dmf_solver_momentum_state(const dmf_solver* s, double* scalars, double* alpha_prev, double* u_prev) {
    if (s == nullptr || scalars == nullptr) return DMF_ERR_BAD_ARG;
    dmf_context* ctx = s->ctx;
    DMF_TRY(check_ctx(ctx));
    const dmf_problem* p = s->p;
    SolverState st;  // (a copy of its own: the solver's page-locked mirror is the stepping loop's)
    HIP_TRY(hipMemcpyAsync(&st, s->state.get(), sizeof(SolverState), hipMemcpyDeviceToHost, ctx->stream));
    if (alpha_prev != nullptr)
        HIP_TRY(hipMemcpyAsync(alpha_prev, s->alpha_prev.get(), (size_t)(p->n_c + s->n_u) * p->S * sizeof(double), hipMemcpyDeviceToHost,
                               ctx->stream));
    if (u_prev != nullptr)
        HIP_TRY(hipMemcpyAsync(u_prev, s->u_prev.get(), (size_t)p->N * s->n_u * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const double out[DMF_MOMENTUM_SCALARS] = {st.a1, st.a2, st.l_w, st.l_w_prev, st.l_h, st.l_h_prev, st.dsq, st.rt_norm2,
                                              st.u_norm2, st.cf, st.cf_prev, (double)st.iters, (double)st.done,
                                              (double)st.arrive, (double)st.mom_n, (double)st.mom_i};
    for (int i = 0; i < DMF_MOMENTUM_SCALARS; ++i) scalars[i] = out[i];
    return DMF_OK;
}

int dmf_solver_destroy(dmf_solver* s) {
    if (s == nullptr) return DMF_OK;
    dmf_context* ctx = s->ctx;
    hipSetDevice(ctx->device);
    // The solver's buffers go back to the context's pool / free lists (with the members that own them), whose reuse is
    // ordered on the context's stream, and its page-locked blocks to the next solver: what must not be in flight is a
    // transfer INTO or OUT OF those blocks.
    if (s->cost_pending) (void)hipEventSynchronize(s->cost_event);
    if (s->in_flight) (void)hipStreamSynchronize(ctx->stream);
    if (s->cost_event) ctx->events.push_back(s->cost_event);
    if (s->mom_host) ctx->pinned_moms.push_back(s->mom_host);
    if (s->h_state) ctx->pinned_states.push_back(s->h_state);
    delete s;
    return DMF_OK;
}

int dmf_solver_describe(const dmf_solver* s, int64_t n_iter2, char* buf, int64_t cap) {
    if (s == nullptr || buf == nullptr || cap < 1 || n_iter2 < 0) return DMF_ERR_BAD_ARG;
    const dmf::IterationPlan plan = dmf::plan_iteration(s->key, s->spec, (int)n_iter2, s->purity != nullptr);
    dmf::describe_plan(s->key, plan, (int)n_iter2, buf, (size_t)cap);
    return DMF_OK;
}

int dmf_solver_u_phase_describe(const dmf_solver* s, int64_t n_iter2, int route, char* buf, int64_t cap) {
    if (s == nullptr || buf == nullptr || cap < 1 || n_iter2 < 0 || n_iter2 > (1 << 20) ||
        (route != DMF_ROUTE_SOLVER && route != DMF_ROUTE_UPDATE_U))
        return DMF_ERR_BAD_ARG;
    dmf::describe_u_phase(s->key, s->spec, (int)n_iter2, s->purity != nullptr, route == DMF_ROUTE_UPDATE_U, buf, (size_t)cap);
    return DMF_OK;
}

int dmf_solver_stop_info(const dmf_solver* s, int* confirm_stops, int64_t* n_confirmed, int64_t* n_unconfirmed,
                         double* last_stream_cost) {
    if (s == nullptr) return DMF_ERR_BAD_ARG;
    if (confirm_stops) *confirm_stops = s->confirm_stops ? 1 : 0;
    if (n_confirmed) *n_confirmed = s->n_confirmed;
    if (n_unconfirmed) *n_unconfirmed = s->n_unconfirmed;
    if (last_stream_cost) *last_stream_cost = s->cf_stream_iter >= 0 ? s->cf_stream : std::nan("");
    return DMF_OK;
}

int dmf_solver_rowpass_launches(const dmf_solver* s, int64_t* total, int64_t* paired) {
    return dmf_solver_rowpass_schedule_counts(s, total, paired, nullptr);
}

int dmf_solver_rowpass_schedule_counts(const dmf_solver* s, int64_t* total, int64_t* paired, int64_t* deferred) {
    if (s == nullptr) return DMF_ERR_BAD_ARG;
    if (total) *total = s->n_rowpass[(int)dmf::RowpassSchedule::One];
    if (paired) *paired = s->n_rowpass[(int)dmf::RowpassSchedule::Pair];
    if (deferred) *deferred = s->n_rowpass[(int)dmf::RowpassSchedule::Deferred];
    return DMF_OK;
}

int dmf_solver_rowpass_byte_launches(const dmf_solver* s, int64_t* bytes) {
    if (s == nullptr || bytes == nullptr) return DMF_ERR_BAD_ARG;
    *bytes = s->n_rowpass[(int)dmf::RowpassSchedule::Bytes];
    return DMF_OK;
}

int dmf_solve(dmf_context* ctx, const dmf_problem* p, const double* u0, const double* alpha0, int64_t n_u,
              int mode, int64_t n_iter1, int64_t n_iter2, double tol, int flags, double* out_u,
              double* out_alpha, double* out_cost, int64_t* out_iters) {
    dmf_solver* raw = nullptr;
    DMF_TRY(dmf_solver_create(ctx, p, u0, alpha0, n_u, mode, flags, &raw));
    SolverPtr s(raw);
    DMF_TRY(dmf_solver_step(raw, n_iter1, n_iter2, tol, nullptr, nullptr));
    return dmf_solver_get(raw, flags, out_u, out_alpha, out_cost, out_iters);
}

}  // extern "C"
