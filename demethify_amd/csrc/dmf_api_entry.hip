// C-ABI of libdemethify_hip.so, part 4: the single-function entry points -- one piece of the algorithm on the caller's
// arrays, for tests and for callers that drive the loop themselves.
#include "dmf_api.h"

using namespace dmf_api;

static double advance_momentum(double a, int64_t n) {
    for (int64_t t = 0; t < n; ++t) a = (1.0 + std::sqrt(1.0 + 4.0 * a * a)) / 2.0;
    return a;
}

// numpy's "linear" percentile (numpy/lib/_function_base_impl.py: _quantile, _get_indexes, _get_gamma):
// virtual index (n - 1) * (q / 100), its floor and the next index, gamma = the fractional part
static dmf::PercentilePlan percentile_plan(int64_t n, double q_percent) {
#pragma clang fp contract(off)  // numpy rounds the product before subtracting the floor
    dmf::PercentilePlan pl{};
    const double quantile = q_percent / 100.0;
    const double vi = (double)(n - 1) * quantile;
    if (vi >= (double)(n - 1)) {
        pl.k_prev = pl.k_next = n - 1;
        pl.gamma = 0.0;
    } else if (vi < 0.0) {
        pl.k_prev = pl.k_next = 0;
        pl.gamma = 0.0;
    } else {
        const double fl = std::floor(vi);
        pl.k_prev = (long long)fl;
        pl.k_next = pl.k_prev + 1;
        pl.gamma = vi - fl;
    }
    return pl;
}

// where a single-function entry point writes its result: the caller's device array, or a pooled one copied out afterwards
static int result_array(dmf_context* ctx, double* out, size_t count, int flags, DevBuf<double>& dst) {
    if (flags & DMF_PTR_DEVICE) dst.borrow(out);
    else HIP_TRY(dst.alloc(ctx, count));
    return DMF_OK;
}
static int deliver_result(dmf_context* ctx, const double* dev, size_t count, int flags, double* out) {
    if (!(flags & DMF_PTR_DEVICE)) HIP_TRY(hipMemcpyAsync(out, dev, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DMF_OK;
}

extern "C" {

// the key of dmf_select_describe / dmf_u_phase_describe: what dmf_solver_create makes of such a problem
static int select_key(int64_t N, int64_t S, int64_t n_c, int64_t n_u, int nd, int level, int64_t n_iter2, int flags,
                      const char* buf, int64_t cap, dmf::ShapeKey& key) {
    if (buf == nullptr || cap < 1 || N < 1 || S < 1 || n_c < 0 || n_u < 1 || nd < 0 || nd > 2 || n_iter2 < 0 ||
        n_c + n_u > dmf::kMaxK)
        return DMF_ERR_BAD_ARG;
    key.N = N;
    key.S = (int)S;
    key.n_c = (int)n_c;
    key.n_u = (int)n_u;
    // (dmf_problem_create builds no integer copies for one sample, beyond 2048 samples or beyond 48 known types)
    key.nd = (S >= 2 && S <= 2048 && n_c <= 48) ? nd : 0;
    key.SD = key.nd > 0 ? (int)((S + 63) / 64 * 64) : 0;
    key.level = level;
    key.d_f32_exact = (flags & DMF_SELECT_COUNTS_F32_EXACT) != 0;
    key.rtp_present = true;
    key.v_align = (flags & DMF_SELECT_V_UNALIGNED) ? 8 : 0;
    key.x16 = key.nd > 0 && (flags & DMF_SELECT_X16) != 0;
    key.x_byte = key.x16 && (flags & DMF_SELECT_COUNTS_BYTE) != 0;
    key.rowpass_pair = !(flags & DMF_SELECT_NO_ROWPASS_PAIR);
    key.rowpass_defer_c = !(flags & DMF_SELECT_NO_ROWPASS_DEFER_C);
    key.rowpass_bytes = !(flags & DMF_SELECT_NO_ROWPASS_BYTES);
    key.rtp_align = 0;
    key.alpha_unit = !(flags & DMF_SELECT_ALPHA_OUTSIDE_UNIT);
    return DMF_OK;
}

int dmf_u_phase_describe(int64_t N, int64_t S, int64_t n_c, int64_t n_u, int nd, int level, int64_t n_iter2, int flags, int route,
                         char* buf, int64_t cap) {
    dmf::ShapeKey key;
    if (n_iter2 > (1 << 20) || S > (1 << 24) || (route != DMF_ROUTE_SOLVER && route != DMF_ROUTE_UPDATE_U)) return DMF_ERR_BAD_ARG;
    DMF_TRY(select_key(N, S, n_c, n_u, nd, level, n_iter2, flags, buf, cap, key));
    const dmf::PathSpec spec = dmf::select_path(key);
    if (!spec.supported) return DMF_ERR_UNSUPPORTED;
    dmf::describe_u_phase(key, spec, (int)n_iter2, (flags & DMF_SELECT_PURITY) != 0, route == DMF_ROUTE_UPDATE_U, buf, (size_t)cap);
    return DMF_OK;
}

int dmf_select_describe(int64_t N, int64_t S, int64_t n_c, int64_t n_u, int nd, int level, int64_t n_iter2, int flags,
                        char* buf, int64_t cap) {
    dmf::ShapeKey key;
    DMF_TRY(select_key(N, S, n_c, n_u, nd, level, n_iter2, flags, buf, cap, key));
    const dmf::PathSpec spec = dmf::select_path(key);
    if (!spec.supported) return DMF_ERR_UNSUPPORTED;
    const dmf::IterationPlan plan = dmf::plan_iteration(key, spec, (int)n_iter2, (flags & DMF_SELECT_PURITY) != 0);
    dmf::describe_plan(key, plan, (int)n_iter2, buf, (size_t)cap);
    return DMF_OK;
}

int dmf_cost_describe(int64_t S, int64_t n_c, int64_t n_u, int has_u16, int64_t SD, int v_align, int rtp_present, int level,
                      char* buf, int64_t cap) {
    if (buf == nullptr || cap < 1 || S < 1 || S > (1 << 24) || n_c < 0 || n_u < 0 || n_c + n_u < 1 || n_c + n_u > dmf::kMaxK ||
        SD < 0 || SD > (1 << 24) || (has_u16 && SD < S) || v_align < 0 || v_align > 15 || level < 0 || level > 4)
        return DMF_ERR_BAD_ARG;
    dmf::CostKey key;
    key.S = (int)S;
    key.n_c = (int)n_c;
    key.n_u = (int)n_u;
    key.d16 = has_u16 != 0;
    key.SD = (int)SD;
    key.v_align = (unsigned)v_align;
    key.rtp_present = rtp_present != 0;
    key.level = level;
    dmf::describe_cost_plan(dmf::cost_plan(key), buf, (size_t)cap);
    return DMF_OK;
}

int dmf_gram_i8_describe(int64_t N, int64_t S, int64_t n_c, int64_t n_u, int nd, char* buf, int64_t cap) {
    if (buf == nullptr || cap < 1 || N < 1 || S < 1 || S > (1 << 24) || n_c < 0 || n_u < 0 || n_c + n_u < 1 ||
        n_c + n_u > dmf::kMaxK)
        return DMF_ERR_BAD_ARG;
    const dmf::GramI8Plan g = dmf::gram_i8_plan(N, (int)((S + 63) / 64 * 64), (int)n_c, (int)n_u, nd);
    if (!g.supported) return DMF_ERR_UNSUPPORTED;
    dmf::describe_gram_i8_plan(g, buf, (size_t)cap);
    return DMF_OK;
}

int dmf_cost(dmf_context* ctx, const dmf_problem* p, const double* u, int64_t n_u, const double* alpha,
             int flags, double* out_cost) {
    DMF_TRY(check_ctx(ctx));
    if (p == nullptr || alpha == nullptr || out_cost == nullptr || n_u < 0) return DMF_ERR_BAD_ARG;
    if (n_u > 0 && u == nullptr) return DMF_ERR_BAD_ARG;
    const int64_t K = p->n_c + n_u;
    if (K < 1) return DMF_ERR_BAD_ARG;
    DevBuf<double> du, da, dout;
    DMF_TRY(import_array(ctx, u, (size_t)p->N * n_u, flags, du));
    DMF_TRY(import_array(ctx, alpha, (size_t)K * p->S, flags, da));
    HIP_TRY(dout.alloc(ctx, 1));
    {
        FamilyScope scope(ctx, DMF_KERNEL_COST);
        HIP_TRY(enqueue_cost(ctx, p->view(), du, da, (int)n_u, ctx->scratch + 1024, dout));
    }
    HIP_TRY(hipMemcpyAsync(out_cost, dout, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DMF_OK;
}

int dmf_project_simplex(dmf_context* ctx, const double* X, int64_t K, int64_t S, double z, int flags,
                        double* out) {
    DMF_TRY(check_ctx(ctx));
    if (X == nullptr || out == nullptr || K < 1 || S < 1) return DMF_ERR_BAD_ARG;
    if (K > dmf::kMaxK) return DMF_ERR_UNSUPPORTED;
    const size_t count = (size_t)K * S;
    DevBuf<double> dx, dout;
    DMF_TRY(import_array(ctx, X, count, flags, dx));
    DMF_TRY(result_array(ctx, out, count, flags, dout));
    HIP_TRY(dmf::launch_project_simplex(dx, dout, (int)K, (int)S, z, ctx->stream));
    return deliver_result(ctx, dout, count, flags, out);
}

// np.percentile (skip_nan false) or np.nanpercentile over axis 0, two percentiles per launch
static int percentile_axis0(dmf_context* ctx, const double* x, int64_t n, int64_t m, const double* q, int64_t n_q, int flags,
                            double* out, bool skip_nan) {
    DMF_TRY(check_ctx(ctx));
    if (x == nullptr || q == nullptr || out == nullptr || n < 1 || m < 1 || n_q < 1) return DMF_ERR_BAD_ARG;
    for (int64_t i = 0; i < n_q; ++i)
        if (!(q[i] >= 0.0 && q[i] <= 100.0)) return DMF_ERR_BAD_ARG;  // numpy: "Percentiles must be in the range [0, 100]"
    if (n > dmf::percentile_max_replicates()) return DMF_ERR_UNSUPPORTED;
    DevBuf<double> dx, dout;
    DMF_TRY(import_array(ctx, x, (size_t)n * m, flags, dx));
    DMF_TRY(result_array(ctx, out, (size_t)n_q * m, flags, dout));
    for (int64_t i = 0; i < n_q; i += 2) {
        const dmf::PercentilePlan p0 = percentile_plan(n, q[i]);
        const bool two = i + 1 < n_q;
        const dmf::PercentilePlan p1 = two ? percentile_plan(n, q[i + 1]) : p0;
        double* out0 = dout + i * m;
        double* out1 = two ? dout + (i + 1) * m : nullptr;
        // (the kernels plan each column from the quantile, q / 100 as percentile_plan divides it, and its own count)
        if (skip_nan)
            HIP_TRY(dmf::launch_nanpercentile_pair(dx, n, m, p0, p1, q[i] / 100.0, q[two ? i + 1 : i] / 100.0, out0, out1,
                                                   ctx->stream));
        else HIP_TRY(dmf::launch_percentile_pair(dx, n, m, p0, p1, out0, out1, ctx->stream));
    }
    return deliver_result(ctx, dout, (size_t)n_q * m, flags, out);
}

int dmf_percentile_axis0(dmf_context* ctx, const double* x, int64_t n, int64_t m, const double* q, int64_t n_q,
                         int flags, double* out) {
    return percentile_axis0(ctx, x, n, m, q, n_q, flags, out, false);
}

int dmf_nanpercentile_axis0(dmf_context* ctx, const double* x, int64_t n, int64_t m, const double* q, int64_t n_q,
                            int flags, double* out) {
    return percentile_axis0(ctx, x, n, m, q, n_q, flags, out, true);
}

int dmf_update_u(dmf_context* ctx, const dmf_problem* p, const double* u, const double* u_prev,
                 const double* alpha, int64_t n_u, int64_t n_iter2, int mode, int flags,
                 double* scalars_io, double* out_u, double* out_u_prev) {
    if (u_prev == nullptr || scalars_io == nullptr || out_u == nullptr || out_u_prev == nullptr || n_iter2 < 0)
        return DMF_ERR_BAD_ARG;
    dmf_solver* raw = nullptr;
    DMF_TRY(dmf_solver_create(ctx, p, u, alpha, n_u, mode, flags, &raw));
    SolverPtr s(raw);
    const size_t un = (size_t)p->N * n_u * sizeof(double);
    const hipMemcpyKind in_kind = (flags & DMF_PTR_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIP_TRY(hipMemcpyAsync(s->u_prev, u_prev, un, in_kind, ctx->stream));
    DMF_TRY(fetch_state(raw));
    s->h_state->a1 = scalars_io[0];
    s->h_state->l_w_prev = scalars_io[1];
    s->h_state->l_w = scalars_io[2];
    DMF_TRY(push_state(raw));
    DMF_TRY(enqueue_u_phase(raw, (int)n_iter2, standalone_row_kind(raw, (int)n_iter2)));
    DMF_TRY(export_array(ctx, s->u, un, flags, out_u));
    DMF_TRY(export_array(ctx, s->u_prev, un, flags, out_u_prev));
    scalars_io[0] = advance_momentum(scalars_io[0], n_iter2);
    if (n_iter2 > 0) scalars_io[1] = scalars_io[2];
    return DMF_OK;
}

int dmf_update_alpha(dmf_context* ctx, const dmf_problem* p, const double* u, int64_t n_u,
                     const double* alpha, const double* alpha_prev, int64_t n_iter2, int flags,
                     double* scalars_io, double* out_alpha, double* out_alpha_prev) {
    if (alpha_prev == nullptr || scalars_io == nullptr || out_alpha == nullptr || out_alpha_prev == nullptr ||
        n_iter2 < 0)
        return DMF_ERR_BAD_ARG;
    dmf_solver* raw = nullptr;
    DMF_TRY(dmf_solver_create(ctx, p, u, alpha, n_u, DMF_MODE_PARTIAL, flags, &raw));
    SolverPtr s(raw);
    const size_t an = (size_t)(p->n_c + n_u) * p->S * sizeof(double);
    const hipMemcpyKind in_kind = (flags & DMF_PTR_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIP_TRY(hipMemcpyAsync(s->alpha_prev, alpha_prev, an, in_kind, ctx->stream));
    DMF_TRY(fetch_state(raw));
    s->h_state->a2 = scalars_io[0];
    s->h_state->l_h_prev = scalars_io[1];
    s->h_state->l_h = scalars_io[2];
    DMF_TRY(push_state(raw));
    DMF_TRY(enqueue_gram(raw, fp64_gram_kind(raw)));  // (the caller's u: FP64 kernels)
    const dmf::AlphaKind kind = dmf::plan_iteration(raw->key, raw->spec, (int)n_iter2, raw->purity != nullptr).alpha;
    DMF_TRY(enqueue_alpha_phase(raw, kind, (int)n_iter2));
    DMF_TRY(export_array(ctx, s->alpha, an, flags, out_alpha));
    DMF_TRY(export_array(ctx, s->alpha_prev, an, flags, out_alpha_prev));
    scalars_io[0] = advance_momentum(scalars_io[0], n_iter2);
    if (n_iter2 > 0) scalars_io[1] = scalars_io[2];
    return DMF_OK;
}

}  // extern "C"
