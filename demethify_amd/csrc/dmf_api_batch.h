// Private to the C-ABI layer of the two batched solver families (dmf_api_small.hip, dmf_api_mid.hip): the steps both entry
// bodies take the same way -- the checked import of the caller's batch inputs and of the train masks of a masked call, the
// workspace both families keep per solve, the poll of the stop flags and the copy-out of the results.
#pragma once
#include <algorithm>

#include "dmf_api.h"
#include "dmf_batch.h"

namespace dmf_api {

// The caller's batch inputs as device arrays: idx (B x N, or none), u0 (un doubles), alpha0 (an doubles), purity (S, or none).
struct BatchInputs {
    DevBuf<long long> idx;
    DevBuf<double> u0, alpha0, purity;
    // idx (or none), range-checked; then the starts.  Two steps, so that a caller's own refusals can stand between them.
    int import_idx(dmf_context* ctx, const int64_t* h_idx, int64_t B, int64_t N, int flags) {
        if (h_idx != nullptr) {
            DMF_TRY(import_array(ctx, h_idx, (size_t)B * N, flags, idx));
            // every index is checked on the device before the first launch: no solve has started when one is refused
            DevBuf<unsigned int> d_bad;
            unsigned int h_bad = 1;
            HIP_TRY(d_bad.alloc(ctx, 1));
            HIP_TRY(dmf::launch_index_range_check(idx, B * N, N, d_bad, ctx->stream));
            HIP_TRY(hipMemcpyAsync(&h_bad, d_bad, sizeof(h_bad), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            if (h_bad != 0) return DMF_ERR_BAD_ARG;
        }
        return DMF_OK;
    }
    int import_starts(dmf_context* ctx, const double* h_u0, const double* h_alpha0, const double* h_purity, int64_t S, size_t un,
                      size_t an, int flags) {
        DMF_TRY(import_array(ctx, h_u0, un, flags, u0));
        DMF_TRY(import_array(ctx, h_alpha0, an, flags, alpha0));
        if (h_purity != nullptr) DMF_TRY(import_array(ctx, h_purity, (size_t)S, flags, purity));
        return DMF_OK;
    }
};

// The train masks of a masked call (B x N x ceil(S / 8) bytes) as a device array, and every solve's kept elements.
struct BatchMasks {
    DevBuf<uint8_t> bits;
    std::vector<long long> n_train;  // B: the set bits among the N x S real positions of mask b
    // The checked import: every solve's kept elements are counted on the device before the first launch, and a fold that
    // keeps none (upstream skips it, ic.py:71; here d would be 0 and l_w a division by zero) is refused while no solve has
    // started.  count(bits, n_part) enqueues the family's count launch, which writes `parts` integer partials per solve.
    template <class Count>
    int import_counted(dmf_context* ctx, const uint8_t* h_bits, int64_t B, int64_t N, int64_t S, int flags, int64_t parts,
                       const Count& count) {
        const size_t nb = (size_t)(S + 7) / 8;
        DMF_TRY(import_array(ctx, h_bits, (size_t)B * N * nb, flags, bits));
        DevBuf<long long> d_part;
        std::vector<long long> h_part((size_t)(B * parts), 0);
        HIP_TRY(d_part.alloc(ctx, h_part.size()));
        HIP_TRY(count((const uint8_t*)bits, (long long*)d_part));
        HIP_TRY(hipMemcpyAsync(h_part.data(), d_part, h_part.size() * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        n_train.assign((size_t)B, 0);
        for (int64_t b = 0; b < B; ++b) {
            for (int64_t w = 0; w < parts; ++w) n_train[(size_t)b] += h_part[(size_t)(b * parts + w)];
            if (n_train[(size_t)b] < 1) return DMF_ERR_BAD_ARG;
        }
        return DMF_OK;
    }
};

// The workspace both families keep: all per-solve state, so that the next launch continues where the last one stopped.
struct BatchWorkspace {
    DevBuf<double> u, u_prev, alpha, alpha_prev, gk, ratio, scal;
    DevBuf<long long> iters;
    DevBuf<int> done;
    int alloc(dmf_context* ctx, int64_t B, size_t un, size_t an, int64_t n_c, int64_t S, int64_t n_iter2, int flags,
              double* out_u) {
        if (flags & DMF_PTR_DEVICE) u.borrow(out_u);  // (the iterate lives in the caller's result array)
        else HIP_TRY(u.alloc(ctx, un));
        HIP_TRY(u_prev.alloc(ctx, un));
        HIP_TRY(alpha.alloc(ctx, an));
        HIP_TRY(alpha_prev.alloc(ctx, an));
        HIP_TRY(gk.alloc(ctx, (size_t)B * (size_t)std::max<int64_t>(dmf::known_jobs((int)n_c) * S, 1)));
        HIP_TRY(ratio.alloc(ctx, (size_t)B * 2 * (size_t)std::max<int64_t>(n_iter2, 1)));
        HIP_TRY(scal.alloc(ctx, (size_t)B * dmf::kBatchScalars));
        HIP_TRY(iters.alloc(ctx, (size_t)B));
        HIP_TRY(done.alloc(ctx, (size_t)B));
        return DMF_OK;
    }
    // the fields SmallArgs and MidArgs have in common: dmf::BatchArgs and what carries the same names behind it
    template <class Args>
    void fill(Args& a, const dmf_problem* p, const BatchInputs& in, int64_t n_u, int mode, int64_t n_iter2, double tol) const {
        a.V = p->V, a.D = p->D, a.Rt = p->Rt;
        a.idx = in.idx, a.u0 = in.u0, a.alpha0 = in.alpha0;
        a.N = p->N, a.S = (int)p->S, a.n_c = (int)p->n_c, a.n_u = (int)n_u, a.mode = mode;
        a.n_iter2 = n_iter2, a.tol = tol;
        a.u = u, a.u_prev = u_prev, a.alpha = alpha, a.alpha_prev = alpha_prev, a.gk = gk, a.ratio = ratio, a.scal = scal;
        a.iters = iters, a.done = done;
    }
    // have all B solves stopped?  Drains the stream once.
    int all_done(dmf_context* ctx, int64_t B, bool* all) const {
        std::vector<int> h_done((size_t)B);
        HIP_TRY(hipMemcpyAsync(h_done.data(), done, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        *all = true;
        for (int64_t b = 0; b < B && *all; ++b) *all = h_done[(size_t)b] != 0;
        return DMF_OK;
    }
    // out_iters[b] = solve b's outer iterations, the final alpha and (unless it already lives there) u: enqueued, not waited for
    int copy_out(dmf_context* ctx, int64_t B, size_t un, size_t an, int flags, double* out_u, double* out_alpha,
                 int64_t* out_iters) const {
        static_assert(sizeof(long long) == sizeof(int64_t), "out_iters is copied as long long");
        HIP_TRY(hipMemcpyAsync(out_iters, iters, (size_t)B * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(out_alpha, alpha, an * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (!(flags & DMF_PTR_DEVICE)) HIP_TRY(hipMemcpyAsync(out_u, u, un * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        return DMF_OK;
    }
};

}  // namespace dmf_api
