// Private to the C-ABI layer (dmf_api_*.hip): the three handle structs, the owner of pool memory, the error macros and
// what the translation units of the layer share.  See include/demethify_hip.h for the contract.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/demethify_hip.h"
#include "dmf_internal.h"
#include "dmf_rowpass_image.h"
#include "dmf_select.h"

using dmf::SolverState;

namespace dmf_api {

int hip_fail(hipError_t e, const char* what, const char* file, int line);  // sets dmf_last_error's text

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return dmf_api::hip_fail(e_, #expr, __FILE_NAME__, __LINE__);    \
    } while (0)

#define DMF_TRY(expr)                 \
    do {                              \
        int s_ = (expr);              \
        if (s_ != DMF_OK) return s_;  \
    } while (0)

constexpr int kEventPool = 2048;

struct FamilyClock {
    std::vector<hipEvent_t> start, stop;
    int used = 0;
    double total_ms = 0.0;
    int64_t launches = 0;
};

}  // namespace dmf_api

struct dmf_context {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    unsigned profiling = 0;  // bit f: record events around the launches of kernel family f
    int stop_confirmation = 0;  // dmf_context_set_stop_confirmation: 0 by error bound, 1 always, 2 never
    int generic_level = 0;  // 0 fused row pass, 1 any-shape Gram-form kernels, 2 schedule-faithful u steps,
                            // 3 separate MFMA row pass + one-pass Gram (the pieces the fused kernel is made of)
    bool x16 = true;        // dmf_context_set_x16: problems created from now on get the X16 copy when their data allow
    bool rowpass_pair = true;  // dmf_context_set_rowpass_pair: solvers created from now on run the row pass two blocks per phase B
    bool rowpass_defer_c = true;  // dmf_context_set_rowpass_defer_c: ... with phase C deferred where that applies
    bool rowpass_bytes = true;    // dmf_context_set_rowpass_bytes: ... reading the problem's byte images where it has them
    double* scratch = nullptr;  // 4096 doubles of reduction scratch
    hipMemPool_t pool = nullptr;  // the context's own stream-ordered pool (the device's default pool is not touched)
    std::unordered_map<void*, size_t> live;                // large blocks handed out by pool_alloc (size by address)
    std::unordered_map<size_t, std::vector<void*>> kept;    // freed large blocks kept for the next allocation of that size
    size_t kept_bytes = 0;
    std::vector<hipEvent_t> events;       // ... and of their cost events
    std::vector<double*> pinned_moms;    // ... and of their momentum-row staging buffers
    std::vector<void*> pinned_states;   // page-locked SolverState mirrors of destroyed solvers, reused by the next ones
                                        // (hipHostMalloc / hipHostFree cost ~0.1 ms each: a restart loop makes one per restart)
    hipStream_t copy_stream = nullptr;  // dmf_stage_upload: uploads beside the kernels of `stream` (created on first use)
    std::mutex copy_mutex;
    // dmf_mask_draw, under copy_mutex: the jump rounds of the last segmented draw's plan (segments of mask_jump_c blocks,
    // mask_jump_w of them) on the device -- the job table, then from byte mask_jump_terms_at on the polynomials' term lists --
    // and per launch { first job, number of jobs }: a sweep draws one shape
    char* mask_jump_table = nullptr;
    size_t mask_jump_terms_at = 0;
    int64_t mask_jump_c = 0, mask_jump_w = 0;
    std::vector<std::pair<size_t, size_t>> mask_jump_rounds;
    dmf_api::FamilyClock clocks[DMF_KERNEL_FAMILIES];
};

namespace dmf_api {

// The context's pool (dmf_api_context.hip).  pool_free is for the pool code, DevBuf and dmf_stage_free alone.
hipError_t pool_alloc(dmf_context* ctx, void** p, size_t bytes);
void pool_free(dmf_context* ctx, void* p);
// A block for the staging calls, which run on worker threads: from the pool on the given stream, past the kept lists (they
// belong to the thread that drives `stream`), and its release before anybody else has seen the block.
hipError_t stage_alloc(dmf_context* ctx, hipStream_t st, void** p, size_t bytes);
void stage_release(dmf_context* ctx, hipStream_t st, void* p);

// Owner of one device array.  Either the array came from pool_alloc and goes back through pool_free when the owner dies
// (or is reset), or it is somebody else's (a caller's DMF_PTR_DEVICE array, another handle's buffer) and is left alone.
// A staging call's block (alloc_staged) lives on that call's stream instead, until it is released to the caller.
// Reads like the pointer it holds.
template <class T>
class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : ctx_(o.ctx_), ptr_(o.ptr_), owned_(o.owned_), stage_(o.stage_) {
        o.ptr_ = nullptr, o.owned_ = false;
    }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            ctx_ = o.ctx_, ptr_ = o.ptr_, owned_ = o.owned_, stage_ = o.stage_;
            o.ptr_ = nullptr, o.owned_ = false;
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    hipError_t alloc(dmf_context* ctx, size_t count) {  // `count` elements, uninitialised
        reset();
        const hipError_t e = pool_alloc(ctx, (void**)&ptr_, count * sizeof(T));
        if (e != hipSuccess) ptr_ = nullptr;
        ctx_ = ctx, owned_ = e == hipSuccess, stage_ = nullptr;
        return e;
    }
    hipError_t alloc_staged(dmf_context* ctx, size_t count, hipStream_t st) {  // stage_alloc on `st`, uninitialised
        reset();
        const hipError_t e = stage_alloc(ctx, st, (void**)&ptr_, count * sizeof(T));
        if (e != hipSuccess) ptr_ = nullptr;
        ctx_ = ctx, owned_ = e == hipSuccess, stage_ = st;
        return e;
    }
    T* release() {  // the array becomes the caller's (who frees it with dmf_stage_free)
        T* p = ptr_;
        ptr_ = nullptr, owned_ = false;
        return p;
    }
    void borrow(const T* p) { reset(), ptr_ = const_cast<T*>(p); }
    void reset() {
        if (owned_ && stage_ != nullptr) stage_release(ctx_, stage_, ptr_);
        else if (owned_) pool_free(ctx_, ptr_);
        ptr_ = nullptr, owned_ = false;
    }
    T* get() const { return ptr_; }
    operator T*() const { return ptr_; }
    T* operator->() const { return ptr_; }

  private:
    dmf_context* ctx_ = nullptr;
    T* ptr_ = nullptr;
    bool owned_ = false;
    hipStream_t stage_ = nullptr;  // alloc_staged: the stream the block was allocated on
};

// the problem's constants: indices into dmf_problem::h_consts and into the device array `consts` that the kernels read
enum ProblemConst { kDsq, kRtSumsq, kDmax, kF32ResidualMax, kIntCountMax, kRtOutsideUnit, kProblemConsts };

// A (k, l, tri(k, l)) job table of the packed Gram: the host arrays (the uploads read them: they live as long as the
// table, so that nobody need wait for the copies) and their device copies.
struct JobTable {
    std::vector<short> h_k, h_l;
    std::vector<int> h_dst;
    DevBuf<short> k, l;
    DevBuf<int> dst;
    int n = 0;
    // every k <= l with l in [l_first, l_last] that `keep` accepts, in the order l-major, k-minor
    template <class Keep>
    void build(int l_first, int l_last, Keep keep) {
        for (int ll = l_first; ll <= l_last; ++ll)
            for (int kk = 0; kk <= ll; ++kk) {
                if (!keep(kk, ll)) continue;
                h_k.push_back((short)kk);
                h_l.push_back((short)ll);
                h_dst.push_back(dmf::tri(kk, ll));
            }
        n = (int)h_k.size();
    }
    int upload(dmf_context* ctx) {  // (enqueued; not waited for)
        HIP_TRY(k.alloc(ctx, n));
        HIP_TRY(l.alloc(ctx, n));
        HIP_TRY(dst.alloc(ctx, n));
        HIP_TRY(hipMemcpyAsync(k, h_k.data(), n * sizeof(short), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(l, h_l.data(), n * sizeof(short), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(dst, h_dst.data(), n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        return DMF_OK;
    }
};

}  // namespace dmf_api

struct dmf_problem {
    dmf_context* ctx = nullptr;
    int64_t N = 0, S = 0, n_c = 0;
    dmf_api::DevBuf<double> V, D, Rt;  // (borrowed when the caller passed device arrays)
    dmf_api::DevBuf<double> Rtp;       // R_trunc, rows zero-padded to a multiple of 4 doubles (borrows Rt if n_c % 4 == 0)
    dmf_api::DevBuf<double> consts;    // device copy of h_consts
    double h_consts[dmf_api::kProblemConsts] = {};  // by ProblemConst: max(D)^2, ||Rt||^2, max(D), max |D - f32(D)|,
                                                    // int-count max or inf, Rt outside [0, 1]
    // integer copies of the counts for the second-generation kernels (dmf_kernels_rowpass2.hip, dmf_kernels_gram_i8.hip):
    // built when every count is an integer in [0, 32639], S <= 2048 and R_trunc lies in [0, 1]
    dmf_api::DevBuf<unsigned short> D16;  // [N16][SD], zero padded
    dmf_api::DevBuf<signed char> Dt8;     // [ND][ceil(N / 32)][SD / 32][32][32] balanced 8-bit digits, MFMA B layout
    int ND = 0;                     // count digits: 0 = no integer copies, 1 (d <= 127), 2 (d <= 32639)
    int SD = 0;
    int64_t N16 = 0, plane_stride = 0;
    // the methylated read counts x = rint(v d) as u16 in D16's layout, when every element is exact to kX16MaxDev
    // (dmf_internal.h): the row pass then reads (X16, D16) instead of (V, D16).  x16_dev: the largest |v d - x| / max(x, 1)
    // seen, x16_sum: sum of x -- their product bounds what the substitution changes in the Gram-form cost.
    dmf_api::DevBuf<unsigned short> X16;
    double x16_dev = 0.0, x16_sum = 0.0;
    // byte images of X16 / D16 ([N16 / 16][SD / 64][1024], dmf_rowpass_image.h) for the row pass's deferred-C schedule: built
    // (build_rowpass_images) where dmf::rowpass_v2_byte_images_wanted: some plan of the problem reads them
    dmf_api::DevBuf<unsigned char> X8, D8;
    bool d_f32_exact = false;    // every count survives a round trip through f32 (the fused tile stores D as f32)
    dmf_api::DevBuf<double> gb_known;  // [(n_c+1)(n_c+2)/2][S]
    dmf::GramRan known_ran;            // which route problem_finalize took for it, as text (dmf_problem_gram_known)
    // a masked problem (dmf_problem_mask) keeps what dmf_solver_holdout_error needs: the train mask as it came (bit-packed,
    // ceil(S / 8) bytes per row, 1 = kept), the number of held-out elements, and -- with integer count copies -- the
    // hold-out weights (1 where held out) as u16 in D16's padded layout, which the u16 cost kernels read in D16's place
    dmf_api::DevBuf<unsigned char> mask_bits;
    dmf_api::DevBuf<unsigned short> W16;
    int64_t n_test = 0;
    // the device arrays as the launch wrappers take them (dmf_internal.h)
    dmf::ProblemView view() const {
        dmf::ProblemView v;
        v.V = V, v.D = D, v.D16 = D16, v.X16 = X16, v.Dt8 = Dt8;
        v.X8 = X8, v.D8 = D8;
        v.plane_stride = plane_stride, v.SD = SD, v.ND = ND;
        v.Rt = Rt, v.Rtp = Rtp;
        v.N = N, v.S = (int)S, v.n_c = (int)n_c;
        return v;
    }
};

// page-locked per-solver block: the SolverState mirror, then one double for dmf_solver_cost_begin's result
constexpr size_t kPinnedStateBytes = (sizeof(SolverState) + 15) / 16 * 16 + 16;

struct dmf_solver {
    dmf_context* ctx = nullptr;
    const dmf_problem* p = nullptr;
    int64_t n_u = 0;
    int mode = 0;
    dmf::ShapeKey key;      // what the kernel selection looks at (dmf_select.h) ...
    dmf::PathSpec spec;     // ... and what it fixed for this solver
    dmf_api::DevBuf<double> cm;        // split u phase (many inner steps): per-row c_i / M_i, allocated on first use
    dmf_api::DevBuf<double> beta_tab;  //   and the momentum coefficients of the inner steps
    int64_t beta_cap = 0;
    dmf_api::DevBuf<long long> slab_i8;   // i64 partial sums of the integer Gram (one slab per row range)
    int64_t slab_i8_words = 0;
    dmf_api::DevBuf<long long> acc_i8;    // reduction scratch of the integer Gram (kept zero between iterations)
    dmf_api::DevBuf<double> purity;  // S per-sample known-block masses: set => Frank-Wolfe alpha phase
    dmf_api::DevBuf<double> u2_partials;
    dmf_api::DevBuf<double> u, u_prev, u_next;
    dmf_api::DevBuf<double> alpha, alpha_prev;
    dmf_api::DevBuf<double> gb;
    dmf::GramRan last_gram;  // what wrote the u-dependent rows of gb in the last outer iteration, as text (DMF_GRAM_LAST)
    int last_gram_source = -1;
    dmf_api::DevBuf<double> slab;
    int64_t slab_doubles = 0;
    dmf_api::DevBuf<double> partials;
    dmf_api::DevBuf<SolverState> state;
    SolverState* h_state = nullptr;  // pinned
    dmf_api::JobTable jobs;  // the per-iteration part of the packed Gram: every (k, l) that involves u
    // deconvolution.py:204 -- the cost before the loop is only ever read by the first stop test (:220): it is computed when
    // a step() call with tol > 0 (or a get() before any iteration) needs it, one 0.5 ms pass over V and D at 1e6 x 256
    bool cf_pending = true;
    // Stop test (:218-220).  The loop's cost comes from the Gram form v^T D v - 2 a.b + a^T G a, whose cancellation error
    // grows with v^T D v (measured 1e-6 .. 1e-5 absolute at 1e6 x 256, depth 120 .. 2500) -- where its bound is not far below tol
    // (confirm_stops), an iteration whose Gram-form |cf - cf_0| falls below kConfirmBand x tol pauses the device
    // (state->done = 2), and the host decides on the streaming cost of deconvolution.py:15-17 for this and the previous
    // iterate (cf_stream, cf_stream_iter), exactly the reference's formula.
    // momentum rows (SolverState::mom): a page-locked staging buffer and its device copy, kMomRows rows of 2 + 2 kMomSteps
    double* mom_host = nullptr;
    dmf_api::DevBuf<double> mom_dev;
    // dmf_solver_cost_begin / _end: the streaming cost taken WITHOUT waiting for it (the caller sets up its next solver
    // meanwhile); the event marks the result's arrival in the page-locked slot behind h_state
    hipEvent_t cost_event = nullptr;
    bool cost_pending = false;
    // Has anything been enqueued for this solver since the host last waited for the stream?  (dmf_solver_destroy then
    // waits; otherwise it must not: another solver's work may be running on the context's stream.)
    bool in_flight = false;
    bool confirm_stops = false;
    double cf_stream = 0.0;
    long long cf_stream_iter = -1;
    // k_rowpass_v2 launches so far, by dmf::RowpassSchedule: on that schedule or one built on it ([One]: all of them)
    long long n_rowpass[dmf::kRowpassSchedules] = {};
    long long n_confirmed = 0, n_unconfirmed = 0;  // stop tests decided on streaming costs / on the Gram form inside the band
    // the iterate and the u phases' scratch as the launch wrappers take them (dmf_internal.h)
    dmf::IterateView iterate() const {
        dmf::IterateView it;
        it.u = u, it.u_prev = u_prev, it.alpha = alpha, it.state = state;
        it.n_u = (int)n_u, it.mode = mode;
        return it;
    }
    dmf::AlphaView alpha_view() const {
        dmf::AlphaView a;
        a.gb = gb, a.alpha = alpha, a.alpha_prev = alpha_prev, a.purity = purity, a.state = state, a.partials = partials;
        a.S = (int)p->S, a.n_c = (int)p->n_c, a.n_u = (int)n_u;
        return a;
    }
    dmf::UScratch scratch() const {
        dmf::UScratch sc;
        sc.cm = cm, sc.beta = beta_tab, sc.slab = slab, sc.u2_partials = u2_partials;
        return sc;
    }
};

namespace dmf_api {

// handles under construction: a failed creation releases through the same destroy functions as a finished handle
struct HandleDeleter {
    void operator()(dmf_problem* p) const { dmf_problem_destroy(p); }
    void operator()(dmf_solver* s) const { dmf_solver_destroy(s); }
};
using ProblemPtr = std::unique_ptr<dmf_problem, HandleDeleter>;
using SolverPtr = std::unique_ptr<dmf_solver, HandleDeleter>;

int clock_drain(dmf_context* ctx, FamilyClock& c);

// Brackets one launch (or a fixed group of launches) of a kernel family with HIP events on
// the context's stream when profiling is enabled.
struct FamilyScope {
    dmf_context* ctx;
    FamilyClock* c = nullptr;
    int slot = -1;
    FamilyScope(dmf_context* ctx_, int family) : ctx(ctx_) {
        if (!((ctx->profiling >> family) & 1u)) return;
        c = &ctx->clocks[family];
        if (c->start.empty()) {
            c->start.resize(kEventPool);
            c->stop.resize(kEventPool);
            for (int i = 0; i < kEventPool; ++i) {
                // timing only: without the system-scope fence a default event carries (its cache write-back and invalidate
                // cost ~5 us of idle GPU per record between two kernels -- 22 us per outer iteration with two families timed)
                hipEventCreateWithFlags(&c->start[i], hipEventDisableSystemFence);
                hipEventCreateWithFlags(&c->stop[i], hipEventDisableSystemFence);
            }
        }
        if (c->used == kEventPool) clock_drain(ctx, *c);
        slot = c->used++;
        hipEventRecord(c->start[slot], ctx->stream);
    }
    ~FamilyScope() {
        if (c != nullptr) hipEventRecord(c->stop[slot], ctx->stream);
    }
};

int check_ctx(dmf_context* ctx);

// a caller's array as a device array: borrowed when it is one already (DMF_PTR_DEVICE), else uploaded and waited for
template <class T>
int import_array(dmf_context* ctx, const void* src, size_t count, int flags, DevBuf<T>& dst) {
    dst.reset();
    if (count == 0) return DMF_OK;
    if (flags & DMF_PTR_DEVICE) {
        dst.borrow(static_cast<const T*>(src));
        return DMF_OK;
    }
    HIP_TRY(dst.alloc(ctx, count));
    HIP_TRY(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DMF_OK;
}
int export_array(dmf_context* ctx, const void* dev_src, size_t bytes, int flags, void* dst);

// dmf_api_problem.hip: the streaming cost of (u, alpha) on a problem's data
hipError_t enqueue_cost(dmf_context* ctx, const dmf::ProblemView& p, const double* u, const double* alpha, int n_u,
                        double* scratch, double* out);
bool cost_reads_u16_only(dmf_context* ctx, const dmf::ProblemView& p, int n_u);
int cost_to_host(dmf_context* ctx, const dmf::ProblemView& p, const double* u, const double* alpha, int n_u,
                 double* host_slot, bool wait);

// dmf_api_solver.hip: the phases of an outer iteration, for the single-function entry points
int enqueue_u_phase(dmf_solver* s, int n_iter2, dmf::RowKind row);
dmf::RowKind standalone_row_kind(const dmf_solver* s, int n_iter2);
// heed_done false: the kernels compute on a converged solver too (dmf_solver_gram); ran: what the launcher ran, as text
int enqueue_gram(dmf_solver* s, dmf::GramKind kind, bool heed_done = true, dmf::GramRan* ran = nullptr);
dmf::GramKind fp64_gram_kind(const dmf_solver* s);
int enqueue_alpha_phase(dmf_solver* s, dmf::AlphaKind kind, int n_iter2);  // kind: plan_iteration(...).alpha
int fetch_state(dmf_solver* s);
int push_state(dmf_solver* s);

}  // namespace dmf_api
