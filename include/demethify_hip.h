/*
 * demethify_hip.h — C-ABI of libdemethify_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for DeMethify's solver hot path.  The reference has no FFI layer: its
 * seam is the set of Python callables that demethify/demethify.py:7, demethify/bootstrap.py:6
 * and demethify/ic.py:8 import from demethify/deconvolution.py.  Each entry point below names
 * the reference callable it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - plain pointers and sizes only; every function returns a dmf_status (0 = ok) and never
 *     throws across the boundary; the caller allocates every output buffer.
 *   - matrices are dense, C-order (row-major) float64; counts are int64 or float64 (flag).
 *   - N = CpG rows, S = samples, n_c = known cell types, n_u = unknown, K = n_c + n_u.
 *     V = meth_frequency (N x S), D = d_x / counts (N x S), Rt = R_trunc (N x n_c),
 *     u (N x n_u), alpha (K x S; the LAST n_u rows are the unknown types).
 *   - pointer arguments are host pointers unless the call's `flags` carries
 *     DMF_PTR_DEVICE, in which case they are device pointers on the context's GPU
 *     (e.g. PyTorch-ROCm `tensor.data_ptr()`); device inputs are borrowed, never freed.
 *   - one context per GPU; a context is not thread-safe, independent contexts are.
 *   - inputs are never mutated (reference convention, deconvolution.py:194-195).
 */
#ifndef DEMETHIFY_HIP_H
#define DEMETHIFY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum dmf_status {
    DMF_OK = 0,
    DMF_ERR_BAD_ARG = 1,      /* null pointer, non-positive size, n_u < 1 where required ...   */
    DMF_ERR_BAD_SHAPE = 2,    /* shapes inconsistent with the problem the handle was built for  */
    DMF_ERR_HIP = 3,          /* a HIP runtime call failed; see dmf_last_error()                */
    DMF_ERR_NONFINITE = 4,    /* NaN/Inf met in an input that the solver cannot propagate        */
    DMF_ERR_UNSUPPORTED = 5,  /* size beyond what the kernels are built for (K > 64, ...)        */
    DMF_ERR_NO_DEVICE = 6     /* no gfx950 device visible                                        */
} dmf_status;

enum {
    DMF_PTR_DEVICE = 1,       /* data pointers of this call are device pointers                  */
    DMF_COUNTS_F64 = 2,       /* `counts` is float64 (default: int64, as pandas yields)          */
    DMF_INIT_IN_UNIT_RANGE = 4 /* dmf_solver_create: the caller vouches that alpha0 lies inside [0, 1] (columns on the
                                * simplex: every initialiser of deconvolution.py:40-78 and :108-137 yields that), so the
                                * library skips its own check -- a device-to-host round trip for device arrays */
};

/* dmf_select_describe flags */
enum {
    DMF_SELECT_COUNTS_F32_EXACT = 1,   /* every count survives a round trip through f32                  */
    DMF_SELECT_PURITY = 2,             /* a purity vector is set (Frank-Wolfe alpha phase)               */
    DMF_SELECT_ALPHA_OUTSIDE_UNIT = 4, /* the starting alpha does not lie inside [0, 1]                  */
    DMF_SELECT_V_UNALIGNED = 8,        /* meth_frequency starts 8 bytes off a 16-byte boundary           */
    DMF_SELECT_X16 = 16,               /* the problem carries X16: every v d is an exact count (with nd > 0) */
    /* what only the row pass's launch plan reads (dmf_u_phase_describe; dmf_select_describe's text does not change) */
    DMF_SELECT_COUNTS_BYTE = 32,           /* every count is at most 255                                 */
    DMF_SELECT_NO_ROWPASS_PAIR = 64,       /* dmf_context_set_rowpass_pair is off                        */
    DMF_SELECT_NO_ROWPASS_DEFER_C = 128,   /* dmf_context_set_rowpass_defer_c is off                     */
    DMF_SELECT_NO_ROWPASS_BYTES = 256      /* dmf_context_set_rowpass_bytes is off                       */
};

/* solver variants */
enum {
    DMF_MODE_PARTIAL = 0,     /* mdwbssmf_deconv: gradient of u taken at the extrapolated point  */
    DMF_MODE_UNSUPERVISED = 1 /* unsupervised_deconv: gradient taken at the previous iterate     */
};

/* kernel families whose device time a profiling context accumulates (dmf_context_kernel_time) */
enum {
    DMF_KERNEL_ROWPASS = 0,   /* u-phase row pass (the dominant, HBM-streaming kernel)           */
    DMF_KERNEL_GRAM = 1,      /* per-sample weighted Gram accumulation for the alpha phase        */
    DMF_KERNEL_ALPHA = 2,     /* alpha inner loop + cost + scalar bookkeeping                    */
    DMF_KERNEL_COST = 3,      /* streaming weighted cost                                         */
    DMF_KERNEL_FAMILIES = 4
};

typedef struct dmf_context dmf_context;
typedef struct dmf_problem dmf_problem;
typedef struct dmf_solver dmf_solver;

const char* dmf_status_string(int status);
/* Text of the last HIP error seen by this thread's most recent failing call ("" if none). */
const char* dmf_last_error(void);
/* Library/ABI version, bumped when a signature changes. */
int dmf_abi_version(void);

/* ---- context: one per GPU -------------------------------------------------------------- */
/* `stream` may be NULL (the context creates its own hipStream) or a hipStream_t to borrow. */
int dmf_context_create(int device, void* stream, dmf_context** out);
int dmf_context_destroy(dmf_context* ctx);
int dmf_context_synchronize(dmf_context* ctx);
/* Record HIP events around the launches of the kernel families above (costs a sync per read).
 * enabled: 0 = off, 1 = every family, else a mask with bit (1 + family) set, e.g. 2 = DMF_KERNEL_ROWPASS only. */
int dmf_context_set_profiling(dmf_context* ctx, int enabled);
int dmf_context_kernel_time(dmf_context* ctx, int family, double* total_ms, int64_t* launches);
int dmf_context_reset_kernel_time(dmf_context* ctx);
/* Kernel selection, for tests: 0 = fastest available (row pass on u16 counts + exact integer-matrix-core Gram,
 * else the first-generation fused FP64 row pass, else the unfused pair), 1 = any-shape Gram-form kernels without
 * MFMA, 2 = schedule-faithful one-launch-per-inner-step, 3 = the unfused pair (FP64-MFMA u-phase row pass + one-pass
 * Gram), 4 = the first-generation fused FP64 row pass (level 0's fall-back for counts beyond 32639 or reference
 * profiles outside [0, 1]).  Set it before creating problems: the integer count copies are built at level 0 only. */
int dmf_context_set_generic(dmf_context* ctx, int level);
/* 1 (default): problems created from now on (and their row gathers) carry X16, the methylated read counts x = rint(v d)
 * as u16, when every element with d > 0 has 0 <= x <= d and |v d - x| <= 8 ulp of max(x, 1) (meth_frequency = X / D);
 * the row pass then reads x and the counts instead of v.  0: they do not, and every kernel reads V.  Tests and A/B runs. */
int dmf_context_set_x16(dmf_context* ctx, int enabled);
/* 1 (default): solvers created from now on run the X16 form of the row pass (65..256 samples; at 65..128 samples up to
 * three unknowns, where the LDS of four workgroups per CU allows it) two 16-row blocks per barrier cycle, the two blocks' inner iterations at the same time on two waves; 0: one block at a time.  Both compute the
 * same results bit for bit.  Tests and A/B runs. */
int dmf_context_set_rowpass_pair(dmf_context* ctx, int enabled);
/* 1 (default): solvers created from now on run the pair schedule at 193..256 samples with phase C deferred -- a wave runs it
 * only in the barrier cycles in which it runs no inner iterations, beside the two waves that do -- when every count of the
 * problem is at most 255 and two workgroups with the schedule's x ring still fit a CU's LDS; 0: the pair schedule as it is.
 * Both compute the same results bit for bit.  Tests and A/B runs. */
int dmf_context_set_rowpass_defer_c(dmf_context* ctx, int enabled);
/* 1 (default): solvers created from now on run the deferred-C schedule from the problem's byte images where it has them
 * (dmf_problem_has_byte_images): x and the counts stream as one byte per element, in the order the kernel's LDS holds them,
 * instead of two; 0: from X16 / D16.  Both compute the same results bit for bit.  Tests and A/B runs. */
int dmf_context_set_rowpass_bytes(dmf_context* ctx, int enabled);
/* How dmf_solver_step decides |cf - cf_0| < tol (deconvolution.py:218-220) for the solvers of this context:
 * 0 (default) = on the Gram-form cost of the loop, with the decisions near the threshold confirmed on the streaming
 * cost of deconvolution.py:15-17 where the Gram form's error bound (1e-15 N S max(counts)) reaches tol / 20;
 * 1 = every decision near the threshold (below 10 tol) is taken on streaming costs, whatever the bound;
 * 2 = Gram form only.  See dmf_solver_stop_info. */
int dmf_context_set_stop_confirmation(dmf_context* ctx, int mode);

/* ---- problem: V, D, Rt resident in HBM + the per-problem constants ----------------------
 * Replaces the (meth_frequency, d_x, R_trunc) argument triple every reference solver call
 * takes (deconvolution.py:40,81,93,107,190).  n_c may be 0 (Rt ignored: unsupervised).
 * Uploads (or borrows) the arrays, converts int64 counts to f64 once and precomputes
 * max(D)^2 (deconvolution.py:197), ||Rt||_F^2 and the known-type blocks of the per-sample
 * Gram matrices. */
int dmf_problem_create(dmf_context* ctx, int64_t N, int64_t S, int64_t n_c,
                       const double* V, const void* counts, const double* Rt,
                       int flags, dmf_problem** out);
/* Row-gathered copy for one bootstrap resample: rows idx[0..N) of V, D, Rt
 * (bootstrap.py:28, sklearn.utils.resample applied to the three arrays).  idx: host int64. */
int dmf_problem_gather(dmf_context* ctx, const dmf_problem* src, const int64_t* idx,
                       int64_t n_idx, dmf_problem** out);
/* The same with the row indices already in HBM (e.g. uploaded by dmf_stage_upload from the thread that drew them, beside
 * the previous replicate's solve): range-checked on the device, DMF_ERR_BAD_ARG when one lies outside [0, N). */
int dmf_problem_gather_device(dmf_context* ctx, const dmf_problem* src, const int64_t* idx_dev,
                              int64_t n_idx, dmf_problem** out);
/* A copy of `src` with a set of elements held out: their counts are 0 in every copy of the counts the kernels read, which
 * is what bi-cross-validation solves per fold (ic.py:68-75, `counts * train_mask`) and what data with missing entries
 * need.  train_bits: the N x S mask, bit-packed row-major, ceil(S / 8) bytes per row, sample s = bit (s & 7) of byte
 * (s >> 3) (numpy: packbits(mask, axis=1, bitorder="little")); 1 = kept, 0 = held out; padding bits are ignored;
 * DMF_PTR_DEVICE in flags: the bits are in HBM.  The result is an ordinary problem for every solver mode, derived on the
 * device in one pass over the rows: max(counts) -- the d = D.max()**2 of deconvolution.py:197 -- is that of the kept
 * elements, the known Gram block is rebuilt; integrality and range of the counts carry over from `src` (a problem without
 * integer count copies yields one without).  It is a full copy: `src` need not outlive it.  It also keeps the mask for
 * dmf_solver_holdout_error.  src must not be a masked problem itself; dmf_problem_gather* refuse a masked source. */
int dmf_problem_mask(dmf_context* ctx, const dmf_problem* src, const uint8_t* train_bits, int flags, dmf_problem** out);
int dmf_problem_destroy(dmf_problem* p);
int dmf_problem_shape(const dmf_problem* p, int64_t* N, int64_t* S, int64_t* n_c);
/* The known block of the problem's packed Gram as dmf_problem_create left it, for tests: out ((n_c + 1)(n_c + 2) / 2 x S host
 * doubles) <- row tri(k, l) = l (l + 1) / 2 + k, k <= l <= n_c, over the extended indices (R_trunc columns, then v): the dense
 * pairs sum_i Rt_ik Rt_il d_is, the right-hand sides sum_i Rt_ik d_is v_is (l = n_c) and v^T D v (k = l = n_c).  out_text (may
 * be NULL) names the route and every launcher that wrote rows, in launch order: "int_known k_gram_i8_w8<...> ... + k_bu_cols2
 * with vDv" (the integer matrix cores, the text of dmf_gram_i8_describe with n_u = 0, then the stream kernel of the right-hand
 * sides; "+ k_bu_cols + k_vdv_cols" or "+ k_bu_cols + k_gram launches=1 .." where v^T D v takes a kernel of its own), "fp64 k_gram_mfma<...> launches=.. ny=.. +
 * k_vdv_cols", "fp64 k_gram launches=1 ..." (levels 1 and 2), "fp64 k_vdv_cols" (n_c = 0). */
int dmf_problem_gram_known(const dmf_problem* p, double* out, char* out_text, int64_t cap);
/* What a problem builder (create, gather, mask) left behind, for tests: the scalars here, the arrays through
 * dmf_problem_copy_out.  out_ints (DMF_REPORT_INTS host int64) <- N, S, n_c, ND (count digits; 0 = no integer copies), SD, N16,
 * plane_stride, then five 0 / 1 flags -- D16, X16, W16, Dt8 and the mask bits exist --, the row width of the padded R_trunc
 * copy in doubles (0: there is none), whether that copy is R_trunc itself (n_c % 4 == 0), n_test (held-out elements of a
 * masked problem) and d_f32_exact.  out_dbls (DMF_REPORT_DBLS host doubles) <- the six constants of the host copy in the
 * order of DMF_ARRAY_CONSTS, then x16_dev and x16_sum.  No address leaves the library.  DMF_ERR_BAD_ARG on a null pointer. */
enum { DMF_REPORT_INTS = 16, DMF_REPORT_DBLS = 8 };
int dmf_problem_report(const dmf_problem* p, int64_t* out_ints, double* out_dbls);
/* *out <- 1 when the problem carries the byte images X8 / D8 of its X16 / D16 (built by create, gather and mask alike when the
 * problem has X16, every count is at most 255 and 193 <= S <= 256: two more bytes per padded element), else 0. */
int dmf_problem_has_byte_images(const dmf_problem* p, int* out);
/* Where (row, sample) of a 16-row block and a 64-sample column group stands in its 1024-byte image; -1 outside 0..15 x 0..63.
 * A pure function, no GPU is touched.  The images: X8, D8 [N16 / 16][SD / 64][1024] bytes, the low bytes of X16 / D16. */
int dmf_rowpass_image_offset(int row, int sample);
/* One array of a problem as it stands on the device, for tests: waits for the context's stream and copies `bytes` bytes to the
 * host buffer `out`.  `bytes` must be the array's size (DMF_ERR_BAD_SHAPE otherwise): V, D N x S doubles; RT N x n_c; RTP
 * N x 4 ceil(n_c / 4) doubles (R_trunc itself where the report says so); D16, X16, W16 N16 x SD u16; DT8 ND planes of
 * plane_stride bytes, [plane][row block of 32][sample block of 32][n][k]; X8, D8 N16 x SD bytes (dmf_rowpass_image_offset); MASK_BITS N x ceil(S / 8) bytes; CONSTS the
 * device copy of the constants, six doubles: max(D)^2, ||Rt||_F^2, max(D), max |D - f32(D)|, max(D) if every count is a
 * non-negative integer else inf, 1 if R_trunc leaves [0, 1] else 0.  DMF_ERR_BAD_ARG for an array the problem does not have,
 * an unknown name or a null pointer. */
enum {
    DMF_ARRAY_V = 0, DMF_ARRAY_D = 1, DMF_ARRAY_RT = 2, DMF_ARRAY_RTP = 3, DMF_ARRAY_D16 = 4, DMF_ARRAY_X16 = 5,
    DMF_ARRAY_W16 = 6, DMF_ARRAY_DT8 = 7, DMF_ARRAY_MASK_BITS = 8, DMF_ARRAY_CONSTS = 9, DMF_ARRAY_X8 = 10, DMF_ARRAY_D8 = 11
};
int dmf_problem_copy_out(const dmf_problem* p, int which, void* out, int64_t bytes);

/* ---- single-function entry points (KAT parity of SURVEY.md section 8a rows 1-4) --------- */
/* cost_f_w(y, R, alpha, d_x), deconvolution.py:15-17, with R = [Rt | u]. */
int dmf_cost(dmf_context* ctx, const dmf_problem* p, const double* u, int64_t n_u,
             const double* alpha, int flags, double* out_cost);
/* Which kernel dmf_cost, dmf_solver_cost / _cost_begin and dmf_solver_holdout_error run for a key, as text naming the kernel
 * and its template arguments: "cost=k_cost_cols2<3,4,odd>" (two samples per lane; NKC = ceil(n_c / 4), NU = n_u, parity of
 * S), "cost=k_cost_cols<2,1,u16>" / "cost=k_cost_cols<0,4,f64>" (one sample per lane, on the u16 or the f64 counts),
 * "cost=k_cost alpha=lds" / "cost=k_cost alpha=global" (any shape).  The launch dispatches on the same plan
 * (csrc/dmf_kernels_stream.hip), so the text cannot say anything else than what runs.
 * dmf_cost_describe: a pure function of the key, no GPU is touched -- has_u16: the problem carries the u16 copy of its
 * counts (integers up to 32639, 2 <= S <= 2048, n_c <= 48, R_trunc in [0, 1], created at level 0), SD its padded row
 * length (S rounded up to 64), v_align the address of meth_frequency modulo 16, rtp_present the padded copy of R_trunc
 * (1 <= n_c <= 48), level the kernel selection level.  dmf_problem_cost_describe: the same for a resident problem at the
 * context's current level.  DMF_ERR_BAD_ARG for n_c + n_u outside [1, 64] and fields out of range. */
int dmf_cost_describe(int64_t S, int64_t n_c, int64_t n_u, int has_u16, int64_t SD, int v_align, int rtp_present, int level,
                      char* buf, int64_t cap);
int dmf_problem_cost_describe(dmf_context* ctx, const dmf_problem* p, int64_t n_u, char* buf, int64_t cap);
/* What the integer Gram (k_gram_i8_w8, csrc/dmf_kernels_gram_i8.hip) launches for a shape with nd = 1 | 2 count digit planes,
 * a pure function like dmf_cost_describe: "k_gram_i8_w8<2,2,6> launches=3 nsh=16 ny=16 blocks=9 last=8 tail=27 xcd=1" --
 * the template arguments <XL, ND, RING> (DMA pieces of a block's row image: 2 when padded n_c + n_u > 16; count digits; block
 * slots of the LDS ring), launches of 64 features each, nsh workgroups of 128 samples per row range, ny row ranges, 32-row
 * blocks of a full range and of the last one, tail = N % 32, xcd = 1 when ny % 8 == 0 (the kernel then keeps a range's
 * workgroups on one XCD).  n_u = 0 describes the known block (features = pairs of R_trunc columns).  The launcher dispatches on
 * the same plan.  DMF_ERR_UNSUPPORTED where the kernel does not take the shape (padded n_c + n_u > 32, more than 576
 * features, a row range whose i32 sums could overflow). */
int dmf_gram_i8_describe(int64_t N, int64_t S, int64_t n_c, int64_t n_u, int nd, char* buf, int64_t cap);
/* projection_simplex_sort_2d(v, z), deconvolution.py:21-37; X and out are K x S. */
int dmf_project_simplex(dmf_context* ctx, const double* X, int64_t K, int64_t S, double z,
                        int flags, double* out);
/* update_u(u, alpha, n_iter2, a1, l_w_, l_w, u_, meth_frequency, R_trunc, n_u, d_x),
 * deconvolution.py:81-90 -> (u, u_, a1, l_w_).  mode selects the gradient point (row 6 of
 * SURVEY.md section 8a).  scalars_io = {a1, l_w_prev, l_w} in, {a1, l_w_prev, l_w} out. */
int dmf_update_u(dmf_context* ctx, const dmf_problem* p, const double* u, const double* u_prev,
                 const double* alpha, int64_t n_u, int64_t n_iter2, int mode, int flags,
                 double* scalars_io, double* out_u, double* out_u_prev);
/* update_alpha(n_iter2, alpha, a2, l_h_, l_h, alpha_, R, d_x, meth_frequency),
 * deconvolution.py:93-102 -> (alpha, alpha_, a2, l_h_), with R = [Rt | u].
 * scalars_io = {a2, l_h_prev, l_h}. */
int dmf_update_alpha(dmf_context* ctx, const dmf_problem* p, const double* u, int64_t n_u,
                     const double* alpha, const double* alpha_prev, int64_t n_iter2, int flags,
                     double* scalars_io, double* out_alpha, double* out_alpha_prev);

/* wls_intercept(x, d_x, R_full), init_func.py:8-14 -- weighted non-negative least squares with intercept, renormalised to
 * proportions -- for every sample at once, with R_full = [Rt | u] (u may be NULL with n_u = 0), weights d_s and the target
 * v_s (DMF_WLS_TARGET_V: what the initialisers pass) or d_s v_s (DMF_WLS_TARGET_DV: what the reference-based run passes,
 * demethify.py:212).  Solved per sample from the centred normal equations G - m m^T / sw, r - m st / sw by Lawson-Hanson
 * with scipy's entry rule and cap of 3 K solves.  DMF_PTR_DEVICE in flags: u is a device array; out_alpha (K x S doubles)
 * and out_status (S ints) are host arrays, like dmf_cost's out_cost.  out_status: 0 ok, 1 not solved here (the sample's
 * K x K normal matrix is rank-deficient to K eps, or the cap was reached: solve that sample on the host), 2 the sample's
 * weights sum to zero (the reference raises ZeroDivisionError there); columns of out_alpha with a non-zero status are left
 * untouched.  K > 64: DMF_ERR_UNSUPPORTED.  DMF_WLS_F64_ARRAYS in flags: the first moments are taken from V and the f64 counts
 * even where the problem carries the u16 copies (x = v d as an exact integer), so that the result is the same bit for bit
 * with and without them: what the SVD initialiser asks for, whose residual is formed from the f64 V as well. */
enum { DMF_WLS_TARGET_V = 0, DMF_WLS_TARGET_DV = 1 };
enum { DMF_WLS_F64_ARRAYS = 8 };
int dmf_wls_intercept(dmf_context* ctx, const dmf_problem* p, const double* u, int64_t n_u, int target,
                      int flags, double* out_alpha, int* out_status);
/* The two halves of dmf_wls_intercept on their own, for tests; host pointers (u as dmf_wls_intercept takes it).
 * dmf_wls_moments: out_mom ((2 K + 2) x S host doubles) <- the first moments exactly as dmf_wls_intercept computes them for
 * the same arguments -- the same set-up, the same k_wls_moments / k_wls_reduce launches, DMF_WLS_F64_ARRAYS honoured alike:
 * rows 0 .. K - 1 m_k = sum_i d_is R_ik, rows K .. 2 K - 1 r_k = sum_i d_is t_is R_ik, row 2 K sw = sum_i d_is, row 2 K + 1
 * st = sum_i d_is t_is, with t = v (DMF_WLS_TARGET_V) or d v (DMF_WLS_TARGET_DV) and R = [Rt | u].
 * dmf_nnls_normal: k_nnls_intercept on a caller's system.  gb (K (K + 1) / 2 x S host doubles): the dense part of a packed
 * Gram, sample s of G_ij (i <= j) at gb[(j (j + 1) / 2 + i) S + s]; mom: a table laid out as above.  Each sample solves the
 * non-negative least squares problem with normal matrix G - m m^T / sw and right-hand side r - m st / sw.  out_status and
 * out_alpha as dmf_wls_intercept leaves them: the proportions coef / max(sum coef, 1e-10) in the columns with status 0, every
 * other column of out_alpha untouched.  K < 1 or S < 1: DMF_ERR_BAD_ARG; K > 64: DMF_ERR_UNSUPPORTED (both before the
 * context is looked at). */
int dmf_wls_moments(dmf_context* ctx, const dmf_problem* p, const double* u, int64_t n_u, int target, int flags,
                    double* out_mom);
int dmf_nnls_normal(dmf_context* ctx, const double* gb, const double* mom, int64_t K, int64_t S, double* out_alpha,
                    int* out_status);

/* The SVD initialiser -- constrained_nndsvd, init_func.py:17-37, and nndsvd_initialize, :40-82, reached from
 * deconvolution.py:68-71, :134-137 and :260-263 -- without an SVD of the N x S matrix.  With Yres = max(V - Rt H1, 1e-8)
 * (init_func.py:27; n_c = 0: V as it is, :135) the three calls below and a symmetric S x S eigendecomposition between the
 * first two, which stays with the caller (this library links no LAPACK), replace svd(Yres) of :44 and the loops of :47-71:
 * with C = Yres^T Yres = E diag(lambda) E^T, sigma_j = sqrt(lambda_j) and u_j = Yres e_j / sigma_j; the construction does not
 * depend on the joint sign of (u_j, e_j).  H1: the n_c x S regression coefficients of :21-23 (dmf_wls_intercept, target v),
 * a host array, or a device array with DMF_PTR_DEVICE in flags; NULL when n_c = 0.  Yres is formed on the fly from the
 * problem's f64 V and Rt, never stored.
 * Shapes: any N, S <= 512, n_c <= 64, rank <= 64 and 8 (S rank + 8 (64 ceil(S / 64) + 16) + 512) <= 163840 bytes (the projection
 * keeps the e_j / sigma_j columns in LDS: every rank up to S = 256, rank 30 at S = 512); beyond: DMF_ERR_UNSUPPORTED (take the
 * host route).
 * A masked problem (its held-out elements are zeros in V) is refused with DMF_ERR_BAD_ARG.
 *
 * dmf_svd_gram: out_C (S x S host doubles) <- Yres^T Yres, on the FP64 matrix cores, equal to its transpose bit for bit
 * and a function of the data and (N, S) alone; out_flags[2] <- the number of negative and of non-finite entries of V (what
 * :41-42 raises on, for the caller to raise).  A non-finite C: DMF_ERR_NONFINITE.  With profiling on, the two launches are
 * clocked under DMF_KERNEL_GRAM. */
int dmf_svd_gram(dmf_context* ctx, const dmf_problem* p, const double* H1, int flags, double* out_C, int64_t* out_flags);
/* dmf_svd_factor: E_over_sigma (S x rank host doubles, column j = e_j / sigma_j) -> *out_T, a device array of N x rank
 * doubles holding t_ij = u_ij (U of :44, columns 0 .. rank - 1), which belongs to the caller and is released with
 * dmf_stage_free; out_norms (2 x rank host doubles) <- per column the sums of max(t, 0)^2 and of max(-t, 0)^2: the squares
 * of n_uup and n_uun of :58-59 (summed in an order that depends on (N, S, rank) alone). */
int dmf_svd_factor(dmf_context* ctx, const dmf_problem* p, const double* H1, const double* E_over_sigma, int64_t rank,
                   int flags, double* out_norms, void** out_T);
/* dmf_svd_finish: T (N x rank, from dmf_svd_factor) <- u0, in place: x = scale_j |t| where sign_j = 0 (:50, component 0),
 * else scale_j max(sign_j t, 0) (:64 / :67, sign_j = +1 or -1 and scale_j = sqrt(sigma_j term) / norm as the caller chose
 * them at :63); x < 1e-11 -> 0 (:70); clipped to [0, 1] (:31, deconvolution.py:136).  out_u: N x rank host doubles; with
 * DMF_PTR_DEVICE in flags NULL or T itself (u0 stays in T for dmf_solver_create) or another device array. */
int dmf_svd_finish(dmf_context* ctx, void* T, int64_t N, int64_t rank, const double* sign, const double* scale, int flags,
                   double* out_u);

/* Bootstrap post-processing (bootstrap.py:51-54 proportions, :75-78 profile estimates):
 * np.percentile(x, q, axis=0) with numpy's default "linear" method, for x = [n replicates][m positions]
 * (C order), q = n_q percentiles in [0, 100]; out = [n_q][m].  Bit-identical to numpy for finite inputs
 * (NaNs are not ordered: inputs are proportions / methylation levels, never NaN).  n <= 19456. */
int dmf_percentile_axis0(dmf_context* ctx, const double* x, int64_t n, int64_t m, const double* q,
                         int64_t n_q, int flags, double* out);
/* np.nanpercentile(x, q, axis=0), same method, arguments and flags: the NaNs of a column are left out and the column's own
 * count n_c of numbers takes n's place in numpy's plan (virtual index (n_c - 1) q / 100, floor, gamma, clip to [0, n_c - 1]),
 * computed per column on the device.  A column without a number gives NaN, one number gives that number for every q.
 * Bit-identical to numpy; on input without NaNs the same bits as dmf_percentile_axis0.  n <= 19456.  For the profile
 * intervals by CpG (dmf_solver_get_u_by_row): a CpG is absent from the replicates that did not draw it. */
int dmf_nanpercentile_axis0(dmf_context* ctx, const double* x, int64_t n, int64_t m, const double* q,
                            int64_t n_q, int flags, double* out);

/* ---- solver: the outer loop, resident on the device --------------------------------------
 * mdwbssmf_deconv (deconvolution.py:190-223) / unsupervised_deconv's loop (:139-184).
 * create = state init (:192-204); step = up to n_outer outer iterations, stopping early when
 * |cf - cf_0| < tol (:220); get = copy out the current (u, alpha). */
int dmf_solver_create(dmf_context* ctx, const dmf_problem* p, const double* u0,
                      const double* alpha0, int64_t n_u, int mode, int flags, dmf_solver** out);
/* Purity-constrained variant (mdwbssmf_deconv_p, deconvolution.py:306-337): after this call the alpha
 * phase of every step is Frank-Wolfe (frank_wolfe_nmf, :280-302) with the known block of sample s held at
 * mass purity[s] and the unknown block at 1 - purity[s]; n_iter2 of dmf_solver_step is then also the
 * number of Frank-Wolfe iterations.  purity: S doubles.  Partial-reference mode only. */
int dmf_solver_set_purity(dmf_solver* s, const double* purity, int flags);
int dmf_solver_step(dmf_solver* s, int64_t n_outer, int64_t n_iter2, double tol,
                    int64_t* iters_done_total, int* converged);
int dmf_solver_get(dmf_solver* s, int flags, double* out_u, double* out_alpha,
                   double* out_cost, int64_t* out_iters);
/* Component matching, for the bootstrap (bootstrap.py:26-46 runs every replicate from a random draw of its own, so the
 * unknown types of two replicates come out in arbitrary order; upstream takes its percentiles over them as they come).
 * dmf_solver_match_components: out_P (n_u x n_u host doubles) <- P[a][b] = sum_j u[j][a] anchor[idx[j]][b] over the N rows
 * of the solver's current u, where anchor_dev is a device array of n_anchor_rows x n_u doubles (the profiles the components
 * are named after) and idx_dev the N int64 row indices in HBM that dmf_problem_gather_device was given for this solver's
 * problem; idx_dev NULL = the identity, which needs n_anchor_rows = N (DMF_ERR_BAD_SHAPE otherwise).  One pass over u and the
 * gathered anchor rows, plain FP64, every sum in an order fixed by (N, n_u): two calls give the same bits.  An index outside
 * [0, n_anchor_rows) is never dereferenced: the call returns DMF_ERR_BAD_ARG and leaves out_P untouched.  The assignment
 * that maximises sum_a P[a][perm[a]] stays with the caller.
 * dmf_solver_get_u_permuted: dst_dev (N x n_u device doubles, not the solver's own u) <- u[:, src_col], i.e.
 * dst[i][b] = u[i][src_col[b]]; src_col: n_u host ints, a permutation of 0 .. n_u - 1 (DMF_ERR_BAD_ARG otherwise).  Complete
 * when the call returns, like dmf_solver_get with DMF_PTR_DEVICE.
 * dmf_solver_get_u_by_row: the same copy with the rows put back by CpG.  idx_dev: the N int64 indices in HBM the solver's
 * problem was gathered with, so row j of u is CpG idx[j]; dst_dev (n_dst_rows x n_u device doubles, not the solver's own u)
 * <- dst[c][b] = u[first[c]][src_col[b]] with first[c] = min { j : idx[j] == c }, i.e. u[np.unique(idx,
 * return_index=True)[1]] scattered to its CpGs, and the quiet NaN 0x7ff8000000000000 in the rows of the CpGs that were not
 * drawn.  src_col as above, or NULL for the identity.  A pure gather: every copied value keeps its bits and two calls give
 * the same bits.  An index outside [0, n_dst_rows) is never dereferenced: the call returns DMF_ERR_BAD_ARG and leaves dst_dev
 * untouched.  Complete when the call returns.
 * With profiling on, the launches of all three are clocked under DMF_KERNEL_GRAM. */
int dmf_solver_match_components(dmf_solver* s, const void* anchor_dev, int64_t n_anchor_rows, const int64_t* idx_dev,
                                double* out_P);
int dmf_solver_get_u_permuted(dmf_solver* s, const int32_t* src_col, void* dst_dev);
int dmf_solver_get_u_by_row(dmf_solver* s, const int64_t* idx_dev, int64_t n_dst_rows, const int32_t* src_col /* NULL = identity */,
                            void* dst_dev);
/* cost_f_w(meth_f, [Rt | u], alpha, counts) of the solver's CURRENT iterate by the streaming formula
 * (deconvolution.py:15-17), without moving u / alpha to the host: what the restart and model-selection loops
 * recompute after every solve (demethify.py:169,199; ic.py:206).  out_cost: host double. */
int dmf_solver_cost(dmf_solver* s, double* out_cost);
/* The same in two halves, for loops that run solve after solve (demethify.py:165-171,195-201; bootstrap.py:26; ic.py:192):
 * _begin enqueues the cost of the current iterate and returns at once, _end waits for it -- in between the caller sets up
 * (and may start stepping) its NEXT solver on the same context, so the GPU works on the cost while the host prepares.
 * One cost in flight per solver; the iterate must not be stepped between the two calls. */
int dmf_solver_cost_begin(dmf_solver* s);
int dmf_solver_cost_end(dmf_solver* s, double* out_cost);
/* Hold-out error of a solver on a masked problem (dmf_problem_mask): *sum_sq = sum over the held-out (i, s) of
 * (v_is - sum_k R_ik alpha_ks)^2 with `full`'s meth_frequency and the solver's current iterate, R = [Rt | u] -- the squared
 * Frobenius norm of ic.py:80, before its division by *n_test, the number of held-out elements.  It is cost_f_w with 0 / 1
 * weights, run by the cost kernels where the iterate lives.  `full`: the problem the mask was applied to (same N, S, n_c:
 * DMF_ERR_BAD_SHAPE otherwise).  DMF_ERR_BAD_ARG when the solver's problem is not a masked one.  Nothing held out: 0, 0. */
int dmf_solver_holdout_error(dmf_solver* s, const dmf_problem* full, double* sum_sq, int64_t* n_test);
/* The solver's packed Gram for its CURRENT u, computed now, for tests: out_gb ((K + 1)(K + 2) / 2 x S host doubles, row
 * tri(k, l) as above over (R_trunc columns, u columns, v)) <- the known block as it stands plus the u-dependent entries
 * (cross, uu) and b_u, by the functions a step itself calls.  kind = DMF_GRAM_INTEGER: k_bu_cols / k_bu_cols2, k_gram_i8_w8,
 * k_gram_v2_reduce, k_gram_v2_finish, whatever path the solver itself runs, in temporaries of its own; u MUST lie in [0, 1]
 * (the fixed-point features: true of every iterate behind a u phase, the caller's business for a u0); DMF_ERR_UNSUPPORTED
 * without integer count copies or where dmf_gram_i8_describe says so.  kind = DMF_GRAM_FP64: k_gram_u, k_gram_mfma or k_gram,
 * as the solver's selection names at the level it was created at.  A converged solver computes too (no done flag is passed);
 * u_norm2 / l_h and the iterate are left alone, and the solver's own Gram buffer is rewritten by the next step before it
 * is read, so stepping on gives the same bits as without this call.  out_text (may be NULL): what ran, the text of
 * dmf_gram_i8_describe, or "k_gram_u<NCT,NU> launches=1 ny=..", "k_gram_mfma<MTW,dma|reg> launches=.. ny=..",
 * "k_gram launches=1 ny=.. nz=..".  kind = DMF_GRAM_LAST computes nothing: out_gb <- the solver's own packed Gram exactly as
 * the last outer iteration of dmf_solver_step left it -- the Gram of the current u, since the alpha phase behind it does not
 * change u -- and out_text <- what wrote its u-dependent rows there ("k_rowpass_fused<3,4> phase C slabs=512 + k_gram_u
 * tail", or the text of the loop's Gram launcher); before any iteration the u-dependent rows are zero and the text empty.
 * (A call with one of the other two kinds rewrites that buffer: ask for DMF_GRAM_LAST first.) */
enum { DMF_GRAM_INTEGER = 0, DMF_GRAM_FP64 = 1, DMF_GRAM_LAST = 2 };
int dmf_solver_gram(dmf_solver* s, int kind, double* out_gb, char* out_text, int64_t cap);
/* The per-row moments of the split u phase for the solver's CURRENT alpha, computed now, for tests: out_cm (N x NV host
 * doubles, NV = n_u + n_u (n_u + 1) / 2) <- row i: c_i = alpha_unk (d_i * (v_i - Rt_i alpha_known))^T (n_u values), then
 * M_i[p] = sum_s alpha_js alpha_ls d_is in packed pair order p = l (l + 1) / 2 + j, j <= l.  It runs the PRODUCER that the
 * split form of this solver's stand-alone u phase launches (what dmf_update_u takes beyond 50 inner steps, and at every count
 * for wide row groups) -- k_cm_i8, or k_u_phase_mfma in split mode -- into the solver's own scratch and copies that out; no
 * inner iteration runs, the iterate is left alone, and every u phase rewrites the scratch before it reads it, so stepping on
 * gives the same bits as without this call.  out_text (may be NULL; 2 KB hold every plan): the producer's launch plan --
 * the part of dmf_solver_u_phase_describe(.., DMF_ROUTE_UPDATE_U, ..) behind "k_cm_i8<nd=..>+k_u_inner_rows ", or the whole
 * "k_u_phase_mfma<..> split .." text.  DMF_ERR_UNSUPPORTED where that u phase has no split form (k_u_phase_big,
 * k_u_phase_gram, k_u_step_direct).  The producers do nothing once the stop test has fired, so a solver that has stopped is
 * refused with DMF_ERR_BAD_ARG instead of handing out an earlier iteration's scratch. */
int dmf_solver_row_moments(dmf_solver* s, double* out_cm, char* out_text, int64_t cap);
/* The momentum state of the outer loop as it stands on the device, for tests: waits for the context's stream, then
 * scalars (DMF_MOMENTUM_SCALARS host doubles) <- a1, a2, l_w, l_w_prev, l_h, l_h_prev, dsq, rt_norm2, u_norm2, cf, cf_prev,
 * then iters, done, arrive, mom_n, mom_i as doubles (mom_n = -1 / 0: no momentum rows in use); alpha_prev (K x S host
 * doubles, may be NULL) <- the previous alpha of the alpha phase; u_prev (N x n_u host doubles, may be NULL) <- the previous u
 * of the u phase.  Read-only: nothing is launched and nothing on the device or in the solver changes, so stepping on gives
 * the same bits as without this call.  (cf is the loop's cost only once an iteration has run.) */
enum { DMF_MOMENTUM_SCALARS = 16 };
int dmf_solver_momentum_state(const dmf_solver* s, double* scalars, double* alpha_prev, double* u_prev);
int dmf_solver_destroy(dmf_solver* s);
/* Which kernels a step with n_iter2 inner iterations would launch for this solver, as text, e.g.
 * "rowpass=k_rowpass_fused<3,4> nw=4 grid=256 tail=5 gram=fused alpha=k_alpha_phase_row16".  For tests (every
 * parity case asserts the path it means to cover) and for bench.py's kernel label.  buf gets at most cap bytes
 * including the terminator. */
int dmf_solver_describe(const dmf_solver* s, int64_t n_iter2, char* buf, int64_t cap);
/* The same text for a shape that need not exist on a device: the kernel-selection table itself (csrc/dmf_select.hip),
 * a pure function of (N, S, n_c, n_u, count digit planes nd = 0 | 1 | 2, kernel level, n_iter2, DMF_SELECT_* flags).
 * No GPU is touched: tests/test_host.py enumerates a grid of shapes against tests/golden/kernel_selection.tsv.
 * DMF_ERR_UNSUPPORTED where no kernel takes the shape. */
int dmf_select_describe(int64_t N, int64_t S, int64_t n_c, int64_t n_u, int nd, int level, int64_t n_iter2, int flags,
                        char* buf, int64_t cap);
/* The u phase alone, with what its launcher launches, for the same key (dmf_u_phase_describe: pure, no GPU is touched) or
 * for a live solver.  route = DMF_ROUTE_SOLVER: the u phase of an outer iteration of dmf_solver_step; DMF_ROUTE_UPDATE_U:
 * the stand-alone u phase of dmf_update_u (no one-launch row pass, no fused kernel).  For the first-generation FP64 row
 * kernels the text is the plan the launcher itself launches from -- template arguments, mode, waves per workgroup, grid,
 * dynamic LDS bytes, whether the LDS limit is raised first, and the largest number of row blocks a workgroup takes:
 *   "k_u_phase_mfma<2,3,vec,d16> split nw=2 grid=512 lds=6912 raise=0 blocks/wg=3"   (scalar | vec | vec,d16; one-launch | split)
 *   "k_rowpass_fused<3,4> nw=4 grid=256 lds=.. raise=1 blocks/wg=3 tail=5"           (nw column groups; 3 nw waves run)
 *   "k_u_phase_big<0,16> n_u=12 nw=4 grid=512 lds=.. raise=0 blocks/wg=2"
 *   "k_u_phase_gram<3> alpha=lds nw=4 grid=.. lds=.. raise=0 blocks/wg=1"            (alpha=lds | global)
 *   "k_u_step_direct n_u=5 nw=4 grid=.. lds=.. raise=0 blocks/wg=2 launches=20"
 * (row blocks of 16 rows; k_u_phase_gram 64, k_u_step_direct 4).  For the split u phase on the integer producer it is the
 * rowpass= part of dmf_select_describe, then the plan launch_cm_i8 dispatches on, one entry per panel of 256 samples:
 *   "k_cm_i8<nd=1>+k_u_inner_rows panels=2 tiles=10 | col0=0 sp=256 k_cm_i8<1,1,4,s4> tpl=5 launches=2 ctiles=2 lds=..
 *    grid=.. blocks/wave=1 | col0=256 sp=44 k_cm_i8<1,1,2,s4> tpl=5 .."
 * k_cm_i8<NKC,ND,NCGX,s4|pairs>; tiles: 16-pair tiles of M_i, tpl of them per launch; ctiles: 16-unknown tiles of c; lds, grid
 * and blocks/wave (32-row blocks of the busiest wave) are the first launch's -- where the last launch holds fewer tiles,
 * " last: tiles=.. lds=.. grid=.. blocks/wave=.." follows.  (2 KB hold every such text.)  For the one-launch row pass
 * k_rowpass_v2 it is the rowpass= part of dmf_select_describe, then the plan launch_rowpass_v2 dispatches on -- template
 * argument MAXW, the schedule (one | pair | deferred | bytes: one block per barrier cycle, two, phase C deferred, the same
 * from the byte images) and the launch as above:
 *   "k_rowpass_v2<3,4> nw=4 grid=512 tail=0 x16 maxw=4 bytes nw=4 grid=512 lds=.. raise=1 blocks/wg=123"
 * so a test knows, before any launch, which schedule a solver runs.  DMF_ERR_UNSUPPORTED where no kernel takes the shape. */
enum { DMF_ROUTE_SOLVER = 0, DMF_ROUTE_UPDATE_U = 1 };
int dmf_u_phase_describe(int64_t N, int64_t S, int64_t n_c, int64_t n_u, int nd, int level, int64_t n_iter2, int flags, int route,
                         char* buf, int64_t cap);
int dmf_solver_u_phase_describe(const dmf_solver* s, int64_t n_iter2, int route, char* buf, int64_t cap);
/* How the stop test |cf - cf_0| < tol (deconvolution.py:218-220) of this solver's dmf_solver_step calls was decided.
 * The loop's cost is the Gram form v^T D v - 2 a.b + a^T G a; where its error bound (it grows with N S max(counts)) is
 * not far below tol, an iteration whose Gram-form difference falls below 10 tol is decided on the STREAMING cost of
 * deconvolution.py:15-17 for this and the previous iterate (confirm_stops = 1; n_confirmed such decisions so far,
 * n_unconfirmed decisions inside that band that had only the Gram form -- the first iteration to enter it);
 * last_stream_cost = the latest streaming cost taken for a stop test (NaN: none).  Any pointer may be NULL. */
int dmf_solver_stop_info(const dmf_solver* s, int* confirm_stops, int64_t* n_confirmed, int64_t* n_unconfirmed,
                         double* last_stream_cost);
/* How many k_rowpass_v2 launches this solver's steps have enqueued (total) and how many of them ran the pair schedule
 * (paired; see dmf_context_set_rowpass_pair).  Tests and A/B runs.  Either pointer may be NULL. */
int dmf_solver_rowpass_launches(const dmf_solver* s, int64_t* total, int64_t* paired);
/* The same, and how many of the paired launches ran the deferred-C schedule (deferred; see
 * dmf_context_set_rowpass_defer_c).  Any pointer may be NULL. */
int dmf_solver_rowpass_schedule_counts(const dmf_solver* s, int64_t* total, int64_t* paired, int64_t* deferred);
/* How many of the deferred launches read the problem's byte images (see dmf_context_set_rowpass_bytes). */
int dmf_solver_rowpass_byte_launches(const dmf_solver* s, int64_t* bytes);
/* One-shot convenience: create + step(n_iter1) + get + destroy. */
int dmf_solve(dmf_context* ctx, const dmf_problem* p, const double* u0, const double* alpha0,
              int64_t n_u, int mode, int64_t n_iter1, int64_t n_iter2, double tol, int flags,
              double* out_u, double* out_alpha, double* out_cost, int64_t* out_iters);

/* ---- small problems: B independent solves of one resident problem per launch, one workgroup per solve.
 * The whole outer loop of mdwbssmf_deconv (demethify/deconvolution.py:190-223, DMF_MODE_PARTIAL) or unsupervised_deconv
 * (:107-184, DMF_MODE_UNSUPERVISED) runs inside one kernel: set-up as :192-204 (a1 = a2 = 1, u_ = u0, alpha_ = alpha0,
 * d = max(counts)^2, l_w, l_h, the cost), then per outer iteration the u phase (:81-90; the gradient at u_temp in partial
 * mode, at the previous iterate in unsupervised mode, :163), l_h (:212), the alpha phase with the sort-based simplex
 * projection (:93-102, :21-37), l_w (:216), the streaming cost sum d (v - R alpha)^2 (:15-17) and the stop test
 * fabs(cf - cf_0) < tol on that cost (:218-220).  No Gram-form cost and no confirmation of stops take part.
 * dmf_solve_small_supported: 1 where the kernel takes the shape, else 0 -- modes DMF_MODE_PARTIAL and DMF_MODE_UNSUPERVISED,
 * 1 <= n_u <= 4, n_c + n_u <= 16, S <= 64, N S <= 2^20 (that bounds how long one launch can run; it is not a measured
 * cross-over).  Pure: no context, no GPU.
 * dmf_solve_small: solve b of B starts from u0[b] (N x n_u) and alpha0[b] (K x S).  idx NULL: every solve runs on the problem's
 * own N rows.  idx given (B x N int64): row i of solve b is row idx[b][i] of the problem, read through the index without a
 * gathered copy -- a bootstrap replicate (demethify/bootstrap.py:28) -- and d is the maximum over the drawn rows.  With
 * DMF_PTR_DEVICE in flags idx, u0, alpha0 and out_u are device arrays; out_alpha (B x K x S), out_cost (B) and out_iters (B)
 * are host arrays.  out_cost[b] is cost_f_w of the final iterate, what the restart pick compares (demethify/demethify.py:199);
 * out_iters[b] the outer iterations solve b ran (at most n_iter1).  A launch runs at most iters_per_launch outer iterations
 * per solve (0: the library's default); between launches the host reads the B stop flags and ends when every solve has
 * stopped or n_iter1 is reached.  All per-solve state is kept in HBM between launches, so the results are the same bit for
 * bit for every iters_per_launch; they do not depend on B, on a solve's slot or on the other solves either.
 * DMF_ERR_UNSUPPORTED outside the envelope, before the context is touched.  DMF_ERR_BAD_ARG: B < 1, a null array, a negative
 * iteration count, a masked problem (as dmf_svd_gram), an index outside [0, N) -- every index is checked on the device
 * before the first launch, as dmf_problem_gather_device checks its own, so no solve has started.  Inputs are never written. */
int dmf_solve_small_supported(int64_t N, int64_t S, int64_t n_c, int64_t n_u, int mode);
int dmf_solve_small(dmf_context* ctx, const dmf_problem* p, int64_t B, const int64_t* idx, const double* u0,
                    const double* alpha0, int64_t n_u, int mode, int64_t n_iter1, int64_t n_iter2, double tol,
                    int64_t iters_per_launch, int flags, double* out_u, double* out_alpha, double* out_cost,
                    int64_t* out_iters);
/* dmf_solve_small_purity: the same B solves under the purity constraint -- mdwbssmf_deconv_p
 * (demethify/deconvolution.py:306-337) with the Frank-Wolfe alpha phase frank_wolfe_nmf (:280-302), i.e.
 * deconvolution.py:280-302,306-337.  Set-up: a1 = 1, u_ = u0, d = max(counts)^2, l_w, the cost; there is no a2, no l_h and no
 * alpha_.  Per outer iteration the u phase as above, then per sample n_iter2 Frank-Wolfe steps restarting at k = 0 from the
 * current alpha: grad = G_s a - b_s, the first-index argmin over the known rows and over the unknown rows, mass purity[s] on
 * the known vertex and 1 - purity[s] (taken in f64) on the unknown one, gamma = 2 / (k + 2),
 * a = (1 - gamma) a + gamma vertex with every product and the sum rounded; then l_w, the streaming cost and the stop test.
 * purity: S doubles shared by all B solves, a host array, or a device array with DMF_PTR_DEVICE in flags.  Everything else
 * is dmf_solve_small's: arguments, envelope (dmf_solve_small_supported), workspace, idx, determinism.  DMF_MODE_PARTIAL only
 * (another mode: DMF_ERR_UNSUPPORTED); a null purity or a problem without a reference (n_c < 1): DMF_ERR_BAD_ARG -- all
 * before the context is touched.  A masked problem is refused as by dmf_solve_small. */
int dmf_solve_small_purity(dmf_context* ctx, const dmf_problem* p, int64_t B, const int64_t* idx, const double* u0,
                           const double* alpha0, const double* purity, int64_t n_u, int mode, int64_t n_iter1,
                           int64_t n_iter2, double tol, int64_t iters_per_launch, int flags, double* out_u,
                           double* out_alpha, double* out_cost, int64_t* out_iters);
/* dmf_solve_small_masked: the same B solves, each on its own hold-out mask -- the folds of a bi-cross-validation
 * (demethify/ic.py:58-89) in one call.  train_bits: B x N x ceil(S / 8) bytes in dmf_problem_mask's layout (row-major, sample s
 * in bit (s & 7) of byte (s >> 3), 1 = kept, 0 = held out, padding bits ignored); a host array, or a device array with
 * DMF_PTR_DEVICE in flags.  Solve b sees the count of an element as 0 where its bit is 0 (`counts * train_mask`, ic.py:75)
 * in every place the kernel reads a count: d = max(counts)^2 is the maximum over the kept elements, the known Gram block,
 * the u phase, the Gram, the streaming cost and therefore the stop test.  v of a held-out element is only ever multiplied
 * by that 0 (`meth_f * train_mask`: V is finite).  out_cost[b] is cost_f_w of the final iterate on the masked data.  After the
 * last launch the hold-out error is taken where the iterates live: out_holdout_sum_sq[b] = sum over the held-out elements of
 * (v - [R_trunc | u_b] alpha_b)^2 on the problem's full V (ic.py:80 before the division), out_n_test[b] = N S minus the
 * number of kept elements (B host doubles, B host int64).  A mask that holds out nothing is valid: 0.0 and 0.
 * Arguments, conventions, envelope, workspace and determinism are dmf_solve_small's: a solve's results do not depend on B, on
 * its slot, on the other solves' masks or on iters_per_launch, bit for bit; an all-ones mask gives dmf_solve_small's results
 * bit for bit.  There is no idx and no purity here.  DMF_ERR_UNSUPPORTED outside the envelope, before the context is touched.
 * DMF_ERR_BAD_ARG: a null train_bits, a masked p, a solve whose mask keeps no element (upstream skips such a fold, ic.py:71;
 * d would be 0) -- the kept elements are counted on the device before any solve starts, and the outputs stay untouched. */
int dmf_solve_small_masked(dmf_context* ctx, const dmf_problem* p, int64_t B, const uint8_t* train_bits, const double* u0,
                           const double* alpha0, int64_t n_u, int mode, int64_t n_iter1, int64_t n_iter2, double tol,
                           int64_t iters_per_launch, int flags, double* out_u, double* out_alpha, double* out_cost,
                           int64_t* out_iters, double* out_holdout_sum_sq, int64_t* out_n_test);

/* ---- mid-size problems: B independent solves of one resident problem, W >= 1 workgroups per solve, three launches per
 * outer iteration for all B solves.  The arithmetic is dmf_solve_small's and therefore the reference's: mdwbssmf_deconv
 * (demethify/deconvolution.py:190-223, DMF_MODE_PARTIAL) or unsupervised_deconv (:107-184, DMF_MODE_UNSUPERVISED) -- set-up as
 * :192-204, the row-local u phase (:81-90; the gradient at u_temp in partial mode, at the previous iterate in unsupervised
 * mode, :163), l_h (:212), the alpha phase with the sort-based projection (:93-102, :21-37), l_w (:216), the streaming cost
 * (:15-17) and the stop test fabs(cf - cf_0) < tol on it (:218-220); no Gram-form cost, no confirmation of stops.  Only the
 * orders of the sums over rows differ: a solve's rows are cut into W slabs of `rows` rows (a multiple of 256, the last slab
 * may be ragged, W <= 64), one workgroup per slab, and a sum over rows is a sum per slab followed by the sum of the slab
 * partials in rising slab order.  Workgroups meet at launch boundaries only; there are no atomics; every order depends on
 * (N, S, n_c, n_u, rows) alone.
 * dmf_solve_mid_supported: 1 where the kernels take the shape, else 0 -- the two modes, 1 <= n_u <= 4, n_c + n_u <= 16,
 * S <= 64, N S <= 2^23 (that bounds the workspace; it is not a measured cross-over).  Pure: no context, no GPU.
 * dmf_solve_mid_plan: the plan of an N x S solve -- *out_rows rows per workgroup, *out_W workgroups per solve with
 * (W - 1) rows < N <= W rows, *out_check_every outer iterations between two reads of the stop flags.  rows_per_workgroup 0:
 * the default, the smallest multiple of 256 with W <= 64; the default check_every is 2^22 / (N S) within [4, 16].  Both are
 * functions of (N, S) alone.  DMF_ERR_BAD_ARG: N or S below 1, a rows_per_workgroup that is not a positive multiple of 256 or
 * that gives W > 64, a null pointer.  Pure: no context, no GPU.
 * dmf_solve_mid: dmf_solve_small's contract -- B, idx (B x N int64 or NULL; a bootstrap replicate, demethify/bootstrap.py:28,
 * d being the maximum over the drawn rows), u0, alpha0, DMF_PTR_DEVICE in flags, out_u / out_alpha / out_cost / out_iters,
 * out_cost[b] = cost_f_w of the final iterate (demethify/demethify.py:199), out_iters[b] its outer iterations, inputs never
 * written -- with rows_per_workgroup (0: the default) and check_every (0: the default) in the place of iters_per_launch.
 * The host enqueues check_every outer iterations, reads the B stop flags and ends when every solve has stopped or n_iter1
 * is reached; the launches of a stopped solve return at once and its iterate is never touched again.  A solve's results do
 * not depend on B, on its slot, on the other solves or on check_every, bit for bit; rows_per_workgroup changes the order of
 * the sums over rows and with it the last bits.  DMF_ERR_UNSUPPORTED outside the envelope, before the context is touched.
 * DMF_ERR_BAD_ARG: B < 1, a null array, a negative count, a bad rows_per_workgroup (as above), a masked problem, an index
 * outside [0, N) -- every index is checked on the device before any solve starts.  The purity-constrained solve is
 * dmf_solve_mid_purity, the one with a hold-out mask per solve dmf_solve_mid_masked, both below. */
int dmf_solve_mid_supported(int64_t N, int64_t S, int64_t n_c, int64_t n_u, int mode);
int dmf_solve_mid_plan(int64_t N, int64_t S, int64_t rows_per_workgroup, int64_t* out_rows, int64_t* out_W,
                       int64_t* out_check_every);
int dmf_solve_mid(dmf_context* ctx, const dmf_problem* p, int64_t B, const int64_t* idx, const double* u0,
                  const double* alpha0, int64_t n_u, int mode, int64_t n_iter1, int64_t n_iter2, double tol,
                  int64_t rows_per_workgroup, int64_t check_every, int flags, double* out_u, double* out_alpha,
                  double* out_cost, int64_t* out_iters);
/* dmf_solve_mid_purity: the same B solves under the purity constraint -- mdwbssmf_deconv_p (demethify/deconvolution.py:306-337)
 * with the Frank-Wolfe alpha phase frank_wolfe_nmf (:280-302), the arithmetic of dmf_solve_small_purity: no a2, no l_h, no
 * alpha_; per outer iteration the u phase, then per sample n_iter2 Frank-Wolfe steps restarting at k = 0 from the current alpha
 * (grad = G_s a - b_s, the first-index argmin over the known rows and over the unknown rows, mass purity[s] on the known
 * vertex and 1 - purity[s] on the unknown one, gamma = 2 / (k + 2), every product and the sum rounded), l_w, the streaming
 * cost and the stop test.  The launches are dmf_solve_mid's with one alpha launch of its own (one workgroup per solve, a
 * 16-lane row per sample, all samples stepping at once); the workspace is dmf_solve_mid's and gains nothing per slab.
 * purity: S doubles shared by all B solves, a host array, or a device array with DMF_PTR_DEVICE in flags.  Everything else is
 * dmf_solve_mid's: arguments, plan, idx, determinism, the envelope dmf_solve_mid_supported in DMF_MODE_PARTIAL with n_c >= 1.
 * DMF_ERR_UNSUPPORTED, before the context is touched: outside the envelope; DMF_MODE_UNSUPERVISED on a problem with a
 * reference.  DMF_ERR_BAD_ARG: a null purity, a problem without a reference (n_c < 1), a masked problem, and every refusal of
 * dmf_solve_mid.  Inputs are never written. */
int dmf_solve_mid_purity(dmf_context* ctx, const dmf_problem* p, int64_t B, const int64_t* idx, const double* u0,
                         const double* alpha0, const double* purity, int64_t n_u, int mode, int64_t n_iter1,
                         int64_t n_iter2, double tol, int64_t rows_per_workgroup, int64_t check_every, int flags,
                         double* out_u, double* out_alpha, double* out_cost, int64_t* out_iters);
/* dmf_solve_mid_masked: the same B solves, each on its own hold-out mask -- the folds of a bi-cross-validation
 * (demethify/ic.py:58-89) in one call, several workgroups per fold.  train_bits, what a solve sees of a held-out element,
 * out_cost, out_holdout_sum_sq and out_n_test are dmf_solve_small_masked's: B x N x ceil(S / 8) bytes in dmf_problem_mask's
 * layout (sample s in bit (s & 7) of byte (s >> 3), 1 = kept, padding bits ignored), a host array or a device array with
 * DMF_PTR_DEVICE; the count of an element is 0 where its bit is 0 in the maximum count (taken over the kept elements), the
 * known Gram block, the u phase, the Gram, the streaming cost and therefore the stop test; out_cost[b] = cost_f_w of the final
 * iterate on the masked data, out_holdout_sum_sq[b] = the sum over the held-out elements of (v - [R_trunc | u_b] alpha_b)^2 on
 * the problem's full V, out_n_test[b] = N S minus the kept elements.  The launches are dmf_solve_mid's, in their masked
 * instances, between two passes of a workgroup per slab: the kept elements are counted before any solve starts, the hold-out
 * error is taken after the last iteration (per slab, the slab partials added in rising slab order).  Everything else is
 * dmf_solve_mid's: arguments, plan, determinism -- a solve's results do not depend on B, on its slot, on the other solves'
 * masks or on check_every, bit for bit, and an all-ones mask gives dmf_solve_mid's results bit for bit.  There is no idx and
 * no purity here.  DMF_ERR_UNSUPPORTED outside dmf_solve_mid_supported, before the context is touched.  DMF_ERR_BAD_ARG: a null
 * train_bits, a masked p, a solve whose mask keeps no element (the outputs stay untouched), and every refusal of
 * dmf_solve_mid. */
int dmf_solve_mid_masked(dmf_context* ctx, const dmf_problem* p, int64_t B, const uint8_t* train_bits, const double* u0,
                         const double* alpha0, int64_t n_u, int mode, int64_t n_iter1, int64_t n_iter2, double tol,
                         int64_t rows_per_workgroup, int64_t check_every, int flags, double* out_u, double* out_alpha,
                         double* out_cost, int64_t* out_iters, double* out_holdout_sum_sq, int64_t* out_n_test);

/* ---- input tables (host side) ---------------------------------------------------------------
 * demethify/demethify.py:103-143 reads each sample file with pandas.read_csv and stacks its `percent_modified` and
 * `valid_coverage` columns.  dmf_table_scan finds the two columns by header name and counts the data rows;
 * dmf_table_read parses them (n_threads threads) into strided destinations: out_freq[row * stride_freq] =
 * value / divide_by (100 for bedmethyl percentages, 1 for csv fractions), out_cov[row * stride_cov] = coverage
 * (col_valid_coverage < 0: no such column, out_cov untouched).  Values are bit-identical to pandas' default parser; any
 * content that parser treats specially (quotes, NA spellings, blank lines, non-integer coverage) yields
 * DMF_ERR_UNSUPPORTED and the caller reads that file with pandas.  dmf_host_alloc returns page-locked host memory when a
 * GPU runtime is present (*pinned = 1), plain memory otherwise. */
int dmf_table_scan(const char* path, char sep, int64_t* n_rows, int* col_percent_modified, int* col_valid_coverage,
                   int* n_cols);
int dmf_table_read(const char* path, char sep, int col_percent_modified, int col_valid_coverage, int64_t n_rows,
                   double* out_freq, int64_t stride_freq, double divide_by, int64_t* out_cov, int64_t stride_cov,
                   int n_threads);
void* dmf_host_alloc(size_t bytes, int* pinned);
void dmf_host_free(void* p, int pinned);

/* ---- output tables.  The profile confidence intervals go out as the reference writes them (demethify/bootstrap.py:85-91:
 * a DataFrame of (lower, upper) tuples through DataFrame.to_csv): header_line, then per row the n_cols quoted cells
 * "(lo, hi)" -- or "(np.float64(lo), np.float64(hi))" with numpy_scalar_repr != 0, what numpy >= 2 makes of the same
 * tuple -- floats as repr() prints them.  lower / upper are row-major (n_rows x n_cols).  Byte-identical to pandas. */
int dmf_write_interval_csv(const char* path, const char* header_line, const double* lower, const double* upper,
                           int64_t n_rows, int n_cols, int numpy_scalar_repr, int n_threads);

/* ---- restart staging.  The reference draws a fresh (u0, alpha0) per restart and solves it, one after the other
 * (demethify/demethify.py:165-171 and 195-201).  dmf_stage_upload copies a host array (page-locked memory from
 * dmf_host_alloc makes it a direct DMA) to a new device buffer on a copy stream of the context's own and returns when
 * the copy is complete; it may be called from a worker thread while the context's stream iterates the restart before.
 * The buffer is then passed to dmf_solver_create with DMF_PTR_DEVICE and released with dmf_stage_free (ordered behind
 * the context's stream). */
int dmf_stage_upload(dmf_context* ctx, const void* host, size_t bytes, void** out_dev);
int dmf_stage_free(dmf_context* ctx, void* dev);
/* The way back, for a buffer the staging calls made (dmf_stage_upload, dmf_mask_draw): `bytes` bytes from `dev` to the host
 * array, on the copy stream, under dmf_stage_upload's threading contract; returns when the copy is complete. */
int dmf_stage_download(dmf_context* ctx, const void* dev, size_t bytes, void* host);

/* ---- hold-out mask draw.  A bi-cross-validation fold's train mask is `np.random.rand(*meth_f.shape) < fraction` of numpy's
 * legacy global generator (ic.py:68): MT19937, whose doubles are integer arithmetic on pairs of its words.  dmf_mask_draw
 * continues that stream on the device and writes the mask straight into the packed form dmf_problem_mask reads, the same
 * bit for bit as the host draw from the same state.  key / *pos: the generator's 624 words and position (0..624; 624 =
 * regenerate first, the state right after seed()), i.e. np.random.get_state()[1:3]; both are updated in place to the state
 * after rand(N, S) -- the key as of the last regeneration, the position behind the last word used -- for set_state.
 * threshold: x < fraction as an integer compare on x 2^53: 0 for fraction <= 0 or NaN, 2^53 for fraction >= 1, else
 * ceil(fraction 2^53) (the product is exact).  *out_bits: a new device buffer of N ceil(S / 8) bytes, every byte written,
 * padding bits zero -- what dmf_problem_mask takes with DMF_PTR_DEVICE -- released with dmf_stage_free; *n_kept: the number of
 * ones.  Where dmf_mask_draw_plan says one segment, one persistent workgroup walks the stream (the recurrence itself allows
 * no more); else the stream is cut into segments, their keys come from the caller's by jump-ahead, and one workgroup per
 * segment draws -- the same results either way.
 * Threading as dmf_stage_upload: it runs on the context's copy stream, may be called from a worker thread while the
 * context's stream iterates, and returns when the mask and the three results are complete.  DMF_ERR_BAD_ARG: a position
 * outside [0, 624], N or S below 1, a threshold above 2^53, a null pointer; DMF_ERR_UNSUPPORTED: S >= 2^31 or more than 2^60
 * elements.  After an error nothing stays allocated and key / *pos are untouched. */
int dmf_mask_draw(dmf_context* ctx, uint32_t key[624], int* pos, int64_t N, int64_t S,
                  uint64_t threshold, void** out_bits, int64_t* n_kept);

/* The segmented draw.  The stream is cut on numpy's own grid of 624-word blocks -- block 0 the caller's key, used from word
 * *pos -- into segments of blocks_per_segment blocks.  A segment's starting key is the caller's carried forward by a
 * polynomial: with phi the characteristic polynomial of MT19937 and g = t^J mod (t phi), word m of the key J words on is the
 * XOR of the raw words x[i + m] over the non-zero terms i of g (modulo t phi, not phi: the low 31 bits of word 0 of an
 * arbitrary key are output but are no part of the state, and a remainder divisible by t never reads them).  The keys are
 * made on the device in rounds that multiply their number by 32 (two launches for 1024 segments); the polynomials are computed on the host at first
 * use and kept per process.  Every byte of the mask is written by exactly one workgroup, the one whose segment holds the
 * byte's first element.
 * dmf_mask_draw_plan: what dmf_mask_draw does for a shape, a function of (N, S) alone and no GPU touched: *segments <=
 * DMF_MASK_DRAW_MAX_SEGMENTS of *blocks_per_segment blocks, together at least the 2 N S + 624 words a draw can reach; one
 * segment is the one-workgroup kernel.  DMF_ERR_BAD_ARG: N or S below 1, a null pointer; DMF_ERR_UNSUPPORTED as above.
 * dmf_mask_draw_segments: dmf_mask_draw with the segment length given -- blocks_per_segment 0: the plan's choice (that is
 * dmf_mask_draw), -1: one workgroup, >= 1: segments of that many blocks, DMF_ERR_BAD_ARG if the shape would need more than
 * DMF_MASK_DRAW_MAX_SEGMENTS of them (or below -1).  Results, threading and errors as dmf_mask_draw.
 * dmf_mt_jump: host only, no context.  Advances numpy's legacy state (key, *pos) exactly as consuming n_words 32-bit words
 * would: the key comes back as of the last regeneration on numpy's grid, *pos as numpy would report it; n_words = 0 leaves
 * both untouched.  DMF_ERR_BAD_ARG: a null pointer, *pos outside [0, 624].  Thread-safe. */
#define DMF_MASK_DRAW_MAX_SEGMENTS 1024
int dmf_mask_draw_plan(int64_t N, int64_t S, int64_t* segments, int64_t* blocks_per_segment);
int dmf_mask_draw_segments(dmf_context* ctx, uint32_t key[624], int* pos, int64_t N, int64_t S, uint64_t threshold,
                           int64_t blocks_per_segment, void** out_bits, int64_t* n_kept);
int dmf_mt_jump(uint32_t key[624], int* pos, uint64_t n_words);

#ifdef __cplusplus
}
#endif
#endif /* DEMETHIFY_HIP_H */
