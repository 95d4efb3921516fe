"""Object wrappers over the C-ABI handles: Context (one per GPU), Problem (V, D, R_trunc resident
in HBM) and Solver (the outer loop's device-resident state).

Inputs may be host numpy arrays (uploaded by the library) or PyTorch-ROCm tensors already on
the context's GPU (borrowed through ``data_ptr()``; torch is used for nothing else).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L

_contexts: dict[int, "Context"] = {}


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _host_f64(x, name):
    a = np.ascontiguousarray(x, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        # upstream lets NaN propagate silently; a device solve cannot stop on it
        raise ValueError(f"{name} holds non-finite values (use --fillna)")
    return a


def _ptr(a):
    if a is None:
        return None
    if _is_torch(a) or hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)


def pack_mask(mask) -> np.ndarray:
    """The bit-packed form of a bool N x S mask that dmf_problem_mask reads: row-major, ceil(S / 8) bytes per row,
    sample s in bit (s & 7) of byte (s >> 3); undo with ``np.unpackbits(bits, axis=1, bitorder="little")[:, :S]``."""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError(f"a mask is N x S, got shape {m.shape}")
    return np.packbits(m.astype(bool, copy=False), axis=1, bitorder="little")


def mask_threshold(fraction) -> int:
    """``x < fraction`` for a double x = k / 2**53 of numpy's legacy generator (k an integer below 2**53) as the integer
    compare ``k < T`` that dmf_mask_draw runs: T = 0 for fraction <= 0 or NaN, 2**53 for fraction >= 1, else
    ceil(fraction * 2**53) -- the product is a scaling by a power of two, hence exact."""
    import math

    f = float(fraction)
    if not f > 0.0:
        return 0
    if f >= 1.0:
        return 1 << 53
    return math.ceil(f * 9007199254740992.0)


def mt_jump(state, n_words: int):
    """The state tuple of numpy's legacy generator (``np.random.get_state()``) after ``n_words`` further 32-bit words --
    what ``np.random.bytes(4 * n_words)`` leaves behind -- by polynomial jump-ahead on the host (dmf_mt_jump): no word in
    between is generated, so 2**60 words cost what 2**10 do.  The Gaussian cache fields are passed through."""
    name, key, pos, *rest = state
    if name != "MT19937" or not 0 <= int(n_words) < 1 << 64:
        raise ValueError("mt_jump takes a legacy MT19937 state and a number of words in [0, 2**64)")
    key = np.ascontiguousarray(key, dtype=np.uint32).copy()
    pos_io = C.c_int(int(pos))
    L.check(L.load().dmf_mt_jump(key.ctypes.data_as(C.c_void_p), C.byref(pos_io), int(n_words)), "dmf_mt_jump")
    return (name, key, pos_io.value, *rest)


class Context:
    """dmf_context: a GPU, a HIP stream and the kernel-family clocks."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self._lib = L.load()
        h = C.c_void_p()
        L.check(self._lib.dmf_context_create(int(device), C.c_void_p(stream) if stream else None, C.byref(h)),
                "dmf_context_create")
        self._h = h
        self.device = int(device)
        self.generic_level = 0  # what set_generic last set: tests that change it put it back

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dmf_context_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - interpreter teardown order
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        L.check(self._lib.dmf_context_synchronize(self._h), "dmf_context_synchronize")

    def set_profiling(self, enabled, families=None):
        """Record HIP events around kernel launches: all families, or only ``families`` (indices into
        ``_lib.KERNEL_FAMILIES``) — every timed launch costs two event records on the stream."""
        mode = int(bool(enabled))
        if mode and families is not None:
            mode = sum(1 << (1 + int(f)) for f in families)
        L.check(self._lib.dmf_context_set_profiling(self._h, mode), "dmf_context_set_profiling")

    def set_generic(self, level: int):
        """Kernel selection for tests: 0 fastest (u16-count row pass + integer-MFMA Gram, falling back to level 4,
        then 3), 1 any-shape Gram-form kernels, 2 schedule-faithful one-launch-per-inner-step kernels, 3 the unfused
        MFMA row pass + one-pass Gram pair, 4 the first-generation fused FP64 row pass.  Set before creating Problems."""
        L.check(self._lib.dmf_context_set_generic(self._h, int(level)), "dmf_context_set_generic")
        self.generic_level = int(level)

    def set_x16(self, enabled: bool):
        """Whether Problems created from now on carry X16, the methylated read counts x = rint(v d) as u16, when every
        element is an exact x / d (the row pass then reads x instead of V).  On by default; off for A/B runs and tests."""
        L.check(self._lib.dmf_context_set_x16(self._h, int(bool(enabled))), "dmf_context_set_x16")

    def set_rowpass_pair(self, enabled: bool):
        """Whether Solvers created from now on run the X16 row pass two 16-row blocks per barrier cycle (65..256 samples).
        On by default; off for A/B runs and tests.  Both forms compute the same results bit for bit."""
        L.check(self._lib.dmf_context_set_rowpass_pair(self._h, int(bool(enabled))), "dmf_context_set_rowpass_pair")

    def set_rowpass_defer_c(self, enabled: bool):
        """Whether Solvers created from now on run the pair schedule with phase C deferred (193..256 samples, every count
        at most 255).  On by default; off for A/B runs and tests.  Both forms compute the same results bit for bit."""
        L.check(self._lib.dmf_context_set_rowpass_defer_c(self._h, int(bool(enabled))), "dmf_context_set_rowpass_defer_c")

    def set_rowpass_bytes(self, enabled: bool):
        """Whether Solvers created from now on run the deferred-C schedule from the problem's byte images (one byte per
        element of x and of the counts instead of two) where it has them.  On by default; off for A/B runs and tests.  Both
        forms compute the same results bit for bit."""
        L.check(self._lib.dmf_context_set_rowpass_bytes(self._h, int(bool(enabled))), "dmf_context_set_rowpass_bytes")

    def set_stop_confirmation(self, mode: int):
        """How step() decides |cf - cf_0| < tol: 0 (default) Gram-form cost, confirmed on the streaming cost where the
        Gram form's error bound reaches tol / 20; 1 always on streaming costs near the threshold; 2 Gram form only."""
        L.check(self._lib.dmf_context_set_stop_confirmation(self._h, int(mode)), "dmf_context_set_stop_confirmation")

    def reset_kernel_time(self):
        L.check(self._lib.dmf_context_reset_kernel_time(self._h), "dmf_context_reset_kernel_time")

    def kernel_time(self, family: int):
        """(total milliseconds, launches) accumulated for one kernel family while profiling."""
        ms, n = C.c_double(), C.c_int64()
        L.check(self._lib.dmf_context_kernel_time(self._h, int(family), C.byref(ms), C.byref(n)),
                "dmf_context_kernel_time")
        return ms.value, n.value

    # ---- single-function entry points -------------------------------------------------
    def project_simplex(self, X, z=1.0):
        X = np.ascontiguousarray(X, dtype=np.float64)
        out = np.empty_like(X)
        K, S = X.shape
        L.check(self._lib.dmf_project_simplex(self._h, _ptr(X), K, S, float(z), 0, _ptr(out)),
                "dmf_project_simplex")
        return out

    def nnls_normal(self, G, mom):
        """k_nnls_intercept on the caller's normal equations (dmf_nnls_normal) -> (proportions, status).  ``G``: (S, K, K)
        symmetric, or the packed (K (K + 1) / 2, S) form the kernel reads (row j (j + 1) / 2 + i for i <= j); ``mom``: the
        (2 K + 2, S) table of ``Problem.wls_moments``.  ``proportions`` (K x S) holds NaN in the columns whose status is not
        0: the library leaves them untouched.  For tests."""
        mom = np.ascontiguousarray(mom, dtype=np.float64)
        if mom.ndim != 2 or mom.shape[0] < 4 or mom.shape[0] % 2:
            raise ValueError(f"mom is (2 K + 2) x S, got shape {mom.shape}")
        K, S = mom.shape[0] // 2 - 1, mom.shape[1]
        G = np.asarray(G, dtype=np.float64)
        if G.shape == (S, K, K):
            if not np.array_equal(G, G.transpose(0, 2, 1)):
                raise ValueError("G must be symmetric")
            i, j = np.triu_indices(K)
            gb = np.empty((K * (K + 1) // 2, S), dtype=np.float64)
            gb[j * (j + 1) // 2 + i] = G[:, i, j].T
        elif G.shape == (K * (K + 1) // 2, S):
            gb = np.ascontiguousarray(G)
        else:
            raise ValueError(f"G shape {G.shape} is neither {(S, K, K)} nor {(K * (K + 1) // 2, S)}")
        out = np.full((K, S), np.nan, dtype=np.float64)
        status = np.full(S, -1, dtype=np.intc)
        L.check(self._lib.dmf_nnls_normal(self._h, _ptr(gb), _ptr(mom), K, S, _ptr(out),
                                          status.ctypes.data_as(C.POINTER(C.c_int))), "dmf_nnls_normal")
        return out, status

    def percentile_axis0(self, x, q):
        """``np.percentile(x, q, axis=0)`` (numpy's default "linear" method, bootstrap.py:51-54 / :75-78) on
        the device.  ``x``: (n replicates, ...) float64, a host array or a CUDA torch tensor; ``q``: a sequence
        of percentiles.  Returns an array / tensor of shape (len(q),) + x.shape[1:] of the same kind as ``x``."""
        return self._percentile_axis0(x, q, "dmf_percentile_axis0")

    def nanpercentile_axis0(self, x, q):
        """``np.nanpercentile(x, q, axis=0)`` on the device, the twin of ``percentile_axis0``: a column's NaNs are left
        out and its own count of numbers plans its percentiles; a column without a number gives NaN
        (dmf_nanpercentile_axis0).  Without NaNs the same bits as ``percentile_axis0``."""
        return self._percentile_axis0(x, q, "dmf_nanpercentile_axis0")

    def _percentile_axis0(self, x, q, entry):
        fn = getattr(self._lib, entry)
        qs = np.ascontiguousarray(np.atleast_1d(q), dtype=np.float64)
        if _is_torch(x) and x.is_cuda:
            import torch

            if x.dtype != torch.float64:
                raise TypeError(f"{entry[4:]} takes float64 data")
            x = x.contiguous()
            n, tail = x.shape[0], tuple(x.shape[1:])
            m = int(np.prod(tail, dtype=np.int64))
            out = torch.empty((len(qs),) + tail, dtype=torch.float64, device=x.device)
            torch.cuda.current_stream(x.device).synchronize()  # x was produced on torch's stream, not ours
            L.check(fn(self._h, _ptr(x), n, m, _ptr(qs), len(qs), L.DMF_PTR_DEVICE, _ptr(out)), entry)
            return out
        if _is_torch(x):
            x = x.numpy()
        x = np.ascontiguousarray(x, dtype=np.float64)
        n, tail = x.shape[0], tuple(x.shape[1:])
        m = int(np.prod(tail, dtype=np.int64))
        out = np.empty((len(qs),) + tail, dtype=np.float64)
        L.check(fn(self._h, _ptr(x), n, m, _ptr(qs), len(qs), 0, _ptr(out)), entry)
        return out


def get_context(device: int | None = None) -> Context:
    """Process-wide context cache; default device = LOCAL_RANK (one process per GPU) or 0."""
    if device is None:
        # DEMETHIFY_DEVICE overrides the one-process-per-GPU default (rehearsing N ranks on one GPU)
        device = int(os.environ.get("DEMETHIFY_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    ctx = _contexts.get(device)
    if ctx is None:
        ctx = _contexts[device] = Context(device)
    return ctx


def _route(route) -> int:
    try:
        return {"solver": L.DMF_ROUTE_SOLVER, "update_u": L.DMF_ROUTE_UPDATE_U}[route]
    except KeyError:
        raise ValueError(f'route must be "solver" or "update_u", got {route!r}') from None


def u_phase_describe(N, S, n_c, n_u, nd=0, level=0, n_iter2=20, flags=0, route="solver"):
    """dmf_u_phase_describe: the u phase of a shape with its launch plan -- a pure function of the key, no GPU is touched.
    None where no kernel takes the shape (DMF_ERR_UNSUPPORTED).  (2 KB: the producer k_cm_i8 prints one entry per panel of
    256 samples.)"""
    buf = C.create_string_buffer(2048)
    st = L.load().dmf_u_phase_describe(int(N), int(S), int(n_c), int(n_u), int(nd), int(level), int(n_iter2), int(flags),
                                       _route(route), buf, len(buf))
    if st == L.DMF_ERR_UNSUPPORTED:
        return None
    L.check(st, "dmf_u_phase_describe")
    return buf.value.decode()


def small_solve_supported(N, S, n_c, n_u, mode=L.DMF_MODE_PARTIAL) -> bool:
    """dmf_solve_small_supported: does ``Problem.solve_many`` take the shape?  Modes partial and unsupervised,
    1 <= n_u <= 4, n_c + n_u <= 16, S <= 64, N * S <= 2**20.  A pure function of its arguments: no GPU is touched."""
    return bool(L.load().dmf_solve_small_supported(int(N), int(S), int(n_c), int(n_u), int(mode)))


def mid_solve_supported(N, S, n_c, n_u, mode=L.DMF_MODE_PARTIAL) -> bool:
    """dmf_solve_mid_supported: does ``Problem.solve_many_mid`` take the shape?  Modes partial and unsupervised,
    1 <= n_u <= 4, n_c + n_u <= 16, S <= 64, N * S <= 2**23.  A pure function of its arguments: no GPU is touched."""
    return bool(L.load().dmf_solve_mid_supported(int(N), int(S), int(n_c), int(n_u), int(mode)))


def mid_solve_plan(N, S, rows_per_workgroup=0):
    """dmf_solve_mid_plan -> (rows, W, check_every): ``Problem.solve_many_mid`` cuts the N rows of a solve into W slabs of
    ``rows`` rows (a multiple of 256, W <= 64, the last slab may be ragged), one workgroup each, and the host reads the stop
    flags every ``check_every`` outer iterations.  ``rows_per_workgroup`` 0: the default, a function of (N, S) alone; any
    other value must be a positive multiple of 256 that gives W <= 64 (ValueError).  No GPU is touched."""
    rows, W, every = C.c_int64(), C.c_int64(), C.c_int64()
    st = L.load().dmf_solve_mid_plan(int(N), int(S), int(rows_per_workgroup), C.byref(rows), C.byref(W), C.byref(every))
    if st == L.DMF_ERR_BAD_ARG:
        raise ValueError(f"no plan for {N} x {S} with rows_per_workgroup = {rows_per_workgroup}: N and S are at least 1, "
                         f"rows_per_workgroup is 0 or a positive multiple of 256 that gives at most {L.MID_MAX_W} workgroups")
    L.check(st, "dmf_solve_mid_plan")
    return rows.value, W.value, every.value


class Problem:
    """dmf_problem: meth_frequency (N x S), counts (N x S), R_trunc (N x n_c or None)."""

    def __init__(self, ctx: Context, V, counts, Rt=None):
        self.ctx = ctx
        self._lib = ctx._lib
        flags = 0
        if _is_torch(V):
            import torch

            flags |= L.DMF_PTR_DEVICE
            for t in (V, counts) + ((Rt,) if Rt is not None else ()):
                if not (t.is_cuda and t.is_contiguous() and t.device.index == ctx.device):
                    raise ValueError("device tensors must be contiguous and on the context's GPU")
            if V.dtype != torch.float64 or (Rt is not None and Rt.dtype != torch.float64):
                raise ValueError("V and R_trunc must be float64")
            if counts.dtype == torch.float64:
                flags |= L.DMF_COUNTS_F64
            elif counts.dtype != torch.int64:
                raise ValueError("counts must be int64 or float64")
            # the tensors were produced on torch's stream, the library reads them on its own
            torch.cuda.current_stream(V.device).synchronize()
            N, S = V.shape
        else:
            V = _host_f64(V, "meth_frequency")
            counts = np.asarray(counts)
            if counts.dtype.kind in "iub":
                counts = np.ascontiguousarray(counts, dtype=np.int64)
            else:
                counts = _host_f64(counts, "counts")
                flags |= L.DMF_COUNTS_F64
            if Rt is not None:
                Rt = _host_f64(Rt, "R_trunc")
            N, S = V.shape
        if tuple(counts.shape) != (N, S):
            raise ValueError(f"counts shape {tuple(counts.shape)} != meth_frequency shape {(N, S)}")
        n_c = 0
        if Rt is not None:
            if Rt.ndim != 2 or Rt.shape[0] != N:
                raise ValueError(f"R_trunc shape {tuple(Rt.shape)} does not match {N} CpG rows")
            n_c = int(Rt.shape[1])
        self._keep = (V, counts, Rt)  # device tensors are borrowed: keep them alive
        self.N, self.S, self.n_c = int(N), int(S), n_c
        h = C.c_void_p()
        L.check(self._lib.dmf_problem_create(ctx._h, self.N, self.S, self.n_c, _ptr(V), _ptr(counts),
                                             _ptr(Rt) if n_c else None, flags, C.byref(h)),
                "dmf_problem_create")
        self._h = h

    @classmethod
    def _from_handle(cls, ctx, h, N, S, n_c):
        self = cls.__new__(cls)
        self.ctx, self._lib, self._h = ctx, ctx._lib, h
        self.N, self.S, self.n_c = N, S, n_c
        self._keep = ()
        return self

    def gather(self, idx) -> "Problem":
        """Row-resampled copy (one bootstrap replicate, bootstrap.py:28).  idx: a host integer array, or the int64 indices
        already in HBM (staging.indices_to_device: uploaded by the thread that drew them)."""
        h = C.c_void_p()
        if getattr(idx, "is_cuda", False):
            n = int(np.prod(idx.shape))
            L.check(self._lib.dmf_problem_gather_device(self.ctx._h, self._h, C.c_void_p(idx.data_ptr()), n, C.byref(h)),
                    "dmf_problem_gather_device")
            return Problem._from_handle(self.ctx, h, n, self.S, self.n_c)
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        L.check(self._lib.dmf_problem_gather(self.ctx._h, self._h, _ptr(idx), idx.size, C.byref(h)),
                "dmf_problem_gather")
        return Problem._from_handle(self.ctx, h, int(idx.size), self.S, self.n_c)

    def masked(self, train_mask) -> "Problem":
        """A copy of this problem with the elements where ``train_mask`` is False held out (their counts are 0), derived
        on the device (dmf_problem_mask): a bi-cross-validation fold (ic.py:68-75), or data with missing entries.
        ``train_mask``: a bool N x S array, or the mask as ``pack_mask`` packs it (uint8, N x ceil(S / 8)) -- a host array,
        a contiguous uint8 CUDA tensor, or a staged upload of those bytes (a DeviceArray carrying ``packed_mask``).
        ``Solver.holdout_error`` of a solver on the result takes this problem as ``full``."""
        nb = (self.S + 7) // 8
        flags = 0
        if getattr(train_mask, "is_cuda", False):
            if _is_torch(train_mask):
                import torch

                ok = (train_mask.dtype == torch.uint8 and train_mask.is_contiguous()
                      and tuple(train_mask.shape) == (self.N, nb) and train_mask.device.index == self.ctx.device)
                if ok:
                    torch.cuda.current_stream(train_mask.device).synchronize()
            else:  # staging.mask_to_device
                ok = getattr(train_mask, "packed_mask", None) == (self.N, nb) and train_mask.ctx is self.ctx
            if not ok:
                raise ValueError(f"a device mask must be the packed bits: contiguous uint8, shape {(self.N, nb)}, on the "
                                 "context's GPU")
            bits, flags = train_mask, L.DMF_PTR_DEVICE
        else:
            m = np.asarray(train_mask)
            if m.dtype == np.bool_:
                if m.shape != (self.N, self.S):
                    raise ValueError(f"mask shape {m.shape} != problem shape {(self.N, self.S)}")
                bits = pack_mask(m)
            elif m.dtype == np.uint8:
                if m.shape != (self.N, nb):
                    raise ValueError(f"packed mask shape {m.shape} != {(self.N, nb)} (ceil(S / 8) bytes per row)")
                bits = np.ascontiguousarray(m)
            else:
                raise TypeError("train_mask must be a bool N x S array or packed uint8 bits")
        h = C.c_void_p()
        L.check(self._lib.dmf_problem_mask(self.ctx._h, self._h, _ptr(bits), flags, C.byref(h)), "dmf_problem_mask")
        out = Problem._from_handle(self.ctx, h, self.N, self.S, self.n_c)
        out._keep = (self,)  # (the library copied data and bits; the parent is what holdout_error will be asked for)
        return out

    def close(self):
        if getattr(self, "_h", None):
            # (a context that is already closed took its pool, and with it this problem's buffers: the garbage collector may
            # finalise a Context before the Problems of a reference cycle that holds both)
            if getattr(self.ctx, "_h", None):
                self._lib.dmf_problem_destroy(self._h)
            self._h = None
            self._keep = ()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- single-function entry points ---------------------------------------------------
    def cost(self, u, alpha) -> float:
        """cost_f_w with R = [R_trunc | u] (deconvolution.py:15-17)."""
        alpha = np.ascontiguousarray(alpha, dtype=np.float64)
        n_u = 0
        if u is not None:
            u = np.ascontiguousarray(u, dtype=np.float64).reshape(self.N, -1)
            n_u = u.shape[1]
        if alpha.shape != (self.n_c + n_u, self.S):
            raise ValueError(f"alpha shape {alpha.shape} != {(self.n_c + n_u, self.S)}")
        out = C.c_double()
        L.check(self._lib.dmf_cost(self.ctx._h, self._h, _ptr(u) if n_u else None, n_u, _ptr(alpha), 0,
                                   C.byref(out)), "dmf_cost")
        return out.value

    def cost_describe(self, n_u: int) -> str:
        """Which kernel ``cost`` -- and a solver's direct_cost / cost_begin -- runs on this problem with n_u unknown types
        at the context's current level, e.g. "cost=k_cost_cols2<3,4,odd>" (dmf_problem_cost_describe)."""
        buf = C.create_string_buffer(128)
        L.check(self._lib.dmf_problem_cost_describe(self.ctx._h, self._h, int(n_u), buf, len(buf)),
                "dmf_problem_cost_describe")
        return buf.value.decode()

    def gram_known(self):
        """(gb_known, text): the known block of the packed Gram as problem creation left it -- ((n_c + 1)(n_c + 2) / 2, S),
        row l (l + 1) / 2 + k for k <= l over (R_trunc columns, v) -- and the route that computed it, "int_known ..." or
        "fp64 ..." (dmf_problem_gram_known).  For tests."""
        out = np.empty(((self.n_c + 1) * (self.n_c + 2) // 2, self.S), dtype=np.float64)
        buf = C.create_string_buffer(256)
        L.check(self._lib.dmf_problem_gram_known(self._h, _ptr(out), buf, len(buf)), "dmf_problem_gram_known")
        return out, buf.value.decode()

    def report(self) -> dict:
        """What the builder of this problem (create, gather, mask) left behind, as a dict: the integers ``_lib.REPORT_INTS``
        -- shapes, digit count, which integer copies and mask bits exist, the padded R_trunc copy's row width and whether
        it is R_trunc itself, n_test, d_f32_exact -- and the doubles ``_lib.REPORT_DBLS`` -- the host copy of the six
        constants, x16_dev, x16_sum (dmf_problem_report).  For tests."""
        ints = (C.c_int64 * len(L.REPORT_INTS))()
        dbls = (C.c_double * len(L.REPORT_DBLS))()
        L.check(self._lib.dmf_problem_report(self._h, ints, dbls), "dmf_problem_report")
        out = {k: int(v) for k, v in zip(L.REPORT_INTS, ints)}
        out.update({k: float(v) for k, v in zip(L.REPORT_DBLS, dbls)})
        return out

    def copy_out(self, name: str, report: dict | None = None) -> np.ndarray:
        """One device array of this problem, by its name in ``_lib.PROBLEM_ARRAYS``, in its own shape: V, D (N, S), Rt
        (N, n_c), Rtp (N, rtp_width), D16 / X16 / W16 (N16, SD) uint16, Dt8 (ND, ceil(N / 32), SD / 32, 32, 32) int8 indexed
        [plane, row block, sample block, n, k], mask_bits (N, ceil(S / 8)) uint8, consts (6,) (dmf_problem_copy_out;
        DMF_ERR_BAD_ARG for an array the problem does not have).  ``report``: this problem's ``report()``, if the caller has
        it already.  For tests."""
        r = self.report() if report is None else report
        shape, dtype = {
            "V": ((r["N"], r["S"]), np.float64), "D": ((r["N"], r["S"]), np.float64),
            "Rt": ((r["N"], r["n_c"]), np.float64), "Rtp": ((r["N"], r["rtp_width"]), np.float64),
            "D16": ((r["N16"], r["SD"]), np.uint16), "X16": ((r["N16"], r["SD"]), np.uint16),
            "W16": ((r["N16"], r["SD"]), np.uint16),
            "Dt8": ((r["ND"], (r["N"] + 31) // 32, r["SD"] // 32, 32, 32), np.int8),
            "mask_bits": ((r["N"], (r["S"] + 7) // 8), np.uint8), "consts": ((6,), np.float64),
        }[name]
        out = np.empty(shape, dtype=dtype)
        L.check(self._lib.dmf_problem_copy_out(self._h, L.PROBLEM_ARRAYS[name], _ptr(out), out.nbytes),
                "dmf_problem_copy_out")
        return out

    def has_byte_images(self) -> bool:
        """Whether this problem carries the byte images X8 / D8 of its X16 / D16 that the row pass's deferred-C schedule streams
        (X16 present, every count <= 255, 193 <= S <= 256) -- dmf_problem_has_byte_images."""
        out = C.c_int()
        L.check(self._lib.dmf_problem_has_byte_images(self._h, C.byref(out)), "dmf_problem_has_byte_images")
        return bool(out.value)

    def copy_out_image(self, name: str, report: dict | None = None) -> np.ndarray:
        """One byte image of this problem, "X8" or "D8" (``_lib.PROBLEM_BYTE_IMAGES``), as (N16 / 16, SD / 64, 1024) uint8
        indexed [16-row block, 64-sample column group, dmf_rowpass_image_offset(row, sample)] (dmf_problem_copy_out;
        DMF_ERR_BAD_ARG where the problem has none).  For tests."""
        r = self.report() if report is None else report
        out = np.empty((r["N16"] // 16, r["SD"] // 64, 1024), dtype=np.uint8)
        L.check(self._lib.dmf_problem_copy_out(self._h, L.PROBLEM_BYTE_IMAGES[name], _ptr(out), out.nbytes),
                "dmf_problem_copy_out")
        return out

    def wls_intercept(self, u=None, target="v", host_arrays=None, f64_arrays=False):
        """``wls_intercept`` (init_func.py:8-14) of every sample at once on the device (dmf_wls_intercept), with
        R_full = [R_trunc | u], the sample's counts as weights and the target meth_frequency (``target="v"``, what the
        initialisers pass) or counts * meth_frequency (``"dv"``, what the reference-based run passes).  ``u``: None, a host
        array or a float64 device array (staging.DeviceArray / CUDA tensor) of N x n_u.  Returns the K x S proportions.

        Samples the device declines (status 1: normal matrix rank-deficient to K eps, or the iteration cap) are solved by
        the host ``init_func.wls_intercept`` from ``host_arrays`` = (meth_f, counts, R_full), or a callable returning that
        tuple (it is only called when needed); without it they raise.  A sample whose counts sum to zero raises
        ZeroDivisionError, as the reference does.  ``self.wls_status`` keeps the per-sample status of the last call.
        ``f64_arrays``: take weights and target from the f64 arrays even where the problem carries X16 (DMF_WLS_F64_ARRAYS):
        the same result bit for bit with X16 on and off."""
        tg, u, n_u, flags = self._wls_args(u, target, f64_arrays)
        K = self.n_c + n_u
        out = np.zeros((K, self.S), dtype=np.float64)
        status = np.full(self.S, -1, dtype=np.intc)
        L.check(self._lib.dmf_wls_intercept(self.ctx._h, self._h, _ptr(u) if n_u else None, n_u, tg, flags, _ptr(out),
                                            status.ctypes.data_as(C.POINTER(C.c_int))), "dmf_wls_intercept")
        self.wls_status = status
        if (status == 2).any():
            raise ZeroDivisionError("Weights sum to zero, can't be normalized")
        redo = np.flatnonzero(status != 0)
        if redo.size:
            if host_arrays is None:
                raise RuntimeError(f"wls_intercept: the device did not solve samples {redo.tolist()} (rank-deficient "
                                   "profiles or iteration cap) and no host_arrays were given to solve them on the host")
            from .init_func import wls_intercept as host_wls

            meth_f, counts, R_full = host_arrays() if callable(host_arrays) else host_arrays
            for k in redo:
                x = counts[:, k:k + 1] * meth_f[:, k:k + 1] if target == "dv" else meth_f[:, k:k + 1]
                out[:, k:k + 1] = host_wls(x, counts[:, k:k + 1], R_full)
        return out

    def wls_moments(self, u=None, target="v", f64_arrays=False):
        """The first moments ``wls_intercept`` takes for the same arguments, read back (dmf_wls_moments): a (2 K + 2) x S
        array, rows 0 .. K - 1 m_k = sum_i d R_k, rows K .. 2 K - 1 r_k = sum_i d t R_k, then sw = sum_i d and st = sum_i d t,
        per sample, with t = meth_frequency (``"v"``) or counts * meth_frequency (``"dv"``).  For tests."""
        tg, u, n_u, flags = self._wls_args(u, target, f64_arrays)
        out = np.empty((2 * (self.n_c + n_u) + 2, self.S), dtype=np.float64)
        L.check(self._lib.dmf_wls_moments(self.ctx._h, self._h, _ptr(u) if n_u else None, n_u, tg, flags, _ptr(out)),
                "dmf_wls_moments")
        return out

    def _wls_args(self, u, target, f64_arrays):
        """(target code, u as the library takes it, n_u, flags) of wls_intercept / wls_moments."""
        try:
            tg = {"v": L.DMF_WLS_TARGET_V, "dv": L.DMF_WLS_TARGET_DV}[target]
        except KeyError:
            raise ValueError(f'target must be "v" or "dv", got {target!r}') from None
        flags, n_u = 0, 0
        if u is not None:
            if getattr(u, "is_cuda", False):
                from .staging import DeviceArray

                if isinstance(u, DeviceArray):
                    ok = u.ctx is self.ctx
                else:
                    ok = (_is_torch(u) and u.is_contiguous() and u.element_size() == 8 and u.is_floating_point()
                          and u.device.index == self.ctx.device)
                    if ok:
                        import torch

                        torch.cuda.current_stream(u.device).synchronize()
                if not ok:
                    raise ValueError("a device u must be a float64 staging.DeviceArray / contiguous CUDA tensor on the "
                                     "context's GPU")
                u = u.reshape(self.N, -1)
                flags = L.DMF_PTR_DEVICE
            else:
                u = _host_f64(u, "u").reshape(self.N, -1)
            n_u = int(u.shape[1])
        if f64_arrays:
            flags |= L.DMF_WLS_F64_ARRAYS
        return tg, u, n_u, flags

    def svd_gram(self, H1=None):
        """``Yres.T @ Yres`` (S x S) of Yres = max(meth_frequency - R_trunc @ H1, 1e-8) -- meth_frequency itself without
        known types -- on the device (dmf_svd_gram) -> (C, negative entries of meth_frequency, non-finite ones)."""
        if self.n_c:
            H1 = _host_f64(H1, "H1")
            if H1.shape != (self.n_c, self.S):
                raise ValueError(f"H1 shape {H1.shape} != {(self.n_c, self.S)}")
        else:
            H1 = None
        out = np.empty((self.S, self.S), dtype=np.float64)
        counts = (C.c_int64 * 2)()
        L.check(self._lib.dmf_svd_gram(self.ctx._h, self._h, _ptr(H1), 0, _ptr(out), counts), "dmf_svd_gram")
        return out, int(counts[0]), int(counts[1])

    def nndsvd(self, rank, keep_on_device=False, host_arrays=None):
        """The SVD initialiser's factors (init_func.py:17-82) on the device -> (u0, H): u0 = the N x rank unknown profiles,
        cut at 1e-11 and clipped to [0, 1] (a host array, or with ``keep_on_device`` a staging.DeviceArray for ``Solver``),
        H = the (n_c + rank) x S factor [H1; H2] before its projection onto the simplex.

        H1 is ``wls_intercept(None, "v", f64_arrays=True)``; the S x S Gram of the residual comes from dmf_svd_gram, its eigendecomposition
        from numpy.linalg.eigh here, the left factors from dmf_svd_factor / dmf_svd_finish.  ``host_arrays`` =
        (meth_f, counts, R_trunc or None), or a callable returning that tuple (called only when needed), serves the samples
        the device regression declines and the whole computation where the kernels do not take the shape, or where the
        Gram route is not the SVD route to working precision (a used eigenvalue below 1e-10 of the largest): the host route
        of init_func.  Without known types a negative entry raises the reference's ValueError."""
        from .init_func import constrained_nndsvd, nndsvd_from_eig, nndsvd_initialize

        rank = int(rank)
        if rank < 1:
            raise ValueError(f"rank must be at least 1, got {rank}")

        def host_route():
            if host_arrays is None:
                raise RuntimeError("nndsvd: the device route does not take this problem and no host_arrays were given")
            meth_f, counts, R_trunc = host_arrays() if callable(host_arrays) else host_arrays
            if self.n_c:
                W, H = constrained_nndsvd(meth_f, R_trunc, counts, rank)
                u0 = W[:, self.n_c:]
            else:
                W, H = nndsvd_initialize(meth_f, rank)
                u0 = np.clip(W, 0, 1)
            u0 = np.ascontiguousarray(u0)
            if keep_on_device:
                from .staging import to_device

                u0, = to_device((u0,), self.ctx)
            return u0, H

        if rank > self.S:
            raise ValueError(f"rank {rank} exceeds the {self.S} samples")
        # (from the f64 arrays, like the residual: u0 and H are then the same bit for bit with X16 on and off)
        H1 = self.wls_intercept(None, "v", host_arrays=host_arrays, f64_arrays=True) if self.n_c else None
        try:
            gram, negatives, _ = self.svd_gram(H1)
        except L.DemethifyHipError as e:
            if e.status != L.DMF_ERR_UNSUPPORTED:
                raise
            return host_route()
        if not self.n_c and negatives:
            raise ValueError("The input matrix contains negative elements.")
        lam, vec = np.linalg.eigh(gram)
        lam, vec = lam[::-1][:rank], np.ascontiguousarray(vec[:, ::-1][:, :rank])
        if not lam[-1] > 1e-10 * lam[0]:
            return host_route()
        sigma = np.sqrt(lam)
        try:
            u_dev, norms = self.svd_factor(H1, vec / sigma)
        except L.DemethifyHipError as e:
            if e.status != L.DMF_ERR_UNSUPPORTED:
                raise
            return host_route()
        sign, scale, H2 = nndsvd_from_eig(sigma, vec, norms)
        u0 = self.svd_finish(u_dev, sign, scale, keep_on_device)
        return u0, (np.vstack([H1, H2]) if self.n_c else H2)

    def svd_factor(self, H1, e_over_sigma):
        """``Yres @ e_over_sigma`` (N x rank; Yres as in svd_gram, e_over_sigma S x rank) left on the device, and the sums of
        max(t, 0)**2 and max(-t, 0)**2 of its columns (dmf_svd_factor) -> (staging.DeviceArray, 2 x rank array)."""
        from .staging import DeviceArray

        H1 = _host_f64(H1, "H1") if self.n_c else None
        e_over_sigma = _host_f64(e_over_sigma, "e_over_sigma")
        if e_over_sigma.ndim != 2 or e_over_sigma.shape[0] != self.S:
            raise ValueError(f"e_over_sigma shape {e_over_sigma.shape} does not match {self.S} samples")
        rank = int(e_over_sigma.shape[1])
        norms = np.empty((2, rank), dtype=np.float64)
        t = C.c_void_p()
        L.check(self._lib.dmf_svd_factor(self.ctx._h, self._h, _ptr(H1), _ptr(e_over_sigma), rank, 0, _ptr(norms),
                                         C.byref(t)), "dmf_svd_factor")
        return DeviceArray(self.ctx, t.value, (self.N, rank)), norms

    def svd_finish(self, t_dev, sign, scale, keep_on_device=False):
        """u0 from svd_factor's array, in place (dmf_svd_finish): column j becomes scale_j |t| (sign_j = 0) or
        scale_j max(sign_j t, 0), cut at 1e-11 and clipped to [0, 1] -> the array itself, or a host copy (the device array
        is then released)."""
        n, rank = t_dev.shape
        sign = np.ascontiguousarray(sign, dtype=np.float64)
        scale = np.ascontiguousarray(scale, dtype=np.float64)
        if sign.shape != (rank,) or scale.shape != (rank,):
            raise ValueError(f"sign and scale need {rank} values each")
        if keep_on_device:
            L.check(self._lib.dmf_svd_finish(self.ctx._h, _ptr(t_dev), n, rank, _ptr(sign), _ptr(scale), L.DMF_PTR_DEVICE,
                                             None), "dmf_svd_finish")
            return t_dev
        u0 = np.empty((n, rank), dtype=np.float64)
        try:
            L.check(self._lib.dmf_svd_finish(self.ctx._h, _ptr(t_dev), n, rank, _ptr(sign), _ptr(scale), 0, _ptr(u0)),
                    "dmf_svd_finish")
        finally:
            t_dev.close()
        return u0

    # the C entry points of the batch families: (plain, purity, masked)
    _BATCH_ENTRIES = {"small": ("dmf_solve_small", "dmf_solve_small_purity", "dmf_solve_small_masked"),
                      "mid": ("dmf_solve_mid", "dmf_solve_mid_purity", "dmf_solve_mid_masked")}

    def _solve_batch(self, family, u0s, alpha0s, mode, n_iter1, n_iter2, tol, tuning, idx=None, purity=None, train_masks=None):
        """The one body of ``solve_many``, ``solve_many_mid`` and their masked siblings: the checks (every ValueError before
        the library is touched), the output arrays, and the family's entry point for the variant -- masked where
        ``train_masks`` is given (``idx`` and ``purity`` are then not looked at), else purity where ``purity`` is.  ``tuning``:
        the family's integers between ``tol`` and the stream in the C argument list."""
        u0s = np.ascontiguousarray(u0s, dtype=np.float64)
        alpha0s = np.ascontiguousarray(alpha0s, dtype=np.float64)
        if u0s.ndim != 3 or u0s.shape[1] != self.N:
            raise ValueError(f"u0s is B x {self.N} x n_u, got shape {u0s.shape}")
        B, _, n_u = u0s.shape
        K = self.n_c + n_u
        if alpha0s.shape != (B, K, self.S):
            raise ValueError(f"alpha0s shape {alpha0s.shape} != {(B, K, self.S)}")
        plain, with_purity, masked = self._BATCH_ENTRIES[family]
        if train_masks is not None:
            name, per_solve, shared = masked, self._packed_train_masks(train_masks, B), ()
        else:
            if idx is not None:
                idx = np.ascontiguousarray(idx, dtype=np.int64)
                if idx.shape != (B, self.N):
                    raise ValueError(f"idx shape {idx.shape} != {(B, self.N)}")
            name, per_solve, shared = plain, idx, ()
            if purity is not None:
                purity = np.ascontiguousarray(purity, dtype=np.float64)
                if purity.shape != (self.S,):
                    raise ValueError(f"purity needs one value per sample ({self.S}), got shape {purity.shape}")
                if int(mode) != L.DMF_MODE_PARTIAL:
                    raise ValueError("a purity constraint needs the partial-reference mode (DMF_MODE_PARTIAL)")
                if self.n_c < 1:
                    raise ValueError("a purity constraint needs a reference: there is no known block to hold at that mass")
                name, shared = with_purity, (_ptr(purity),)
        out = [np.empty((B, self.N, n_u), dtype=np.float64), np.empty((B, K, self.S), dtype=np.float64),
               np.empty(B, dtype=np.float64), np.empty(B, dtype=np.int64)]  # u, alpha, cost, iters
        if train_masks is not None:
            out += [np.empty(B, dtype=np.float64), np.empty(B, dtype=np.int64)]  # holdout_sum_sq, n_test
        entry = getattr(self._lib, name)
        L.check(entry(self.ctx._h, self._h, B, _ptr(per_solve), _ptr(u0s), _ptr(alpha0s), *shared, n_u, int(mode), int(n_iter1),
                      int(n_iter2), float(tol), *(int(t) for t in tuning), 0, *(_ptr(o) for o in out)), name)
        return tuple(out)

    def solve_many(self, u0s, alpha0s, mode, n_iter1, n_iter2, tol, idx=None, iters_per_launch=0, purity=None):
        """B independent solves of this problem in one call, one workgroup per solve (dmf_solve_small) ->
        (u[B, N, n_u], alpha[B, K, S], cost[B], iters[B]).  ``u0s`` (B, N, n_u) and ``alpha0s`` (B, K, S): the starting
        points; ``idx`` (B, N) integers or None: row i of solve b is row ``idx[b, i]`` of the problem (a bootstrap
        replicate), None = the problem's own rows.  ``cost[b]`` is cost_f_w of solve b's final iterate, ``iters[b]`` its
        outer iterations.  ``iters_per_launch``: outer iterations per kernel launch, 0 = the library's default; the results
        do not depend on it.  Host arrays in, fresh host arrays out; nothing is mutated.  Shapes outside
        ``small_solve_supported`` raise (DMF_ERR_UNSUPPORTED): there is no fall-back to the per-solve path here.

        ``purity`` (S fractions, shared by the B solves; None = no constraint): the purity-constrained solve
        (dmf_solve_small_purity, ``mdwbssmf_deconv_p``) -- every sample's known block keeps mass ``purity[s]`` and its unknown
        block ``1 - purity[s]``, the alpha phase is Frank-Wolfe.  Partial mode on a problem with a reference only, and a
        vector of S values: anything else raises ValueError before any device call."""
        return self._solve_batch("small", u0s, alpha0s, mode, n_iter1, n_iter2, tol, (iters_per_launch,), idx=idx, purity=purity)

    def solve_many_mid(self, u0s, alpha0s, mode, n_iter1, n_iter2, tol, idx=None, rows_per_workgroup=0, check_every=0,
                       purity=None):
        """B independent solves of this problem in one call, several workgroups per solve (dmf_solve_mid; DESIGN.md section
        6.3) -> (u[B, N, n_u], alpha[B, K, S], cost[B], iters[B]).  Arguments, shapes, errors and results are
        ``solve_many``'s; the shapes taken are those of ``mid_solve_supported`` (N * S up to 2**23), anything else raises
        (DMF_ERR_UNSUPPORTED): there is no fall-back.  ``rows_per_workgroup``: rows per slab, 0 = the default of
        ``mid_solve_plan``; it orders the sums over rows and so may change the last bits.  ``check_every``: outer iterations
        between two reads of the stop flags, 0 = the default; the results do not depend on it.  A hold-out mask per solve:
        ``solve_many_mid_masked``.

        ``purity`` (S fractions, shared by the B solves; None = no constraint, the call as it is without the keyword): the
        purity-constrained solve (dmf_solve_mid_purity, ``mdwbssmf_deconv_p``), checked as ``solve_many`` checks it -- a vector
        of S values, partial mode, a problem with a reference, anything else raises ValueError before any device call."""
        return self._solve_batch("mid", u0s, alpha0s, mode, n_iter1, n_iter2, tol, (rows_per_workgroup, check_every), idx=idx,
                                 purity=purity)

    def solve_many_masked(self, u0s, alpha0s, train_masks, mode, n_iter1, n_iter2, tol, iters_per_launch=0):
        """B independent solves of this problem, each on its own hold-out mask, in one call (dmf_solve_small_masked: the
        folds of a bi-cross-validation, ic.py:58-89) -> (u[B, N, n_u], alpha[B, K, S], cost[B], iters[B],
        holdout_sum_sq[B], n_test[B]).  ``train_masks``: a bool array of shape (B, N, S), True = kept, or the masks as
        ``pack_mask`` packs them, uint8 of shape (B, N, ceil(S / 8)).  Solve b sees the count of an element as 0 where its
        mask is False; ``cost[b]`` is cost_f_w on those masked data, ``holdout_sum_sq[b]`` the squared error of the final
        iterate on the held-out elements of the full data and ``n_test[b]`` their number (the fold's error is their
        quotient).  Everything else is ``solve_many``'s.  Shape errors raise ValueError before any device call; a mask that
        keeps no element is refused by the library (DMF_ERR_BAD_ARG) before any solve starts."""
        return self._solve_batch("small", u0s, alpha0s, mode, n_iter1, n_iter2, tol, (iters_per_launch,), train_masks=train_masks)

    def _packed_train_masks(self, train_masks, B):
        """The train masks of B solves as the masked batch entries take them: uint8 (B, N, ceil(S / 8)) in ``pack_mask``'s
        layout, from a bool (B, N, S) array or from such bits.  Anything else raises ValueError."""
        nb = (self.S + 7) // 8
        m = np.asarray(train_masks)
        if m.dtype == np.bool_:
            if m.shape != (B, self.N, self.S):
                raise ValueError(f"train_masks shape {m.shape} != {(B, self.N, self.S)}")
            return np.packbits(m, axis=2, bitorder="little")  # (pack_mask's layout, one mask after the other)
        if m.dtype == np.uint8:
            if m.shape != (B, self.N, nb):
                raise ValueError(f"packed train_masks shape {m.shape} != {(B, self.N, nb)} (ceil(S / 8) bytes per row)")
            return np.ascontiguousarray(m)
        raise ValueError("train_masks must be a bool (B, N, S) array or packed uint8 bits (B, N, ceil(S / 8))")

    def solve_many_mid_masked(self, u0s, alpha0s, train_masks, mode, n_iter1, n_iter2, tol, rows_per_workgroup=0,
                              check_every=0):
        """B independent solves of this problem, each on its own hold-out mask, several workgroups per solve
        (dmf_solve_mid_masked) -> (u[B, N, n_u], alpha[B, K, S], cost[B], iters[B],
        holdout_sum_sq[B], n_test[B]).  ``train_masks``, what a solve sees of a held-out element and the results are
        ``solve_many_masked``'s; ``rows_per_workgroup``, ``check_every`` and the shapes taken are ``solve_many_mid``'s.  No
        ``idx`` and no ``purity``.  Shape errors raise ValueError before any device call; a mask that keeps no element is
        refused by the library (DMF_ERR_BAD_ARG) before any solve starts."""
        return self._solve_batch("mid", u0s, alpha0s, mode, n_iter1, n_iter2, tol, (rows_per_workgroup, check_every),
                                 train_masks=train_masks)

    def update_u(self, u, u_prev, alpha, n_iter2, a1, l_w_prev, l_w, mode=L.DMF_MODE_PARTIAL):
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(self.N, -1)
        u_prev = np.ascontiguousarray(u_prev, dtype=np.float64).reshape(u.shape)
        alpha = np.ascontiguousarray(alpha, dtype=np.float64)
        n_u = u.shape[1]
        if alpha.shape != (self.n_c + n_u, self.S):
            raise ValueError(f"alpha shape {alpha.shape} != {(self.n_c + n_u, self.S)}")
        sc = (C.c_double * 3)(float(a1), float(l_w_prev), float(l_w))
        out_u, out_up = np.empty_like(u), np.empty_like(u)
        L.check(self._lib.dmf_update_u(self.ctx._h, self._h, _ptr(u), _ptr(u_prev), _ptr(alpha), n_u,
                                       int(n_iter2), int(mode), 0, sc, _ptr(out_u), _ptr(out_up)),
                "dmf_update_u")
        return out_u, out_up, sc[0], sc[1]

    def update_alpha(self, u, alpha, alpha_prev, n_iter2, a2, l_h_prev, l_h):
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(self.N, -1)
        alpha = np.ascontiguousarray(alpha, dtype=np.float64)
        alpha_prev = np.ascontiguousarray(alpha_prev, dtype=np.float64)
        n_u = u.shape[1]
        if alpha.shape != (self.n_c + n_u, self.S) or alpha_prev.shape != alpha.shape:
            raise ValueError(f"alpha shape {alpha.shape} != {(self.n_c + n_u, self.S)}")
        sc = (C.c_double * 3)(float(a2), float(l_h_prev), float(l_h))
        out_a, out_ap = np.empty_like(alpha), np.empty_like(alpha)
        L.check(self._lib.dmf_update_alpha(self.ctx._h, self._h, _ptr(u), n_u, _ptr(alpha), _ptr(alpha_prev),
                                           int(n_iter2), 0, sc, _ptr(out_a), _ptr(out_ap)),
                "dmf_update_alpha")
        return out_a, out_ap, sc[0], sc[1]


class Solver:
    """dmf_solver: state init (deconvolution.py:192-204) + stepping of the outer loop."""

    def __init__(self, problem: Problem, u0, alpha0, mode=L.DMF_MODE_PARTIAL):
        """u0 (N x n_u) and alpha0 (K x S): host arrays, or BOTH float64 device arrays on the context's GPU
        (staging.to_device: the initialisation of the next restart, uploaded while this one iterates; or CUDA tensors)."""
        self.problem = problem
        self._lib = problem._lib
        flags = 0
        if getattr(u0, "is_cuda", False) or getattr(alpha0, "is_cuda", False):
            from .staging import DeviceArray

            for t in (u0, alpha0):
                if isinstance(t, DeviceArray):
                    ok = t.ctx is problem.ctx
                else:
                    ok = (_is_torch(t) and t.is_cuda and t.is_contiguous() and t.element_size() == 8
                          and t.is_floating_point() and t.device.index == problem.ctx.device)
                if not ok:
                    raise ValueError("u0 and alpha0 must both be host arrays, or both be float64 device arrays "
                                     "(staging.DeviceArray / contiguous CUDA tensors) on the context's GPU")
            u0 = u0.reshape(problem.N, -1)
            flags = L.DMF_PTR_DEVICE
            if getattr(alpha0, "in_unit_range", None) is True:  # (checked on the host by the thread that uploaded it)
                flags |= L.DMF_INIT_IN_UNIT_RANGE
        else:
            u0 = np.ascontiguousarray(u0, dtype=np.float64).reshape(problem.N, -1)
            alpha0 = np.ascontiguousarray(alpha0, dtype=np.float64)
        self.n_u = int(u0.shape[1])
        self.K = problem.n_c + self.n_u
        if tuple(alpha0.shape) != (self.K, problem.S):
            raise ValueError(f"alpha shape {tuple(alpha0.shape)} != {(self.K, problem.S)}")
        h = C.c_void_p()
        L.check(self._lib.dmf_solver_create(problem.ctx._h, problem._h, _ptr(u0), _ptr(alpha0), self.n_u,
                                            int(mode), flags, C.byref(h)), "dmf_solver_create")
        self._h = h

    def set_purity(self, purity):
        """Switch the alpha phase to the purity-constrained Frank-Wolfe update (deconvolution.py:280-302):
        per-sample mass of the known block, S values in [0, 1]."""
        purity = np.ascontiguousarray(purity, dtype=np.float64).ravel()
        if purity.shape != (self.problem.S,):
            raise ValueError(f"purity needs one value per sample ({self.problem.S}), got {purity.shape}")
        L.check(self._lib.dmf_solver_set_purity(self._h, _ptr(purity), 0), "dmf_solver_set_purity")

    def step(self, n_outer: int, n_iter2: int, tol: float):
        """Run up to n_outer outer iterations; returns (total iterations so far, converged)."""
        it, conv = C.c_int64(), C.c_int()
        L.check(self._lib.dmf_solver_step(self._h, int(n_outer), int(n_iter2), float(tol), C.byref(it),
                                          C.byref(conv)), "dmf_solver_step")
        return it.value, bool(conv.value)

    def get(self):
        """(u, alpha, cost, iterations) of the current iterate, as fresh host arrays."""
        u = np.empty((self.problem.N, self.n_u), dtype=np.float64)
        alpha = np.empty((self.K, self.problem.S), dtype=np.float64)
        cost, it = C.c_double(), C.c_int64()
        L.check(self._lib.dmf_solver_get(self._h, 0, _ptr(u), _ptr(alpha), C.byref(cost), C.byref(it)),
                "dmf_solver_get")
        return u, alpha, cost.value, it.value

    def direct_cost(self) -> float:
        """cost_f_w of the current iterate by the streaming formula (deconvolution.py:15-17), computed where the
        iterate lives: what demethify.py:169,199 and ic.py:206 recompute after a solve."""
        out = C.c_double()
        L.check(self._lib.dmf_solver_cost(self._h, C.byref(out)), "dmf_solver_cost")
        return out.value

    def holdout_error(self, full: Problem):
        """(sum of squares, n_test) of this solver's masked problem (``full.masked(...)``): the sum over the held-out
        elements of (meth_frequency - [R_trunc | u] @ alpha)**2 with ``full``'s frequencies -- ic.py:80 before its
        division by the number of held-out elements -- computed where the iterate lives (dmf_solver_holdout_error)."""
        ss, n = C.c_double(), C.c_int64()
        L.check(self._lib.dmf_solver_holdout_error(self._h, full._h, C.byref(ss), C.byref(n)), "dmf_solver_holdout_error")
        return ss.value, n.value

    def cost_begin(self):
        """Enqueue direct_cost() without waiting for it (dmf_solver_cost_begin): set up the next solver, then cost_end()."""
        L.check(self._lib.dmf_solver_cost_begin(self._h), "dmf_solver_cost_begin")

    def cost_end(self) -> float:
        out = C.c_double()
        L.check(self._lib.dmf_solver_cost_end(self._h, C.byref(out)), "dmf_solver_cost_end")
        return out.value

    def describe(self, n_iter2: int = 20) -> str:
        """Which kernels a step with n_iter2 inner iterations launches (dmf_solver_describe)."""
        buf = C.create_string_buffer(512)
        L.check(self._lib.dmf_solver_describe(self._h, int(n_iter2), buf, len(buf)), "dmf_solver_describe")
        return buf.value.decode()

    def u_phase_describe(self, n_iter2: int = 20, route="solver") -> str:
        """What the u phase of this solver launches, with its launch plan (dmf_solver_u_phase_describe).  ``route``:
        "solver" (an outer iteration of step()) or "update_u" (the stand-alone u phase of Problem.update_u)."""
        buf = C.create_string_buffer(2048)
        L.check(self._lib.dmf_solver_u_phase_describe(self._h, int(n_iter2), _route(route), buf, len(buf)),
                "dmf_solver_u_phase_describe")
        return buf.value.decode()

    def gram(self, kind="integer"):
        """(gb, text): the packed Gram ((K + 1)(K + 2) / 2, S) for the solver's CURRENT u, computed now by the kernels a step
        calls, and what ran (dmf_solver_gram).  ``kind``: "integer" (k_bu_cols + k_gram_i8_w8 + reduce + finish; u must lie
        in [0, 1]; DMF_ERR_UNSUPPORTED where the integer Gram does not take the problem) or "fp64" (k_gram_u / k_gram_mfma /
        k_gram, as the solver's selection names) -- or "last": nothing is computed, the solver's own packed Gram as the last
        outer iteration of step() left it, with the text of what wrote it.  For tests: the iterate and a later step() are
        unaffected."""
        try:
            k = {"integer": L.DMF_GRAM_INTEGER, "fp64": L.DMF_GRAM_FP64, "last": L.DMF_GRAM_LAST}[kind]
        except KeyError:
            raise ValueError(f'kind must be "integer", "fp64" or "last", got {kind!r}') from None
        out = np.empty(((self.K + 1) * (self.K + 2) // 2, self.problem.S), dtype=np.float64)
        buf = C.create_string_buffer(256)
        L.check(self._lib.dmf_solver_gram(self._h, k, _ptr(out), buf, len(buf)), "dmf_solver_gram")
        return out, buf.value.decode()

    def row_moments(self):
        """(cm, text): the per-row moments of the split u phase, (N, n_u + n_u (n_u + 1) / 2) doubles -- c_i, then M_i in
        packed pair order p = l (l + 1) / 2 + j, j <= l -- for the solver's CURRENT alpha, computed now by the producer that
        the split form of its stand-alone u phase launches (k_cm_i8, or k_u_phase_mfma in split mode), and that producer's
        launch plan (dmf_solver_row_moments).  DMF_ERR_UNSUPPORTED where that u phase has no split form; DMF_ERR_BAD_ARG on
        a solver that has stopped (its producers do nothing).  For tests: the iterate and a later step() are unaffected."""
        n_u = self.n_u
        out = np.empty((self.problem.N, n_u + n_u * (n_u + 1) // 2), dtype=np.float64)
        buf = C.create_string_buffer(2048)
        L.check(self._lib.dmf_solver_row_moments(self._h, _ptr(out), buf, len(buf)), "dmf_solver_row_moments")
        return out, buf.value.decode()

    def momentum_state(self, arrays=True):
        """The momentum state of the outer loop as it stands on the device (dmf_solver_momentum_state): a dict of the
        scalars ``_lib.MOMENTUM_SCALARS`` -- a1, a2, l_w, l_w_prev, l_h, l_h_prev, dsq, rt_norm2, u_norm2, cf, cf_prev as
        floats, iters, done, arrive, mom_n, mom_i as ints -- and, with ``arrays``, "alpha_prev" (K x S) and "u_prev"
        (N x n_u) as fresh host arrays.  For tests: read-only, the iterate and a later step() are unaffected."""
        sc = (C.c_double * len(L.MOMENTUM_SCALARS))()
        alpha_prev = np.empty((self.K, self.problem.S), dtype=np.float64) if arrays else None
        u_prev = np.empty((self.problem.N, self.n_u), dtype=np.float64) if arrays else None
        L.check(self._lib.dmf_solver_momentum_state(self._h, sc, _ptr(alpha_prev), _ptr(u_prev)),
                "dmf_solver_momentum_state")
        out = {name: (int(v) if i >= 11 else float(v)) for i, (name, v) in enumerate(zip(L.MOMENTUM_SCALARS, sc))}
        if arrays:
            out["alpha_prev"], out["u_prev"] = alpha_prev, u_prev
        return out

    def stop_info(self):
        """How the stop tests of this solver's step() calls were decided (dmf_solver_stop_info): a dict with
        confirm_stops (streaming-cost confirmation active for the last step() call), n_confirmed, n_unconfirmed and
        last_stream_cost (NaN: none taken)."""
        on, nc, nu, cs = C.c_int(), C.c_int64(), C.c_int64(), C.c_double()
        L.check(self._lib.dmf_solver_stop_info(self._h, C.byref(on), C.byref(nc), C.byref(nu), C.byref(cs)),
                "dmf_solver_stop_info")
        return {"confirm_stops": bool(on.value), "n_confirmed": nc.value, "n_unconfirmed": nu.value,
                "last_stream_cost": cs.value}

    def rowpass_launches(self):
        """(k_rowpass_v2 launches so far, how many of them ran the pair schedule) -- dmf_solver_rowpass_launches."""
        total, paired = C.c_int64(), C.c_int64()
        L.check(self._lib.dmf_solver_rowpass_launches(self._h, C.byref(total), C.byref(paired)),
                "dmf_solver_rowpass_launches")
        return total.value, paired.value

    def rowpass_byte_launches(self):
        """How many of the deferred-C launches so far read the problem's byte images -- dmf_solver_rowpass_byte_launches."""
        n = C.c_int64()
        L.check(self._lib.dmf_solver_rowpass_byte_launches(self._h, C.byref(n)), "dmf_solver_rowpass_byte_launches")
        return n.value

    def rowpass_schedule_counts(self):
        """(k_rowpass_v2 launches so far, of them on the pair schedule, of those with phase C deferred) --
        dmf_solver_rowpass_schedule_counts."""
        total, paired, deferred = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(self._lib.dmf_solver_rowpass_schedule_counts(self._h, C.byref(total), C.byref(paired), C.byref(deferred)),
                "dmf_solver_rowpass_schedule_counts")
        return total.value, paired.value, deferred.value

    def get_alpha(self):
        """The current proportions (K x S) as a fresh host array; u stays on the device."""
        alpha = np.empty((self.K, self.problem.S), dtype=np.float64)
        L.check(self._lib.dmf_solver_get(self._h, 0, None, _ptr(alpha), None, None), "dmf_solver_get")
        return alpha

    def _on_device(self, t, floating):
        """Is ``t`` a staging.DeviceArray of this context, or a contiguous float64 (``floating``) / int64 CUDA tensor on its
        GPU?  (A tensor was produced on torch's stream and is read on ours: that stream is waited for.)"""
        from .staging import DeviceArray

        ctx = self.problem.ctx
        if isinstance(t, DeviceArray):
            return t.ctx is ctx
        ok = (_is_torch(t) and t.is_cuda and t.is_contiguous() and t.element_size() == 8
              and t.is_floating_point() == floating and t.device.index == ctx.device)
        if ok:
            import torch

            ok = floating or t.dtype == torch.int64
        if ok:
            torch.cuda.current_stream(t.device).synchronize()
        return ok

    def match_components(self, anchor, idx=None):
        """P (n_u x n_u host array), P[a, b] = sum_j u[j, a] * anchor[idx[j], b]: the inner products of this solver's profile
        columns with the anchor's, computed where both live (dmf_solver_match_components).  ``anchor``: the n_rows x n_u
        profiles the components are named after, a staging.DeviceArray or a contiguous float64 CUDA tensor on the context's
        GPU; ``idx``: the int64 row indices this solver's problem was gathered with, as staging.indices_to_device returns
        them (or an int64 CUDA tensor); None = the identity (the anchor then has this problem's N rows).  An index outside
        the anchor's rows raises (DMF_ERR_BAD_ARG).  ``bootstrap.match_components(P)`` turns P into the assignment."""
        on_device = self._on_device
        if not on_device(anchor, True):
            raise ValueError("anchor must be a float64 staging.DeviceArray / contiguous CUDA tensor on the context's GPU")
        n_el = int(np.prod(tuple(anchor.shape)))
        if n_el == 0 or n_el % self.n_u:
            raise ValueError(f"anchor shape {tuple(anchor.shape)} does not hold rows of {self.n_u} profiles")
        n_rows = n_el // self.n_u
        if idx is not None:
            if not on_device(idx, False):
                raise ValueError("idx must be the int64 row indices in HBM (staging.indices_to_device) on the context's GPU")
            if int(np.prod(tuple(idx.shape))) != self.problem.N:
                raise ValueError(f"idx holds {int(np.prod(tuple(idx.shape)))} indices, the problem has {self.problem.N} rows")
        P = np.empty((self.n_u, self.n_u), dtype=np.float64)
        L.check(self._lib.dmf_solver_match_components(self._h, _ptr(anchor), n_rows, _ptr(idx), _ptr(P)),
                "dmf_solver_match_components")
        return P

    def copy_u_to(self, tensor, columns=None):
        """Copy the current profile estimate u (N x n_u, C order) into a float64 CUDA torch tensor of N * n_u elements
        on the context's GPU (device to device): the bootstrap keeps its replicate stack in HBM.  ``columns``: a permutation
        of 0 .. n_u - 1; the tensor then receives ``u[:, columns]`` (dmf_solver_get_u_permuted)."""
        if not (_is_torch(tensor) and tensor.is_cuda and tensor.is_contiguous() and tensor.numel() == self.problem.N * self.n_u
                and tensor.element_size() == 8 and tensor.device.index == self.problem.ctx.device):
            raise ValueError("copy_u_to needs a contiguous float64 CUDA tensor of N * n_u elements on the context's GPU")
        if columns is not None:
            cols = np.ascontiguousarray(columns, dtype=np.int32).ravel()
            if cols.size != self.n_u or not np.array_equal(np.sort(cols), np.arange(self.n_u)):
                raise ValueError(f"columns must be a permutation of 0..{self.n_u - 1}, got {list(np.ravel(columns))}")
            L.check(self._lib.dmf_solver_get_u_permuted(self._h, cols.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(tensor)),
                    "dmf_solver_get_u_permuted")
            return
        L.check(self._lib.dmf_solver_get(self._h, L.DMF_PTR_DEVICE, _ptr(tensor), None, None, None), "dmf_solver_get")

    def copy_u_by_cpg(self, tensor, idx, n_rows, columns=None):
        """The current profile estimate with its rows put back by CpG (dmf_solver_get_u_by_row): ``idx`` holds the int64 row
        indices this solver's problem was gathered with (staging.indices_to_device, or an int64 CUDA tensor), so row j of u
        is CpG ``idx[j]`` of ``n_rows``; ``tensor``, a contiguous float64 CUDA tensor of n_rows * n_u elements on the
        context's GPU, receives in row c the row of u at the lowest position that drew CpG c -- ``u[np.unique(idx,
        return_index=True)[1]]`` -- and NaN where c was not drawn.  ``columns`` as in ``copy_u_to``.  A pure gather: the
        copied values keep their bits.  An index outside 0 .. n_rows - 1 raises (DMF_ERR_BAD_ARG), the tensor untouched."""
        n_rows = int(n_rows)
        if not (_is_torch(tensor) and tensor.is_cuda and tensor.is_contiguous() and tensor.numel() == n_rows * self.n_u
                and n_rows >= 1 and tensor.element_size() == 8 and tensor.is_floating_point()
                and tensor.device.index == self.problem.ctx.device):
            raise ValueError("copy_u_by_cpg needs a contiguous float64 CUDA tensor of n_rows * n_u elements on the context's GPU")
        if not self._on_device(idx, False):
            raise ValueError("idx must be the int64 row indices in HBM (staging.indices_to_device) on the context's GPU")
        if int(np.prod(tuple(idx.shape))) != self.problem.N:
            raise ValueError(f"idx holds {int(np.prod(tuple(idx.shape)))} indices, the problem has {self.problem.N} rows")
        cols = None
        if columns is not None:
            cols = np.ascontiguousarray(columns, dtype=np.int32).ravel()
            if cols.size != self.n_u or not np.array_equal(np.sort(cols), np.arange(self.n_u)):
                raise ValueError(f"columns must be a permutation of 0..{self.n_u - 1}, got {list(np.ravel(columns))}")
            cols = cols.ctypes.data_as(C.POINTER(C.c_int32))
        L.check(self._lib.dmf_solver_get_u_by_row(self._h, _ptr(idx), n_rows, cols, _ptr(tensor)), "dmf_solver_get_u_by_row")

    def get_cost(self):
        """(cost, iterations) of the current iterate without copying u / alpha back."""
        cost, it = C.c_double(), C.c_int64()
        L.check(self._lib.dmf_solver_get(self._h, 0, None, None, C.byref(cost), C.byref(it)), "dmf_solver_get")
        return cost.value, it.value

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dmf_solver_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
