"""Model selection: how many unknown cell types?  Host-side mirror of demethify/ic.py.

The information criteria are kept exactly as coded upstream (ic.py:11-22), including the BIC
expression that is not the textbook one.  The sweep over candidate n_u (ic.py:169-218, hard-coded
1..25 upstream) is embarrassingly parallel: with torch.distributed initialised the candidates are
dealt to the ranks longest-first and only the per-candidate scores and the winner's factors are
exchanged.  CCC and BCV sweeps run on one rank from one resident upload; a bi-cross-validation fold
(ic.py:58-89) is derived from it on the device (Problem.masked) and its hold-out error taken there
(Solver.holdout_error); from DEVICE_MASK_MIN_ELEMENTS elements on the mask itself is drawn there too (staging.draw_mask: numpy's
stream continued on the GPU, bit for bit), for the initialisers that do not read the masked data.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L
from . import shard
from . import init_func
from .batch import family, solve_chunked
from .deconvolution import _init_unsupervised, cost_f_w, init_BSSMF_md, solve_problem
from .device import Problem, Solver, get_context
from .staging import Prefetcher
from .init_func import wls_intercept

__all__ = ["compute_bic", "compute_aic", "compute_consensus_matrix", "compute_ccc", "run_deconvolution",
           "bicross_validation", "evaluate_best_ic", "batched_ic_ineligible", "SMALL_BATCH_IC_MAX_ELEMENTS",
           "MID_BATCH_IC_MIN_ELEMENTS", "MID_BATCH_IC_MAX_ELEMENTS", "MID_BATCH_IC_CRITERIA"]


def _n_free(n_u, n_cpg, n_ct, n_samples):
    return n_u * n_cpg + (n_ct + n_u - 1) * n_samples


def compute_bic(cost, n_u, n_cpg, n_ct, n_samples):
    """ic.py:11-15, as coded."""
    l = n_samples * n_cpg
    k = _n_free(n_u, n_cpg, n_ct, n_samples)
    return 2 * np.log(cost) * k * np.log(l) + (k * np.log(l) * (k + 1)) / (l - k - 1)


def compute_aic(cost, n_u, n_cpg, n_ct, n_samples):
    """ic.py:18-22."""
    l = n_samples * n_cpg
    k = _n_free(n_u, n_cpg, n_ct, n_samples)
    return l * np.log(cost / l) + 2 * k + (2 * k * (k + 1)) / (l - k - 1)


def compute_consensus_matrix(alpha_runs):
    """ic.py:24-37: fraction of runs in which two samples share their dominant cell type."""
    labels = np.stack([np.argmax(a, axis=0) for a in alpha_runs])  # (runs, samples)
    same = labels[:, :, None] == labels[:, None, :]
    return same.sum(axis=0) / float(len(alpha_runs))


def compute_ccc(alpha_runs):
    """ic.py:40-45: Brunet's cophenetic correlation coefficient of the consensus matrix."""
    from scipy.cluster.hierarchy import cophenet, linkage
    from scipy.spatial.distance import pdist

    distances = pdist(compute_consensus_matrix(alpha_runs), metric="euclidean")
    ccc, _ = cophenet(linkage(distances, method="average"), distances)
    return ccc


def _init_on(problem, meth_f, counts, ref, n_u, init_option, seed):
    """(u0, alpha0) of one candidate.  ``problem``: the resident upload of (meth_f, counts, ref), which the "SVD"
    initialiser runs on above its gate -- on the calling thread, which must then be the one that drives the context."""
    n_ct = ref.shape[1] if ref is not None else 0
    on_device = problem if (init_option == "SVD" and problem is not None
                            and init_func.device_svd(meth_f.shape[0], meth_f.shape[1], n_ct, n_u)) else None
    if ref is not None:
        u0, _, a0 = init_BSSMF_md(init_option, meth_f, counts, ref, n_u, seed=seed, rb_alg=wls_intercept, _stack=False,
                                  problem=on_device, _svd_host=on_device is None)
    else:
        u0, a0 = _init_unsupervised(init_option, meth_f, n_u, seed, problem=on_device, _svd_host=on_device is None)
    return u0, a0


def _solve(problem, meth_f, counts, ref, n_u, init_option, seed, iter1, iter2, tol):
    u0, a0 = _init_on(problem, meth_f, counts, ref, n_u, init_option, seed)
    mode = L.DMF_MODE_PARTIAL if ref is not None else L.DMF_MODE_UNSUPERVISED
    return solve_problem(problem, u0, a0, mode, iter1, iter2, tol)


def run_deconvolution(meth_f, counts, ref, n_u, init_option, seed, iter1, iter2, tol, problem=None):
    """ic.py:47-55 -> (u, R, alpha).  ``problem`` lets a sweep reuse one device-resident upload."""
    own = problem is None
    if own:
        problem = Problem(get_context(), meth_f, counts, ref)
    try:
        u, alpha = _solve(problem, meth_f, counts, ref, n_u, init_option, seed, iter1, iter2, tol)
    finally:
        if own:
            problem.close()
    R = np.hstack((ref, u.reshape(-1, n_u))) if ref is not None else u
    return u, R, alpha


# The number of elements N x S from which a fold's mask is drawn on the device (staging.draw_mask) instead of on the host:
# the smallest measured size from which the device leg is the faster one at every larger measured size.  Measured
# (profiles/r14_mask_draw_segments.txt, the segmented draw against the host leg: 350 x 10, 1e4 x 64, 1e5 x 64, 1e6 x 256) the
# host is the faster one at 350 x 10 alone, where the plan is one workgroup, and the device from 1e4 x 64 on.
DEVICE_MASK_MIN_ELEMENTS = 640_000


def _bcv_draw_fold(meth_f, counts, ref, n_u, init_option, seed, fraction, stage=None, draw=None):
    """The host half of one bi-cross-validation fold, in the reference's draw order (ic.py:68-75): the train mask from
    numpy's global generator, then the initialiser -- which reseeds -- on the masked data.  Returns None for a fold the
    reference skips (empty train or test set: nothing further is drawn), else (train_mask, u0, alpha0, staged) with
    ``staged = stage(train_mask)``: the device driver packs and uploads the mask here, on the drawing thread.

    ``draw(shape, fraction) -> (packed bits, number of ones)``, when one is offered, makes the same mask from the same
    generator and leaves the generator where ``rand`` would have: it is used from DEVICE_MASK_MIN_ELEMENTS elements on when
    the initialiser does not read the data ("uniform_" and "beta", and whatever option the initialisers silently replace
    by "uniform_" because n_u exceeds the samples); the fold is then (None, u0, alpha0, packed bits)."""
    shapes_only = init_option in ("uniform_", "beta") or n_u > meth_f.shape[1]
    if draw is not None and shapes_only and meth_f.size >= DEVICE_MASK_MIN_ELEMENTS:
        bits, n_train = draw(meth_f.shape, fraction)
        if n_train == meth_f.size or n_train == 0:
            if hasattr(bits, "close"):
                bits.close()
            return None
        try:
            u0, a0 = _init_on(None, meth_f, counts, ref, n_u, init_option, seed)
        except BaseException:
            if hasattr(bits, "close"):
                bits.close()
            raise
        return None, u0, a0, bits
    train_mask = np.random.rand(*meth_f.shape) < fraction
    n_train = int(np.sum(train_mask))
    if n_train == train_mask.size or n_train == 0:
        return None
    if init_option in ("uniform", "SVD"):
        # the initialisers in scope that read the data (rb_alg on every sample column; the SVD of the residual): they see
        # the masked arrays, and "SVD" stays on the host route whatever the size (a masked problem never takes the device
        # regression or the device Gram: DESIGN section 7a / 7b)
        init_f, init_c = meth_f * train_mask, counts * train_mask
    else:
        init_f, init_c = meth_f, counts  # (uniform_ / beta take the shapes only)
    u0, a0 = _init_on(None, init_f, init_c, ref, n_u, init_option, seed)
    return train_mask, u0, a0, stage(train_mask) if stage is not None else None


class _DeviceFolds:
    """The device half of a fold: the masked problem derived from the resident one (Problem.masked), the solve, and the
    hold-out error where the iterate lives; (u, alpha) leave the device only for a fold that beats ``best``."""

    def __init__(self, problem, unsupervised, iter1, iter2, tol):
        self.problem = problem
        self.mode = L.DMF_MODE_UNSUPERVISED if unsupervised else L.DMF_MODE_PARTIAL
        self.steps = (iter1, iter2, tol)

    def stage(self, train_mask):
        from .device import pack_mask
        from .staging import mask_to_device

        return mask_to_device(pack_mask(train_mask), self.problem.ctx)

    def draw(self, shape, fraction):
        from .staging import draw_mask

        return draw_mask(shape, fraction, self.problem.ctx)

    def __call__(self, fold, best):
        _, u0, a0, bits = fold
        try:
            with self.problem.masked(bits) as fold_problem, Solver(fold_problem, u0, a0, self.mode) as s:
                s.step(*self.steps)
                sum_sq, n_test = s.holdout_error(self.problem)
                test_error = sum_sq / n_test
                factors = None
                if test_error < best:
                    u, alpha, _, _ = s.get()
                    factors = (u, alpha)
        finally:
            bits.close()
        return test_error, factors


# The number of elements N x S up to which the command line (DEMETHIFY_BATCH=1) sends an --ic sweep through
# evaluate_best_ic(batched=True): the largest measured size at which the batched leg wins for BCV and CCC there and at every
# smaller measured size.  Measured (tools/small_ic_bench.py, profiles/small_batch_ic_bench.txt; candidates n_u = 1..4, medians
# of five, per-solve against batched): 350 x 10 with 20 folds of BCV 646 ms against 213 ms and with 20 restarts of CCC 441 ms
# against 210 ms, 1 000 x 16 BCV 515 ms against 305 ms and CCC 358 ms against 270 ms -- and 10 000 x 64 with 5 folds of BCV
# 0.22 s against 12.9 s: there one workgroup per fold loses, as for the restarts (bootstrap.SMALL_BATCH_MAX_ELEMENTS), so the
# gate sits at 1 000 x 16.
SMALL_BATCH_IC_MAX_ELEMENTS = 16000
# The criteria the command line sends through the batch below that gate.  AIC / BIC are not among them: their one solve
# per candidate as a batch of one is ONE workgroup on one CU, measured slower on the 350 x 10 example (22 ms against 125 ms for
# the four candidates), so the command line leaves them on the per-solve path; evaluate_best_ic(batched=True) takes them.
SMALL_BATCH_IC_CRITERIA = ("CCC", "BCV")


# The range of N x S in which the command line (DEMETHIFY_BATCH_MID_IC=1) sends an --ic sweep through
# evaluate_best_ic(batched=True, batch_kernel="mid"), and the criteria it sends: by the rule of bootstrap.MID_BATCH_*, the
# contiguous range of MEASURED sizes at which the mid-size leg beats both the per-solve leg and the one-launch batch in every
# gated criterion, and the criteria that won (tools/mid_ic_bench.py, profiles/mid_batch_ic_bench.txt).  MIN > MAX is a closed
# gate.  Measured (candidates n_u = 1..4, at most 200 outer iterations, medians of five; per-solve on the commit before /
# one-launch batch / mid-size batch): 1 000 x 16 (6 + 2) BCV with 20 folds 515 / 305 / 196 ms, CCC with 20 restarts
# 355 / 271 / 181 ms, AIC 21 / 220 / 144 ms; 4 000 x 16 (6 + 2) BCV 590 / 864 / 255 ms, CCC 469 / 789 / 239 ms, AIC
# 25 / 648 / 178 ms; 10 000 x 64 (12 + 4) BCV with 5 folds 221 / 12 770 / 818 ms, CCC 672 / 10 756 / 1 097 ms, AIC
# 36 / 9 247 / 647 ms; 32 768 x 64 (12 + 4) BCV 331 / - / 1 466 ms, CCC 996 / - / 2 253 ms, AIC 48 / - / 1 054 ms.  The mid-size
# leg wins BCV and CCC at 16 000 and 64 000 elements and loses both from 640 000 on; AIC (one solve per candidate: a batch of
# one) loses at every size and stays out, so BIC, the same single solve, stays out with it.
MID_BATCH_IC_MIN_ELEMENTS, MID_BATCH_IC_MAX_ELEMENTS = 16000, 64000
MID_BATCH_IC_CRITERIA = ("CCC", "BCV")


def batched_ic_ineligible(n_u, n_rows, n_samples, n_ct, mode, kernel="small"):
    """Why a candidate ``n_u`` of a model-selection sweep cannot go through ``Problem.solve_many`` /
    ``Problem.solve_many_masked``, as a sentence, or None when it can.  The batched kernel's envelope only (nothing else
    stands between a sweep and the batch: every initialiser runs on host arrays before the call).  ``kernel``: "small" (the
    default) or "mid" -- ``Problem.solve_many_mid`` / ``Problem.solve_many_mid_masked``, several workgroups per solve, with
    an envelope of their own.  Touches no device."""
    fam = family(kernel)
    if n_u < 1:
        return "there is no unknown cell type to solve for"
    return fam.outside(n_rows, n_samples, n_ct, n_u, mode)


def _stack_inits(part, n_rows, n_u):
    """(u0s, alpha0s) of a slice of (u0, alpha0, ...) tuples, as the batch methods take them."""
    return (np.stack([np.asarray(item[0], dtype=np.float64).reshape(n_rows, n_u) for item in part]),
            np.stack([item[1] for item in part]))


def _bcv_batched(meth_f, n_u, counts, iter1, iter2, tol, n_folds, seed, ref, init_option, fraction, problem, batch_kernel):
    """bicross_validation(batched=True): every fold is drawn first, on the host and in the reference's order (the draws do
    not depend on the solves, so the generator's stream is the serial one), the folds upstream skips are dropped, the rest
    are solved by ``problem.solve_many_masked`` (``batch_kernel`` "mid": ``problem.solve_many_mid_masked``) in chunks, and
    ic.py:80-86 is replayed in fold order."""
    folds = []
    for _ in range(n_folds):
        fold = _bcv_draw_fold(meth_f, counts, ref, n_u, init_option, seed, fraction)
        if fold is not None:
            folds.append(fold)
    mode = L.DMF_MODE_PARTIAL if ref is not None else L.DMF_MODE_UNSUPERVISED
    n_rows, n_samples = meth_f.shape
    solved = solve_chunked(problem, family(batch_kernel), (n_rows, n_samples, 0 if ref is None else ref.shape[1], n_u), folds,
                           lambda part: (*_stack_inits([f[1:] for f in part], n_rows, n_u), np.stack([f[0] for f in part])),
                           (mode, iter1, iter2, tol), masked=True)
    total_press, best_u, best_alpha, min_error = 0, None, None, float("inf")
    for b in range(len(folds)):
        test_error = solved[4][b] / solved[5][b]
        total_press += test_error
        if test_error < min_error:
            min_error, best_u, best_alpha = test_error, solved[0][b], solved[1][b]
    return total_press, best_u, best_alpha


def bicross_validation(meth_f, n_u, counts, iter1, iter2, tol, n_folds=10, seed=None, ref=None,
                       init_option="uniform_", fraction=0.3, problem=None, _fold_solver=None, batched=False,
                       batch_kernel="small"):
    """ic.py:58-89: random-mask hold-out error (returns the SUM over folds, as upstream).

    The data are uploaded once (``problem``: a resident upload of (meth_f, counts, ref) to reuse; created here when
    none is given); each fold derives its masked problem on the device and takes its error there.  The draws stay on the
    host and in the reference's order -- seed once, then per fold the mask and the (reseeding) initialiser -- on ONE worker
    thread (numpy's global generator), one fold ahead of the GPU; above the gate of _bcv_draw_fold that thread has the
    device continue the generator's stream for the mask (``solve.draw``) and takes the generator up behind it.
    ``_fold_solver(fold, best) -> (test_error, (u, alpha) or None)`` replaces the device half (tests drive the draw order
    through it without a GPU); its ``stage`` and ``draw`` attributes, where it has them, are picked up like _DeviceFolds'.

    ``batched``: the folds go through ``Problem.solve_many_masked``, one workgroup per fold with its mask read in the kernel
    and the hold-out error taken where the iterates live, instead of one masked problem and one solver
    per fold.  Draws, skipped folds, the running sum and the first strict minimum are the serial route's.  Only inside the
    kernel's envelope (``batched_ic_ineligible``): any other shape raises ValueError before any device work.
    ``batch_kernel`` (with ``batched``): "small", the default, or "mid" -- the folds go through
    ``Problem.solve_many_mid_masked``, several workgroups per fold, inside that family's envelope;
    any other value raises ValueError."""
    family(batch_kernel, "batch_kernel")
    if batched:
        reason = batched_ic_ineligible(n_u, meth_f.shape[0], meth_f.shape[1], 0 if ref is None else ref.shape[1],
                                       L.DMF_MODE_UNSUPERVISED if ref is None else L.DMF_MODE_PARTIAL, kernel=batch_kernel)
        if reason is not None:
            raise ValueError(f"bicross_validation(batched=True): {reason}")
        np.random.seed(seed)
        own = problem is None
        if own:
            problem = Problem(get_context(), meth_f, counts, ref)
        try:
            return _bcv_batched(meth_f, n_u, counts, iter1, iter2, tol, n_folds, seed, ref, init_option, fraction, problem,
                                batch_kernel)
        finally:
            if own:
                problem.close()
    np.random.seed(seed)
    total_press, best_u, best_alpha, min_error = 0, None, None, float("inf")
    own = problem is None and _fold_solver is None
    if own:
        problem = Problem(get_context(), meth_f, counts, ref)
    feed = None
    try:
        solve = _fold_solver if _fold_solver is not None else _DeviceFolds(problem, ref is None, iter1, iter2, tol)
        stage, draw_mask = getattr(solve, "stage", None), getattr(solve, "draw", None)

        def draw(_):
            return _bcv_draw_fold(meth_f, counts, ref, n_u, init_option, seed, fraction, stage, draw_mask)

        feed = Prefetcher(range(n_folds), draw, depth=1, workers=1)
        for _, fold in feed:
            if fold is None:
                continue
            test_error, factors = solve(fold, min_error)
            total_press += test_error
            if test_error < min_error:
                min_error, (best_u, best_alpha) = test_error, factors
    finally:
        if feed is not None:
            feed.close()
        if own:
            problem.close()
    return total_press, best_u, best_alpha


def _note_per_solve(candidates, rank, kernel="small"):
    if candidates and rank == 0:
        print(f"note: candidates n_u = {candidates} are {family(kernel).envelope}: they take the per-solve path")


def _solve_many_chunked(problem, inits, mode, iter1, iter2, tol, n_u, kernel="small"):
    """``problem.solve_many`` on a list of (u0, alpha0), at most bootstrap.batch_chunk solves per call -> (u, alpha, cost);
    ``kernel`` "mid": ``problem.solve_many_mid``, at most bootstrap.mid_batch_chunk solves per call."""
    return solve_chunked(problem, family(kernel), (problem.N, problem.S, problem.n_c, n_u), inits,
                         lambda part: (*_stack_inits(part, problem.N, n_u), None), (mode, iter1, iter2, tol))[:3]


def evaluate_best_ic(meth_f, ref, counts, init_option, ic, seed, iter1, iter2, tol, n_restarts=5,
                     n_u_values=None, batched=False, batch_kernel="small"):
    """ic.py:169-218 -> (u, alpha, n_u, list of criterion values).

    ``n_u_values`` defaults to upstream's hard-coded ``range(1, 26)`` (ic.py:171).  AIC / BIC sweeps
    are sharded across the ranks of an initialised torch.distributed job; CCC and BCV run serially.

    ``batched``: a candidate inside the batched kernel's envelope (``batched_ic_ineligible``) is solved through
    ``Problem.solve_many`` -- the restarts of CCC in one call, the one solve of AIC / BIC as a batch of one, whose cost is
    the cost_f_w the formula takes -- or, for BCV, through ``bicross_validation(batched=True)``.  Any other candidate takes the
    per-solve path inside the same sweep, and one note on rank 0 lists which did.  Initialisers, seeds, the order of the
    candidates and the rank sharding of AIC / BIC are the same either way.

    ``batch_kernel`` (with ``batched``): "small", the default, or "mid" -- the mid-size batch and
    its envelope in the place of the one-launch batch: CCC restarts and the AIC / BIC solve through
    ``Problem.solve_many_mid``, BCV folds through ``Problem.solve_many_mid_masked``.  Any other value raises ValueError.
    """
    family(batch_kernel, "batch_kernel")
    default_range = n_u_values is None
    if default_range:
        n_u_values = range(1, 25 + 1)
    n_u_values = list(n_u_values)
    n_cpg, n_samples = meth_f.shape
    n_ct = ref.shape[1] if ref is not None else 0

    if ic == "minka":
        # upstream calls run_deconvolution with 6 of its 9 arguments here (ic.py:189)
        raise TypeError("run_deconvolution() missing 3 required positional arguments: 'iter1', 'iter2', and 'tol'")

    if ic in ("CCC", "BCV"):
        best_ic, best = float("inf"), (None, None, None)
        scores, per_solve = [], []
        mode = L.DMF_MODE_PARTIAL if ref is not None else L.DMF_MODE_UNSUPERVISED
        # one resident upload for the whole sweep: every restart (CCC) and every fold (BCV) of every candidate solves on it
        with Problem(get_context(), meth_f, counts, ref) as problem:
            for n_u in n_u_values:
                in_batch = batched and batched_ic_ineligible(n_u, n_cpg, n_samples, n_ct, mode, batch_kernel) is None
                if batched and not in_batch:
                    per_solve.append(n_u)
                if ic == "CCC" and in_batch:
                    inits = [_init_on(problem, meth_f, counts, ref, n_u, init_option, seed + restart)
                             for restart in range(n_restarts)]
                    us, alphas, _ = _solve_many_chunked(problem, inits, mode, iter1, iter2, tol, n_u, batch_kernel)
                    u, alpha = us[-1], alphas[-1]  # (the serial loop leaves its last restart's factors behind)
                    score = -compute_ccc(list(alphas))
                elif ic == "CCC":
                    runs = []
                    for restart in range(n_restarts):
                        u, _, alpha = run_deconvolution(meth_f, counts, ref, n_u, init_option, seed + restart, iter1,
                                                        iter2, tol, problem=problem)
                        runs.append(alpha)
                    score = -compute_ccc(runs)
                else:
                    score, u, alpha = bicross_validation(meth_f, n_u, counts, iter1, iter2, tol, fraction=0.3,
                                                         n_folds=n_restarts, seed=seed, ref=ref,
                                                         init_option=init_option, problem=problem, batched=in_batch,
                                                         batch_kernel=batch_kernel)
                scores.append(score)
                if score < best_ic:
                    best_ic, best = score, (u, alpha, n_u)
        _note_per_solve(per_solve, 0, batch_kernel)
        return best[0], best[1], best[2], scores

    # AIC / BIC: one solve per candidate; candidates dealt to ranks longest-first (cost grows with n_u)
    rank, world, _ = shard.dist_state()
    # (checked on every rank before any solve, so that all ranks fail -- or trim -- together)
    not_positive = [n for n in n_u_values if n < 1]
    if not_positive:
        raise ValueError(f"candidate n_u values {not_positive}: a number of unknown cell types is at least 1")
    too_many = [n for n in n_u_values if n_ct + n > L.MAX_K]
    if too_many and default_range:
        # upstream's hard-coded 1..25 (ic.py:171) with a reference matrix of 40 or more known types: the kernels take
        # L.MAX_K cell types in total, so the sweep ends where they do -- a deliberate difference, said out loud
        n_u_values = [n for n in n_u_values if n_ct + n <= L.MAX_K]
        if rank == 0:
            print(f"note: with {n_ct} known cell types the sweep stops at {L.MAX_K - n_ct} unknown ones "
                  f"({L.MAX_K} cell types in total is what the kernels are built for; upstream would go on to 25)")
        if not n_u_values:
            raise ValueError(f"{n_ct} known cell types leave no room for an unknown one ({L.MAX_K} in total at most)")
    elif too_many:
        raise ValueError(f"candidate n_u values {too_many} need more than {L.MAX_K} cell types in total "
                         f"({n_ct} known): outside what the kernels are built for")
    order = sorted(range(len(n_u_values)), key=lambda i: -n_u_values[i])
    mine = [order[i] for i in range(rank, len(order), world)]
    formula = compute_bic if ic == "BIC" else compute_aic
    local, keep = [], None  # keep = this rank's best candidate only (the reference keeps the running best, ic.py:212)

    def on_device(n_u):  # the "SVD" initialiser of this candidate runs on the sweep's resident problem
        return init_option == "SVD" and n_u <= n_samples and init_func.device_svd(n_cpg, n_samples, n_ct, n_u)

    def draw(i):
        # the candidate's initialisation (numpy's global generator: ONE worker thread), drawn while the GPU solves the
        # candidate before it -- except where it runs on the device: that is the solving thread's work (a context is not
        # thread-safe)
        n_u = n_u_values[i]
        return None if on_device(n_u) else _init_on(None, meth_f, counts, ref, n_u, init_option, seed)

    mode = L.DMF_MODE_PARTIAL if ref is not None else L.DMF_MODE_UNSUPERVISED
    if batched:  # (every rank sees the same list: eligibility is a function of the shape)
        _note_per_solve([n for n in n_u_values if batched_ic_ineligible(n, n_cpg, n_samples, n_ct, mode, batch_kernel) is not None],
                        rank, batch_kernel)
    with Problem(get_context(), meth_f, counts, ref) as problem:
        feed = Prefetcher(mine, draw, depth=1, workers=1)
        try:
            for i, drawn in feed:
                n_u = n_u_values[i]
                u0, a0 = drawn if drawn is not None else _init_on(problem, meth_f, counts, ref, n_u, init_option, seed)
                if batched and batched_ic_ineligible(n_u, n_cpg, n_samples, n_ct, mode, batch_kernel) is None:
                    # a batch of one: out_cost is cost_f_w(meth_f, R, alpha, counts) of the final iterate (ic.py:206)
                    us, alphas, costs = _solve_many_chunked(problem, [(u0, a0)], mode, iter1, iter2, tol, n_u, batch_kernel)
                    score = float(formula(costs[0], n_u, n_cpg, n_ct, n_samples))
                    local.append((i, score))
                    if score < (keep[0] if keep else float("inf")) or (keep and score == keep[0] and i < keep[1]):
                        keep = (score, i, us[0], alphas[0])
                    continue
                with Solver(problem, u0, a0, mode) as s:
                    s.step(iter1, iter2, tol)
                    cost = s.direct_cost()  # cost_f_w(meth_f, R, alpha, counts), ic.py:206, where the iterate lives
                    score = float(formula(cost, n_u, n_cpg, n_ct, n_samples))
                    local.append((i, score))
                    # strict '<' on the score, lowest candidate index among equal scores: what ic.py:212 does serially
                    # (a NaN score never wins, exactly as `ic_result < best_ic` upstream); only a candidate that becomes
                    # this rank's best leaves the device
                    if score < (keep[0] if keep else float("inf")) or (keep and score == keep[0] and i < keep[1]):
                        u, alpha, _, _ = s.get()
                        keep = (score, i, u, alpha)
        finally:
            feed.close()
    scores = [s for _, s in shard.gather_objects(local)]
    best_i, best_score = None, float("inf")
    for i, score in enumerate(scores):  # running strict minimum in candidate order, ic.py:212-216
        if score < best_score:
            best_i, best_score = i, score
    if best_i is None:  # every score NaN / inf: upstream returns its initial Nones
        return None, None, None, scores
    n_best = n_u_values[best_i]
    owner = order.index(best_i) % world
    if rank == owner:
        assert keep is not None and keep[1] == best_i
        payload = (keep[2], keep[3])
    else:
        payload = (np.empty((n_cpg, n_best)), np.empty((n_ct + n_best, n_samples)))
    u, alpha = shard.broadcast_arrays(payload, owner)
    return u, alpha, n_best, scores
