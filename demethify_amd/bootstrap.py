"""Bootstrap confidence intervals: host-side mirror of demethify/bootstrap.py.

Replicate i resamples the CpG rows with replacement (``sklearn.utils.resample(..., random_state=seed_i)``
upstream, i.e. ``RandomState(seed_i).randint(0, N, N)`` applied to meth_f, counts and ref alike), runs a
full solve on the resampled problem and contributes one column per sample / unknown to the percentile
bounds.  The full data set is uploaded once; each replicate is a row gather on the device; the percentiles
over the replicates are taken on the device too (dmf_percentile_axis0).  With torch.distributed initialised,
replicate i runs on rank i mod world, the KB-sized proportions are gathered and the profile stacks are
re-partitioned by CpG range with one all-to-all.
"""
from __future__ import annotations

import os

import numpy as np
import pandas as pd

from . import _lib as L
from . import init_func, shard
from .batch import batch_chunk, family, mid_batch_chunk, solve_chunked  # noqa: F401  (the chunk rules are imported from here)
from .deconvolution import (_ICA_REFUSAL, _OUT_OF_SCOPE_INITS, _init_guard, _init_unsupervised, init_BSSMF_md,
                            init_BSSMF_md_p, solve_problem, svd_factors)
from .device import Problem, Solver, get_context
from .init_func import wls_intercept

__all__ = ["bt_ci", "bootstrap_seed_sequence", "bootstrap_row_indices", "match_components"]


def bootstrap_seed_sequence(seed, n_bootstrap):
    """bootstrap.py:27: ``seed = seed + i`` inside the loop is cumulative (seed_0 + i (i + 1) / 2).
    A list-valued seed (CLI ``--seed s``) fails here exactly as upstream does (TypeError)."""
    out = []
    for i in range(n_bootstrap):
        seed = seed + i if seed is not None else None
        out.append(seed)
    return out


def bootstrap_row_indices(seed, n_rows):
    """Row indices sklearn's ``resample`` draws for ``random_state=seed`` (bootstrap.py:28)."""
    return np.random.RandomState(seed).randint(0, n_rows, size=(n_rows,))


def match_components(P):
    """The assignment of a replicate's unknown components to the anchor's: ``perm[a]`` is the anchor component that
    replicate component ``a`` is named after, the permutation that maximises ``sum_a P[a, perm[a]]`` for
    ``P = u_rep.T @ u_anchor[idx]`` (Solver.match_components).  With the column norms fixed this is the assignment of
    least total squared distance between the profiles.  Aligned profiles are ``u[:, argsort(perm)]``, aligned
    proportions permute the last n_u rows of alpha the same way."""
    from scipy.optimize import linear_sum_assignment

    P = np.asarray(P, dtype=np.float64)
    if P.ndim != 2 or P.shape[0] != P.shape[1]:
        raise ValueError(f"P must be square, got shape {P.shape}")
    rows, cols = linear_sum_assignment(P, maximize=True)
    perm = np.empty(P.shape[0], dtype=np.int64)
    perm[rows] = cols
    return perm


def _device_stack(n_local, width):
    """(n_local, width) float64 buffer on this process's GPU for the replicate profiles (B x N x n_u doubles: 16 GB at
    500 x 1e6 x 4, held in HBM instead of travelling to the host and back for the percentiles), or None when PyTorch
    is not importable (the stack then lives on the host, as upstream's)."""
    try:
        import torch
    except ImportError:  # pragma: no cover - torch is part of the target image
        return None
    if not torch.cuda.is_available() or n_local == 0:
        return None
    return torch.empty((n_local, width), dtype=torch.float64, device=torch.device("cuda", get_context().device))


# The number of elements N x S up to which the command line (DEMETHIFY_BATCH=1) sends bootstrap replicates and restarts
# through Problem.solve_many: the largest measured size at which the batched leg wins there and at every smaller measured
# size.  Measured (tools/small_batch_bench.py, profiles/small_batch_bench.txt; medians of five, per-solve against batched):
# 350 x 10 with 2 500 replicates 7.57 s against 0.27 s and with 64 restarts 153 ms against 15 ms, 1 000 x 16 with 64 restarts
# 183 ms against 40 ms -- and 10 000 x 64 with 64 restarts 0.61 s against 4.05 s: there one workgroup per solve loses, so the
# gate sits at 1 000 x 16.
SMALL_BATCH_MAX_ELEMENTS = 16000
# The same gate for purity-constrained runs (--purity; dmf_solve_small_purity), set from the --purity legs of the same tool
# (profiles/small_batch_purity_bench.txt; 100 x 500 iterations, medians of five, per-solve against batched): 350 x 10 with
# 2 500 replicates 21.37 s against 0.28 s and with 64 restarts 226 ms against 5.5 ms, 1 000 x 16 with 64 restarts 1.63 s
# against 67 ms.  The batched leg wins at every measured size, so the gate is the largest of them; nothing larger has been
# measured under purity (without it the batched leg loses at 10 000 x 64, above).
SMALL_BATCH_PURITY_MAX_ELEMENTS = 16000
# The range of N x S in which the command line (DEMETHIFY_BATCH_MID=1) sends bootstrap replicates and restarts through
# Problem.solve_many_mid (several workgroups per solve): the contiguous range of MEASURED sizes at
# which the mid-size leg beats both the per-solve leg and the one-launch batch (tools/mid_batch_bench.py,
# profiles/mid_batch_bench.txt).  MIN > MAX would be a closed gate.  Measured (medians of five; per-solve on the commit
# before / solve_many / solve_many_mid), 64 restarts of at most 200 outer iterations: 1 000 x 16 (6 + 2) 194 / 40 / 28 ms,
# 4 000 x 16 (6 + 2) 296 / 183 / 67 ms, 10 000 x 64 (12 + 4) 609 / 4 050 / 719 ms, 32 768 x 64 829 / - / 2 083 ms,
# 131 072 x 64 1 048 / - / 9 124 ms; bt_ci with 500 replicates at 10 000 x 64 (6 + 2) 4 556 / 4 064 / 2 306 ms.  The mid-size
# leg wins at 16 000 and 64 000 elements; at 640 000 it wins the bootstrap and loses the restarts, so that size stays out.
MID_BATCH_MIN_ELEMENTS, MID_BATCH_MAX_ELEMENTS = 16000, 64000
# The same range for purity-constrained runs (--purity with DEMETHIFY_BATCH_MID_PURITY=1; Problem.solve_many_mid(purity=...),
# dmf_solve_mid_purity), by the same rule, from tools/mid_batch_purity_bench.py (profiles/mid_batch_purity_bench.txt).
# Measured (medians of five, 100 x 500 iterations; per-solve on the commit before / solve_many(purity) /
# solve_many_mid(purity)), 64 restarts: 1 000 x 16 (6 + 2) 1 631 / 67 / 42 ms, 4 000 x 16 (6 + 2) 1 431 / 227 / 67 ms,
# 10 000 x 64 (12 + 4) 3 154 / 2 595 / 414 ms, 32 768 x 64 (12 + 4) 3 419 / - / 1 185 ms; bt_ci with 500 replicates at
# 10 000 x 64 (6 + 2) 19 136 / 1 944 / 1 366 ms.  The mid-size leg wins every case at every measured size, 16 000, 64 000,
# 640 000 and 2 097 152 elements, so the gate is that whole range; nothing larger and nothing smaller was measured.
MID_BATCH_PURITY_MIN_ELEMENTS, MID_BATCH_PURITY_MAX_ELEMENTS = 16000, 2097152


def batched_ineligible(n_u, n_rows, n_samples, n_ct, init_option, purity, mode, observe=None, align=False,
                       profile_rows="position", purity_batched=False, kernel="small", mid_purity=False):
    """Why a loop of solves cannot go through ``Problem.solve_many`` (one launch for many solves), as a sentence, or None
    when it can: at least one unknown type, no purity constraint, nobody watching single replicates, no component
    alignment, profile rows by position, an initialiser that does not read the data (``uniform_``, ``beta``, or the silent
    replacement by ``uniform_`` when there are more unknown types than samples) and a shape the kernel takes.
    ``purity_batched``: the caller has asked for the purity variant of the kernel (``solve_many(purity=...)``), so a purity
    vector passes where there is a reference to hold at that mass.  ``kernel``: "small" (``Problem.solve_many``, the default)
    or "mid" (``Problem.solve_many_mid``, several workgroups per solve): the mid-size batch has an envelope of its own, and
    it refuses a purity vector whatever ``purity_batched`` says unless ``mid_purity`` is set (a switch of its own, because
    the refusal without it is pinned): then ``solve_many_mid(purity=...)`` takes the vector where there is a reference to
    hold at that mass.  Touches no device."""
    fam = family(kernel)
    if n_u < 1:
        return "there is no unknown cell type to solve for"
    if purity is not None and np.size(purity) > 0:
        if kernel == "mid" and not mid_purity:
            return "the purity-constrained alpha phase is not part of the mid-size batch"
        if kernel == "small" and not purity_batched:
            return ("the purity-constrained alpha phase is not part of the batched kernel unless it is asked for "
                    "(bt_ci(..., batched_purity=True), batched_ineligible(..., purity_batched=True))")
        if mode != L.DMF_MODE_PARTIAL or n_ct < 1:
            return "a purity constraint has no meaning without a reference: there is no known block to hold at that mass"
    if observe is not None:
        return "_observe looks at one replicate's solver, which a batched solve does not have"
    if align:
        return "aligning the unknown components needs every replicate's solver"
    if profile_rows != "position":
        return 'profile_rows="cpg" needs every replicate\'s solver'
    option = "uniform_" if (init_option != "uniform_" and n_u > n_samples) else init_option
    if option not in ("uniform_", "beta"):
        return f"the initialiser {init_option!r} reads the resampled data"
    return fam.outside(n_rows, n_samples, n_ct, n_u, mode)


def bt_ci(confidence_level, n_bootstrap, n_u, meth_f, counts, ref, init_option, n_iter1, n_iter2, tol, header,
          outdir, samples, purity, seed, materialize=True, _observe=None, anchor=None, align_unknown=None,
          profile_rows="position", batched=False, batched_purity=False, batch_kernel="small", batched_mid_purity=False):
    """bootstrap.py:10-93 -> [proportions CI DataFrame, (profile CI DataFrame)]; writes the two CSVs.
    materialize=False (the CLI, which ignores the return value) skips building the N-row DataFrame of tuples for the
    profile intervals: the CSV is written by the library and the second result is the (lower, upper) array pair.
    _observe(i, seed_i, row_indices, solver) is called after replicate i's solve (tests look at the replicate through it;
    ``solver.component_perm`` is the replicate's assignment, None where it was not aligned).

    ``ref=None`` (no reference panel; upstream's bt_ci fails at ``ref.shape`` there): every replicate is an unsupervised
    solve of the resampled data from ``_init_unsupervised(init_option, ..., seeds[i])``, ``header`` is [] and the rows of
    the proportions table are the unknown_cell_i.  ``purity`` has no meaning without a reference (ValueError).

    ``align_unknown``: name the unknown components of every replicate after those of one solve, the anchor, before the
    percentiles are taken: P = u_rep.T @ u_anchor[idx] on the device, ``match_components(P)``, and
    the replicate's profile columns / proportion rows are stored in the anchor's order.  None = True without a reference
    and False with one (upstream's unaligned percentiles, every existing call as before); skipped for n_u == 1.
    ``anchor`` = (u, alpha) of the solve the components are named after (the CLI passes its point estimate); absent, it is
    solved here on every rank from the unresampled data, ``seed`` and the same initialiser.

    ``profile_rows``: what row j of the profile intervals speaks about.  "position" (the default, upstream's): the j-th
    resampled row of every replicate, B different CpGs.  "cpg": CpG j's own estimates -- replicate i contributes
    ``u_i[first_i[j]]``, the row of the lowest position that drew CpG j, and nothing where it did not draw it (NaN in the
    stack); the bounds are ``np.nanpercentile`` over the replicates, (nan, nan) for a CpG no replicate drew (DESIGN.md
    section 6.1).  Composes with ``align_unknown``; ignored for n_u == 0; the proportions table is the same either way.

    ``batched``: this rank's replicates go through ``Problem.solve_many`` in chunks, one workgroup per replicate, rows
    read through the replicate's index list.  Row indices and initialisers are drawn per replicate
    from seed_i in the reference's order, exactly as without it.  Only for the cases ``batched_ineligible`` accepts; any
    other raises ValueError naming the reason before any device work.  A purity vector is among those reasons unless
    ``batched_purity`` is set as well: the replicates then run the purity variant of the kernel (``solve_many(purity=p / 100)``)
    from ``init_BSSMF_md_p``'s starting points.  (Two switches because ``batched=True`` alone is pinned to refuse purity.)

    ``batch_kernel``: which batch ``batched=True`` means.  "small" (the default): ``Problem.solve_many``, as above.  "mid":
    ``Problem.solve_many_mid``, several workgroups per replicate, in chunks of ``mid_batch_chunk``;
    eligibility is ``batched_ineligible(..., kernel="mid")``, which refuses a purity vector whatever ``batched_purity`` says.
    ``batched_mid_purity`` (looked at only with ``batched=True, batch_kernel="mid"``) opens it: the purity replicates then go
    through ``solve_many_mid(purity=p / 100)`` in the same chunks.  Any other ``batch_kernel`` raises ValueError."""
    if profile_rows not in ("position", "cpg"):
        raise ValueError(f'profile_rows must be "position" or "cpg", got {profile_rows!r}')
    fam = family(batch_kernel, "batch_kernel")
    if batched:
        will_align = bool(ref is None if align_unknown is None else align_unknown) and n_u >= 2
        reason = batched_ineligible(n_u, meth_f.shape[0], meth_f.shape[1], 0 if ref is None else ref.shape[1], init_option,
                                    purity, L.DMF_MODE_UNSUPERVISED if ref is None else L.DMF_MODE_PARTIAL, _observe,
                                    will_align, profile_rows, purity_batched=bool(batched_purity), kernel=batch_kernel,
                                    mid_purity=bool(batched_mid_purity))
        if reason is not None:
            prefix = "bt_ci(batched=True)" if batch_kernel == "small" else f'bt_ci(batched=True, batch_kernel="{batch_kernel}")'
            raise ValueError(f"{prefix}: {reason}")
    by_cpg = profile_rows == "cpg"
    if ref is None:
        if n_u < 1:
            raise ValueError("a bootstrap without a reference needs at least one unknown cell type")
        if purity:
            raise ValueError("--purity without a reference has no meaning: there is no known block to hold at that mass")
        # deconvolution.py:108-117, before any device work
        option = "uniform_" if (init_option != "uniform_" and n_u > meth_f.shape[1]) else init_option
        if option == "uniform":
            raise NameError("name 'R_trunc' is not defined")  # upstream's undefined name (deconvolution.py:117), kept
        if option in _OUT_OF_SCOPE_INITS:
            raise NotImplementedError(_ICA_REFUSAL)
    if align_unknown is None:
        align_unknown = ref is None
    align = bool(align_unknown) and n_u >= 2
    purity_frac = None
    if purity:
        # upstream quirk kept: bt_ci takes the raw percentages and uses p / 100 (bootstrap.py:18) while main()
        # passes 1 - p / 100 to the point estimate (demethify.py:77)
        purity_frac = np.array(purity) / 100.0
    supervised = n_u == 0
    a = 1 - confidence_level / 100
    lower_percentile = 100 * (a / 2)
    upper_percentile = 100 * (1 - (a / 2))
    n_rows, n_samples = meth_f.shape
    n_ct = 0 if ref is None else ref.shape[1]
    mode = L.DMF_MODE_UNSUPERVISED if ref is None else L.DMF_MODE_PARTIAL

    rank, world, _ = shard.dist_state()
    seeds = bootstrap_seed_sequence(seed, n_bootstrap)
    local = []
    if supervised and init_func.device_wls(n_rows, n_samples, n_ct):
        # one resident problem; a replicate is a row gather on the device and one regression launch for all its samples
        # (samples the device declines are solved on the host, from indexed copies made for that replicate only)
        from .staging import indices_to_device

        ctx = get_context()
        with Problem(ctx, meth_f, counts, ref) as full:
            for i in shard.my_items(n_bootstrap, rank, world):
                idx = bootstrap_row_indices(seeds[i], n_rows)
                with full.gather(indices_to_device(idx, ctx)) as resampled:
                    props = resampled.wls_intercept(None, "dv", host_arrays=lambda: (meth_f[idx], counts[idx], ref[idx]))
                local.append((i, (None, props)))
    elif supervised:
        for i in shard.my_items(n_bootstrap, rank, world):
            idx = bootstrap_row_indices(seeds[i], n_rows)
            mf, ct, rf = meth_f[idx], counts[idx], ref[idx]
            props = np.concatenate([wls_intercept(ct[:, k:k + 1] * mf[:, k:k + 1], ct[:, k:k + 1], rf)
                                    for k in range(n_samples)], axis=1)
            local.append((i, (None, props)))
    elif batched:
        # one resident problem, one solve_many call per chunk of this rank's replicates: replicate i reads its rows through
        # idx_i and starts from the initialiser of seed_i (data-free: only the shapes of the arrays it is given matter)
        u_stack = None
        mine = shard.my_items(n_bootstrap, rank, world)
        shape_f = np.broadcast_to(meth_f[:1], meth_f.shape)

        def stack(part):
            idx = np.stack([bootstrap_row_indices(seeds[i], n_rows) for i in part])
            inits = []
            for i in part:
                if ref is None:
                    inits.append(_init_unsupervised(init_option, shape_f, n_u, seeds[i]))
                elif purity_frac is not None:
                    u0, _, a0 = init_BSSMF_md_p(init_option, shape_f, np.broadcast_to(counts[:1], counts.shape),
                                                np.broadcast_to(ref[:1], ref.shape), n_u, purity_frac, seed=seeds[i],
                                                rb_alg=wls_intercept, _stack=False)
                    inits.append((u0, a0))
                else:
                    u0, _, a0 = init_BSSMF_md(init_option, shape_f, np.broadcast_to(counts[:1], counts.shape),
                                              np.broadcast_to(ref[:1], ref.shape), n_u, rb_alg=wls_intercept, seed=seeds[i],
                                              _stack=False)
                    inits.append((u0, a0))
            return np.stack([u0 for u0, _ in inits]), np.stack([a0 for _, a0 in inits]), idx

        with Problem(get_context(), meth_f, counts, ref) as full:
            solved = solve_chunked(full, fam, (n_rows, n_samples, n_ct, n_u), mine, stack, (mode, n_iter1, n_iter2, tol),
                                   purity=purity_frac)
        local.extend((i, (solved[0][j], solved[1][j])) for j, i in enumerate(mine))
    else:
        # The host work of the replicates ahead (MT19937 index draw of N rows; uniform N x n_u + Dirichlet init: ~10 + ~13 ms
        # at 1e6 rows) runs on worker threads while the GPU gathers and solves replicate i.  The row draw has its own
        # RandomState(seed_i) (what sklearn's resample does); the init re-seeds numpy's GLOBAL stream with seed_i
        # (deconvolution.py:41), so the draws do not depend on the order the threads run in -- but only ONE thread may
        # run initialisers at a time.  When the init does not look at the resampled data ('uniform_' and the other
        # data-free options) the two draws are independent and get a thread each; otherwise one thread does both.
        from .staging import Prefetcher, indices_to_device, reserve, to_device

        ctx = get_context()
        reserve(((n_rows, n_u), (n_ct + n_u, n_samples), (n_rows,)), count=2)

        mine = shard.my_items(n_bootstrap, rank, world)
        # "SVD" reads the data too, and above its gate it does so on the device: on the replicate's gathered problem, by the
        # solving thread (a context is not thread-safe), with u0 staying in HBM; the worker threads then only draw the rows
        svd_on_device = (init_option == "SVD" and n_u <= n_samples
                         and init_func.device_svd(n_rows, n_samples, n_ct, n_u))
        needs_data = init_option in ("uniform", "SVD") and not svd_on_device

        def svd_init(resampled, idx):
            u0, H = svd_factors(lambda: (meth_f[idx], counts[idx], None if ref is None else ref[idx]), None, None, n_u,
                                problem=resampled, keep_on_device=True)
            if ref is None:  # deconvolution.py:135-137: no guard on the unsupervised path
                a0 = init_func.project_simplex_columns(H)
            elif purity_frac is not None:  # deconvolution.py:262, as coded
                a0 = np.vstack((purity_frac * init_func.project_simplex_columns(H[:-n_u]),
                                init_func.project_simplex_columns(H[-n_u:])))
            else:
                a0 = _init_guard(init_func.project_simplex_columns(H), n_u)
            return (u0,) + tuple(to_device((a0,), ctx))

        def draw_init(i, idx=None):
            mf = meth_f[idx] if needs_data else np.broadcast_to(meth_f[:1], meth_f.shape)
            if ref is None:  # (below the device gate "SVD" takes the host route on the resampled rows)
                return to_device(_init_unsupervised(init_option, mf, n_u, seeds[i]), ctx)
            ct = counts[idx] if needs_data else np.broadcast_to(counts[:1], counts.shape)
            rf = ref[idx] if needs_data else np.broadcast_to(ref[:1], ref.shape)
            if purity_frac is not None:
                u0, _, a0 = init_BSSMF_md_p(init_option, mf, ct, rf, n_u, purity_frac, seed=seeds[i], rb_alg=wls_intercept, _stack=False)
            else:
                u0, _, a0 = init_BSSMF_md(init_option, mf, ct, rf, n_u, rb_alg=wls_intercept, seed=seeds[i], _stack=False)
            return to_device((u0, a0), ctx)  # page-locked copy + upload on the context's copy stream, here in the worker

        def draw_rows(i):
            # (the row indices travel to HBM from here too: 8 MB from pageable memory took the solving thread ~1 ms per replicate)
            idx = bootstrap_row_indices(seeds[i], n_rows)
            return idx, indices_to_device(idx, ctx)

        def draw_both(i):
            idx, idx_dev = draw_rows(i)
            return (idx, idx_dev) + tuple(draw_init(i, idx))

        def start_feeds():
            if needs_data:
                return (Prefetcher(mine, draw_both, depth=2, workers=1),)
            if svd_on_device:
                return (Prefetcher(mine, draw_rows, depth=2, workers=1),)
            return (Prefetcher(mine, draw_rows, depth=2, workers=1), Prefetcher(mine, draw_init, depth=2, workers=1))

        def solve_anchor(full):
            # the solve the components are named after: the unresampled data, `seed`, the replicates' initialiser
            if ref is None:
                u0, a0 = _init_unsupervised(init_option, meth_f, n_u, seed, problem=full)
            elif purity_frac is not None:
                u0, _, a0 = init_BSSMF_md_p(init_option, meth_f, counts, ref, n_u, purity_frac, seed=seed, rb_alg=wls_intercept,
                                            _stack=False, problem=full)
            else:
                u0, _, a0 = init_BSSMF_md(init_option, meth_f, counts, ref, n_u, rb_alg=wls_intercept, seed=seed, _stack=False,
                                          problem=full)
            return solve_problem(full, u0, a0, mode, n_iter1, n_iter2, tol, purity=purity_frac)

        # (an anchor solved here draws from numpy's global generator: the worker threads start after it)
        feeds = start_feeds() if not (align and anchor is None) else ()
        u_stack = _device_stack(len(mine), n_rows * n_u)  # replicate profiles stay in HBM when torch is there
        anchor_dev = None
        try:
            with Problem(ctx, meth_f, counts, ref) as full:
                if align:
                    if anchor is None:
                        anchor = solve_anchor(full)
                        feeds = start_feeds()
                    anchor_u = np.ascontiguousarray(anchor[0], dtype=np.float64).reshape(n_rows, -1)
                    if anchor_u.shape[1] != n_u:
                        raise ValueError(f"anchor profiles have shape {np.shape(anchor[0])}, expected {(n_rows, n_u)}")
                    anchor_dev, = to_device((anchor_u,), ctx)  # resident for every replicate's comparison
                for j, parts in enumerate(zip(*feeds)):
                    if needs_data:
                        (i, (idx, idx_dev, u0, a0)), = parts
                    elif svd_on_device:
                        (i, (idx, idx_dev)), = parts
                        u0 = a0 = None
                    else:
                        (i, (idx, idx_dev)), (i2, (u0, a0)) = parts
                        assert i == i2
                    with full.gather(idx_dev) as resampled, \
                            Solver(resampled, *(svd_init(resampled, idx) if svd_on_device else (u0, a0)), mode) as s:
                        if purity_frac is not None:
                            s.set_purity(purity_frac)
                        s.step(n_iter1, n_iter2, tol)
                        # which anchor component each of the replicate's is: n_u x n_u inner products taken where the
                        # profiles live, the assignment on the host; `order` renames columns / rows on the way out
                        s.component_perm = match_components(s.match_components(anchor_dev, idx_dev)) if align else None
                        order = np.argsort(s.component_perm) if align else None
                        if _observe is not None:
                            _observe(i, seeds[i], idx, s)
                        if u_stack is not None:
                            if by_cpg:
                                s.copy_u_by_cpg(u_stack[j], idx_dev, n_rows, columns=order)
                            else:
                                s.copy_u_to(u_stack[j], columns=order)
                            u, alpha = None, s.get_alpha()
                        else:
                            u, alpha, _, _ = s.get()
                            if align:
                                u = np.ascontiguousarray(u[:, order])
                            if by_cpg:
                                u = _rows_by_cpg(u, idx, n_rows)
                        if align:
                            alpha[n_ct:] = alpha[n_ct:][order]
                        local.append((i, (u, alpha)))
        finally:
            for f in feeds:
                f.close()
    # proportions (K x S per replicate, KB-sized) go to every rank
    merged = shard.gather_objects([(i, pa) for i, (_, pa) in local])
    props_stack = np.stack([pa for _, pa in merged])  # (B, K, S)
    q = [lower_percentile, upper_percentile]

    results = []
    if supervised:
        # (no device in play on this branch: NNLS per sample on the host, as upstream)
        lower_p, upper_p = np.percentile(props_stack, q, axis=0)
    else:
        lower_p, upper_p = get_context().percentile_axis0(props_stack, q)
    unknown_header = [] if supervised else ["unknown_cell_" + str(i + 1) for i in range(n_u)]
    cell_types = header + unknown_header
    table = {f"Sample_{i + 1}": [(lower_p[k, i], upper_p[k, i]) for k in range(n_ct + n_u)]
             for i in range(n_samples)}
    proportions_df = pd.DataFrame(table, index=cell_types)
    proportions_df.columns = samples
    proportions_df.index.name = "Cell Type"
    if rank == 0:
        proportions_df.to_csv(outdir + "/confidence_interval_celltypes_proportions.csv", index=True)
    results.append(proportions_df)

    if not supervised:
        # Profile estimates: B x N x n_u doubles (16 GB at 500 x 1e6 x 4).  Each rank holds the replicates it
        # ran; one all-to-all re-partitions them by CpG range and every rank takes the percentiles of its
        # range on its GPU (shard.percentile_over_replicates); rank 0 writes the CSV.
        if u_stack is not None:
            local_u = u_stack
        else:
            local_u = (np.stack([pu.reshape(-1) for _, (pu, _) in local]) if local else np.empty((0, n_rows * n_u)))
        percentile_fn = get_context().nanpercentile_axis0 if by_cpg else get_context().percentile_axis0
        bounds = shard.percentile_over_replicates(local_u, n_bootstrap, q, percentile_fn)
        if bounds is not None:
            # by resampled position, as upstream, or by CpG (profile_rows)
            lower_u, upper_u = (b.reshape(n_rows, n_u) for b in bounds)
            path = outdir + "/confidence_interval_methylation_estimate.csv"
            if not _write_interval_csv(path, unknown_header, lower_u, upper_u) or materialize:
                # upstream's way (bootstrap.py:85-91): N Python tuples per column through DataFrame.to_csv, ~20 s at 1e6 rows
                ref_estimate_df = pd.DataFrame({unknown_header[k]: [(lower_u[j, k], upper_u[j, k]) for j in range(n_rows)]
                                                for k in range(n_u)})
                if not os.path.exists(path):
                    ref_estimate_df.to_csv(path, index=False)
                results.append(ref_estimate_df)
            else:
                results.append((lower_u, upper_u))
    return results


def _rows_by_cpg(u, idx, n_rows):
    """``u`` (one row per resampled position, position j being CpG ``idx[j]``) as one row per CpG: the row of the lowest
    position that drew it, NaN where none did -- the host twin of Solver.copy_u_by_cpg."""
    out = np.full((n_rows, u.shape[1]), np.nan)
    cpgs, first = np.unique(idx, return_index=True)
    out[cpgs] = u[first]
    return out


def _write_interval_csv(path, columns, lower, upper) -> bool:
    """The (lower, upper) table as DataFrame.to_csv writes a DataFrame of tuples, by the library's writer
    (dmf_write_interval_csv: byte-identical, tests/test_host.py; a NaN bound is written ``nan``, as repr writes it).
    False if a column name would need CSV quoting."""
    import ctypes as C

    if any(ch in name for name in columns for ch in ',"\r\n'):
        return False
    lib = L.load()
    lower = np.ascontiguousarray(lower, dtype=np.float64)
    upper = np.ascontiguousarray(upper, dtype=np.float64)
    numpy_scalar_repr = int(str((np.float64(0.5),)).startswith("(np.float64("))  # numpy >= 2 prints scalars that way
    try:
        os.remove(path)
    except OSError:
        pass
    rc = lib.dmf_write_interval_csv(path.encode(), ",".join(columns).encode(), lower.ctypes.data_as(C.c_void_p),
                                    upper.ctypes.data_as(C.c_void_p), lower.shape[0], lower.shape[1], numpy_scalar_repr,
                                    min(16, os.cpu_count() or 1))
    return rc == 0
