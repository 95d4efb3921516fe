"""``demethify`` command line: same flags, defaults, input formats and output files as the
reference's demethify/demethify.py, with the solver running on the GPU.

Multi-GPU: launch one process per GPU, e.g.
    python -m torch.distributed.run --nproc-per-node 8 -m demethify_amd --methfreq ... --restart 64
Restarts, bootstrap replicates and model-selection candidates are then sharded over the ranks
(demethify_amd/shard.py); rank 0 writes the output files.

Deliberate differences from upstream, all flagged at run time:
  * ``--restart r``: upstream re-runs the SAME seed r times; here restart k > 0 uses seed + k
    (restart 0 is bit-compatible), SURVEY.md section 8b.
  * ``--plot`` is ignored with a note and ``--init SVD|ICA`` exits with a message (outside this build's scope).
  * ``--confidence`` without ``--ref`` (upstream's bootstrap fails at ``ref.shape``): needs ``--nbunknown >= 1``; the point
    estimate runs first and every replicate's unknown types are matched to its profiles before the percentiles are taken
    (DESIGN.md section 6).  With ``--ref`` the intervals are upstream's, unaligned.
  * ``DEMETHIFY_CI_ROWS=cpg`` (environment; default ``position``, upstream's): row j of
    confidence_interval_methylation_estimate.csv is the interval of CpG j's own estimates over the replicates that drew it,
    (nan, nan) where none did, instead of the percentiles by resampled position.
  * ``DEMETHIFY_BATCH=1`` (environment; default ``0``): ``--confidence`` replicates and ``--restart`` restarts of a small
    problem are solved many per kernel launch, one workgroup each, when the case is eligible
    (bootstrap.batched_ineligible) and N x S is at most bootstrap.SMALL_BATCH_MAX_ELEMENTS (with ``--purity``:
    bootstrap.SMALL_BATCH_PURITY_MAX_ELEMENTS, the purity variant of the kernel); otherwise a one-line note says
    why not and the run takes the per-solve path.  With ``--ic`` the sweep's restarts (CCC) and folds (BCV) go the same
    way (evaluate_best_ic(batched=True)) for the criteria of ic.SMALL_BATCH_IC_CRITERIA up to
    ic.SMALL_BATCH_IC_MAX_ELEMENTS elements; a candidate outside the kernel's envelope takes the per-solve path inside it.
  * ``DEMETHIFY_BATCH_MID=1`` (environment; default ``0``): where the route above was not taken, ``--confidence`` replicates
    and ``--restart`` restarts go through ``Problem.solve_many_mid`` (several workgroups per solve) when the case is eligible
    (bootstrap.batched_ineligible(kernel="mid")) and N x S lies within [bootstrap.MID_BATCH_MIN_ELEMENTS,
    bootstrap.MID_BATCH_MAX_ELEMENTS]; otherwise a one-line note says why and the per-solve path runs.  ``--ic`` sweeps have
    a switch of their own (``DEMETHIFY_BATCH_MID_IC``, below): this one leaves them on the per-solve path.  A ``--purity`` run
    is refused by it with a note.
  * ``DEMETHIFY_BATCH_MID_PURITY=1`` (environment; default ``0``): asked after the two above, for ``--purity`` runs only:
    ``--confidence`` replicates and ``--restart`` restarts go through ``Problem.solve_many_mid(purity=...)`` (the Frank-Wolfe
    alpha launch of the mid-size batch) when the case is eligible (bootstrap.batched_ineligible(kernel="mid",
    mid_purity=True)) and N x S lies within [bootstrap.MID_BATCH_PURITY_MIN_ELEMENTS,
    bootstrap.MID_BATCH_PURITY_MAX_ELEMENTS]; otherwise a one-line note says why and the per-solve path runs.
  * ``DEMETHIFY_BATCH_MID_IC=1`` (environment; default ``0``): asked for ``--ic`` sweeps after ``DEMETHIFY_BATCH``'s own
    ``--ic`` route was not taken: the sweep goes through evaluate_best_ic(batched=True, batch_kernel="mid") -- CCC restarts and
    the AIC / BIC solve through ``Problem.solve_many_mid``, BCV folds through ``Problem.solve_many_mid_masked`` (a hold-out
    mask per solve, several workgroups per solve) -- when the criterion is in ic.MID_BATCH_IC_CRITERIA and N x S lies within
    [ic.MID_BATCH_IC_MIN_ELEMENTS, ic.MID_BATCH_IC_MAX_ELEMENTS]; otherwise a one-line note says why and the per-solve path
    runs.  A candidate outside the mid-size batch's envelope takes the per-solve path inside the sweep.
  * ``--ic NAME [n [lo hi]]``: upstream sweeps the hard-coded range 1..25 (ic.py:171); two more values after the
    restart count restrict the sweep to lo..hi unknown types (``--ic BIC 5 2 12``).  Without them: 1..25, as upstream.
"""
from __future__ import annotations

import argparse
import os
import sys
import warnings
from time import time
from typing import NamedTuple

import numpy as np
import pandas as pd

from . import tables

logo = r"""
    ____                      __  __    _ ____
   / __ \___  ____ ___  ___  / /_/ /_  (_) __/_  __
  / / / / _ \/ __ `__ \/ _ \/ __/ __ \/ / /_/ / / /
 / /_/ /  __/ / / / / /  __/ /_/ / / / / __/ /_/ /
/_____/\___/_/ /_/ /_/\___/\__/_/ /_/_/_/  \__, /
                                          /____/    (MI355X build)
"""


class BatchSwitch(NamedTuple):
    """One DEMETHIFY_BATCH* switch (the module docstring says what each is for), as ``main``'s ``batch_route`` reads it."""
    switch: str
    family: str  # batch.family: "small", one workgroup per solve, or "mid", several
    applies: str  # "solves" (--restart restarts and --confidence replicates) or "--ic"
    module: str  # where the gate constants live: they are read through the module at every call
    gate: tuple  # (MIN name, or None for a one-sided gate, MAX name): the sizes N x S at which the route was measured faster
    # "solves" and --purity: "own gate" (eligible, inside ``purity_gate``), "refused" (with batched_ineligible's sentence, and
    # silently where an "only" switch is on as well: that one speaks for a purity run) or "only" (silent without --purity)
    purity: str = None
    purity_gate: tuple = None
    purity_keyword: str = None  # the bt_ci keyword a purity run sets next to batched= and batch_kernel=
    criteria: str = None  # "--ic": the name of the tuple of criteria the route is taken for


# in the order of asking: per ``applies`` the first switch that is on and accepts takes the run, each refusal prints its note
BATCH_SWITCHES = (
    BatchSwitch("DEMETHIFY_BATCH", "small", "solves", "bootstrap", (None, "SMALL_BATCH_MAX_ELEMENTS"), purity="own gate",
                purity_gate=(None, "SMALL_BATCH_PURITY_MAX_ELEMENTS"), purity_keyword="batched_purity"),
    BatchSwitch("DEMETHIFY_BATCH_MID", "mid", "solves", "bootstrap", ("MID_BATCH_MIN_ELEMENTS", "MID_BATCH_MAX_ELEMENTS"),
                purity="refused"),
    BatchSwitch("DEMETHIFY_BATCH_MID_PURITY", "mid", "solves", "bootstrap",
                ("MID_BATCH_PURITY_MIN_ELEMENTS", "MID_BATCH_PURITY_MAX_ELEMENTS"), purity="only",
                purity_keyword="batched_mid_purity"),
    BatchSwitch("DEMETHIFY_BATCH", "small", "--ic", "ic", (None, "SMALL_BATCH_IC_MAX_ELEMENTS"), criteria="SMALL_BATCH_IC_CRITERIA"),
    BatchSwitch("DEMETHIFY_BATCH_MID_IC", "mid", "--ic", "ic", ("MID_BATCH_IC_MIN_ELEMENTS", "MID_BATCH_IC_MAX_ELEMENTS"),
                criteria="MID_BATCH_IC_CRITERIA"),
)


def build_parser():
    """Flag surface of demethify/demethify.py:27-45 (same names, nargs, types and defaults)."""
    parser = argparse.ArgumentParser(description="DeMethify - Partial reference-based Methylation Deconvolution")
    parser.add_argument('--methfreq', nargs='+', type=str, required=True, help='Methylation frequency file path (values between 0 and 1)')
    parser.add_argument('--ref', nargs='?', type=str, help='Methylation reference matrix file path')
    parser.add_argument('--iterations', nargs=2, type=int, help='Numbers of iterations for outer and inner loops (default without purity = 10000, 20, with purity= 100, 500)')
    parser.add_argument('--nbunknown', nargs=1, type=int, help="Number of unknown cell types to estimate ")
    parser.add_argument('--purity', nargs='+', type=float, help="The purities of the samples in percent [0,100], if known")
    parser.add_argument('--termination', nargs=1, type=float, default=1e-2, help='Termination condition for cost function (default = 1e-2)')
    parser.add_argument('--init', nargs="?", default='uniform_', help='Initialisation option, the default is uniform_, and the options are: uniform, uniform_, beta, SVD, ICA. ')
    parser.add_argument('--outdir', nargs='?', required=True, help='Output directory')
    parser.add_argument('--fillna', action="store_true", help='Replace every NA by 0 in the given data')
    parser.add_argument('--ic', nargs="+", help='Select number of unknown cell types by minimising a criterion (AIC, BIC, CCC, BCV, minka)')
    parser.add_argument('--confidence', nargs=2, type=int, help='Outputs bootstrap confidence intervals, takes confidence level and boostrap iteration numbers as input.')
    parser.add_argument('--plot', action="store_true", help='Plot cell type proportions estimates for each sample, eventually with confidence intervals. ')
    parser.add_argument('--restart', nargs=1, type=int, help='Number of random restarts among which to select the one with the lowest cost/highest loglikelihood')
    parser.add_argument('--seed', nargs=1, type=int, default=1, help='Set a seed integer number for random number generation for reproducibility. ')
    parser.add_argument('--noprint', action="store_true", help='Doesnt show the logo.')
    parser.add_argument('--bedmethyl', action='store_true', help="Flag to indicate that the input will be bedmethyl files, modkit style")
    return parser


def read_inputs(args, parsed=None):
    """demethify.py:102-143: bedmethyl (tab separated, percent) or csv (fractions) input.  The per-sample files
    are parsed in parallel (and 1 / world of them per rank when distributed): demethify_amd/tables.py."""
    ref, header = None, []
    sep = '\t' if args.bedmethyl else ','
    if args.ref:
        table = pd.read_csv(args.ref, sep=sep)
        if args.bedmethyl:
            table = table.iloc[:, 3:]
        if args.fillna:
            table = table.fillna(0)
        header = list(table.columns)
        ref = table.values
    meth_f, counts = tables.read_samples(args.methfreq, bool(args.bedmethyl), bool(args.fillna), parsed=parsed)
    return ref, header, meth_f, counts


def _init_distributed():
    """One process per GPU when launched through torch.distributed.run; no-op otherwise."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return 0
    import torch
    import torch.distributed as dist

    device = int(os.environ.get("DEMETHIFY_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    backend = os.environ.get("DEMETHIFY_DIST_BACKEND", "nccl" if torch.cuda.is_available() else "gloo")
    if torch.cuda.is_available():
        torch.cuda.set_device(device)
    if backend == "nccl":  # RCCL over xGMI: one rank per GPU
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", device))
    else:  # gloo: CPU collectives (tests; several ranks may then share one GPU via DEMETHIFY_DEVICE)
        dist.init_process_group(backend="gloo")
    return dist.get_rank()


def main(argv=None):
    warnings.filterwarnings("ignore")
    args = build_parser().parse_args(argv)

    # ---- post-parse normalisation, demethify.py:51-100
    if args.restart is None:
        args.restart = 1
    else:
        args.restart = args.restart[0]
    if not args.iterations:
        args.iterations = [100, 500] if args.purity else [10000, 20]
    if isinstance(args.termination, list):
        args.termination = args.termination[0]
    purity = None
    if args.purity:  # demethify.py:69-77
        purity = np.array(args.purity)
        if np.any((purity >= 0) & (purity <= 1)):
            print("Purity is between 0 and 1, are you sure that it's a percentage?")
        elif np.any((purity < 0) & (purity > 100)):
            sys.stderr.write("Error: Invalid value for purity, not within [0,100] bounds.")
            sys.exit(1)
        purity = 1 - (purity / 100.0)
    nb_r = 5
    ic_range = None
    if args.ic:
        if args.nbunknown:
            sys.stderr.write("Error: --ic cannot be used with --nbunknown.\n")
            sys.exit(1)
        if len(args.ic) > 1:
            nb_r = int(args.ic[1])
        if len(args.ic) == 4:  # extension: candidate range lo..hi (upstream ignores anything after the count)
            lo, hi = int(args.ic[2]), int(args.ic[3])
            if lo < 1 or hi < lo:
                sys.stderr.write("Error: --ic NAME n lo hi needs 1 <= lo <= hi.\n")
                sys.exit(1)
            ic_range = range(lo, hi + 1)
        elif len(args.ic) > 2:
            sys.stderr.write("Error: --ic takes NAME [n_restarts [lo hi]].\n")
            sys.exit(1)
        args.ic = args.ic[0]
    if args.init in ("SVD", "ICA"):
        sys.stderr.write(f"Error: --init {args.init} (one-shot LAPACK initialiser, demethify/init_func.py) is not part "
                         "of this build; use uniform_, uniform or beta.\n")
        sys.exit(1)
    # DEMETHIFY_CI_ROWS: what a row of confidence_interval_methylation_estimate.csv speaks about (bt_ci's profile_rows)
    ci_rows = os.environ.get("DEMETHIFY_CI_ROWS", "position")
    if ci_rows not in ("position", "cpg"):
        sys.stderr.write(f'Error: DEMETHIFY_CI_ROWS must be "position" or "cpg", got "{ci_rows}".\n')
        sys.exit(1)
    switched_on = {}  # the DEMETHIFY_BATCH* switches of BATCH_SWITCHES
    for switch in dict.fromkeys(row.switch for row in BATCH_SWITCHES):
        value = os.environ.get(switch, "0")
        if value not in ("0", "1"):
            sys.stderr.write(f'Error: {switch} must be "0" or "1", got "{value}".\n')
            sys.exit(1)
        switched_on[switch] = value == "1"
    if args.plot:
        sys.stderr.write("Note: --plot is ignored, plotting (seaborn/colorcet) is outside this build's scope.\n")

    # this rank's share of the sample files is parsed BEFORE the process group / the GPU come up: the parser's
    # worker pool is forked, and a fork must not start from a process that holds a HIP runtime and RCCL threads
    parsed = tables.parse_share(args.methfreq, bool(args.bedmethyl), bool(args.fillna))
    rank = _init_distributed()
    if not args.noprint and rank == 0:
        print(logo)
    outdir = os.path.join(os.getcwd(), args.outdir)
    if rank == 0 and not os.path.exists(outdir):
        print(f'Creating directory {outdir} to store results')
        os.mkdir(outdir)
    if args.nbunknown is None:
        args.nbunknown = [0]

    ref, header, meth_f, counts = read_inputs(args, parsed)
    del parsed
    args.methfreq = [name.split("/")[-1] for name in args.methfreq]

    # imported late so that ``--help`` and argument errors work on a box without the GPU library
    from . import _lib as L
    from . import shard, staging
    from . import batch
    from . import bootstrap as bootstrap_mod
    from . import ic as ic_mod
    from .bootstrap import bt_ci
    from . import init_func
    from .deconvolution import _init_guard, _init_unsupervised, init_BSSMF_md, init_BSSMF_md_p, rd, set_seed
    from .device import Problem, Solver, get_context
    from .ic import evaluate_best_ic
    from .init_func import wls_intercept

    time_start = time()
    gate_modules = {"bootstrap": bootstrap_mod, "ic": ic_mod}
    n_u = args.nbunknown[0]
    ic_n_u = None

    def batch_route(applies, what, align=False, profile_rows="position"):
        """The first row of BATCH_SWITCHES for `applies` whose switch is on and which takes `what`, or None for the per-solve
        path; every switch that is on and refuses says why in a one-line note."""
        n_rows, n_samples = meth_f.shape
        rows = [row for row in BATCH_SWITCHES if row.applies == applies and switched_on[row.switch]]
        for row in rows:
            if args.purity and row.purity == "refused" and any(other.purity == "only" for other in rows):
                continue
            if not args.purity and row.purity == "only":
                continue
            module = gate_modules[row.module]
            if row.criteria is not None:
                reason = None
                if args.ic not in getattr(module, row.criteria):
                    reason = f"{args.ic} was not measured faster through {batch.family(row.family).called} (ic.{row.criteria})"
            else:
                reason = bootstrap_mod.batched_ineligible(
                    n_u, n_rows, n_samples, ref.shape[1] if args.ref else 0, args.init, args.purity,
                    L.DMF_MODE_PARTIAL if args.ref else L.DMF_MODE_UNSUPERVISED, None, align, profile_rows,
                    purity_batched=row.purity == "own gate", kernel=row.family, mid_purity=row.purity == "only")
            if reason is None:
                lo_name, hi_name = row.purity_gate if args.purity and row.purity_gate else row.gate
                lo, hi = None if lo_name is None else getattr(module, lo_name), getattr(module, hi_name)
                if lo is None and n_rows * n_samples > hi:
                    reason = f"{n_rows} x {n_samples} elements are more than {hi_name} = {hi}"
                elif lo is not None and not lo <= n_rows * n_samples <= hi:
                    reason = (f"{n_rows} x {n_samples} elements are outside [{lo_name}, {hi_name}] = [{lo}, {hi}]"
                              + (" (the gate is closed)" if lo > hi else ""))
            if reason is None:
                return row
            if rank == 0:
                print(f"Note: {row.switch}=1 is not used for {what}: {reason}; taking the per-solve path.")
        return None

    def batch_keywords(row):
        """What the route `row` adds to a bt_ci or evaluate_best_ic call: a keyword is passed only when its route is taken,
        so without the switches the call is what it was."""
        if row is None:
            return {}
        kw = {"batched": True} if row.family == "small" else {"batched": True, "batch_kernel": row.family}
        if row.purity_keyword and args.purity:
            kw[row.purity_keyword] = True
        return kw

    def bootstrap(anchor=None):
        row = batch_route("solves", "--confidence", align=not args.ref and n_u >= 2, profile_rows=ci_rows)
        bt_ci(args.confidence[0], args.confidence[1], n_u, meth_f, counts, ref, args.init, args.iterations[0],
              args.iterations[1], args.termination, header if args.ref else [], outdir, args.methfreq, args.purity,
              args.seed, materialize=False, anchor=anchor, profile_rows=ci_rows, **batch_keywords(row))

    if args.confidence and args.ref:
        bootstrap()
    elif args.confidence and n_u < 1:
        sys.exit(f'Invalid number of unknown value! : "{args.nbunknown}" ')

    if args.ic:
        ic_kw = batch_keywords(batch_route("--ic", "--ic"))
        ref_estimate, proportions, ic_n_u, _scores = evaluate_best_ic(
            meth_f, ref, counts, args.init, args.ic, args.seed, iter1=args.iterations[0], iter2=args.iterations[1],
            tol=args.termination, n_restarts=nb_r, n_u_values=ic_range, **ic_kw)
        unknown_header = ["unknown_cell_" + str(i + 1) for i in range(ic_n_u)]
        header = header + unknown_header
    elif (not args.ref) or (n_u > 0 and meth_f.shape[1] >= 1):
        if not args.ref and n_u < 1:
            sys.exit(f'Invalid number of unknown value! : "{args.nbunknown}" ')
        unsupervised = not args.ref
        K = (0 if unsupervised else ref.shape[1]) + n_u
        if args.restart > 1 and rank == 0:
            print(f"restart k > 0 uses seed + k (upstream repeats the same seed); {args.restart} restarts")
        restarts_row = batch_route("solves", "--restart") if args.restart > 1 else None
        with Problem(get_context(), meth_f, counts, None if unsupervised else ref) as problem:
            if args.restart > 1 and restarts_row is None:
                staging.reserve(((meth_f.shape[0], n_u), (K, meth_f.shape[1])), count=2)

            # --init uniform on a large problem: u0 is drawn on the host as init_BSSMF_md / init_BSSMF_md_p draw it (set_seed,
            # then rd.uniform: the same stream), alpha0 = wls_intercept per sample comes from the device, where the problem
            # already is (solve_one: the context is not to be used from the worker thread)
            device_init = (not unsupervised and args.init == "uniform" and n_u <= meth_f.shape[1]
                           and init_func.device_wls(meth_f.shape[0], meth_f.shape[1], K))

            def draw_init(seed_k):
                if unsupervised:
                    return _init_unsupervised(args.init, meth_f, n_u, seed_k)
                if purity is not None:
                    u0, _, a0 = init_BSSMF_md_p(args.init, meth_f, counts, ref, n_u, purity, rb_alg=wls_intercept,
                                                seed=seed_k, _stack=False)
                else:
                    u0, _, a0 = init_BSSMF_md(args.init, meth_f, counts, ref, n_u, rb_alg=wls_intercept, seed=seed_k, _stack=False)
                return u0, a0

            def prepare(k):
                # the restart's initialisation (legacy-numpy draws, NNLS), drawn and uploaded one restart ahead of the
                # GPU by a worker thread (staging.Prefetcher)
                seed_k = shard.restart_seed(args.seed, k)
                if device_init:
                    set_seed(seed_k)
                    u0 = rd.uniform(size=(meth_f.shape[0], n_u))
                    return staging.to_device((u0,), problem.ctx)[0], u0
                u0, a0 = draw_init(seed_k)
                if args.restart > 1:
                    return staging.to_device((u0, a0), problem.ctx)
                return u0, a0

            def solve_one(k, best_cost, prepared):
                u0, a0 = prepared
                if device_init:
                    u0_host = a0
                    a0 = problem.wls_intercept(u0, "v", host_arrays=lambda: (meth_f, counts, np.c_[ref, u0_host]))
                    if purity is None:  # (init_BSSMF_md_p returns without the guard)
                        a0 = _init_guard(a0, n_u)
                    a0, = staging.to_device((a0,), problem.ctx)
                mode = L.DMF_MODE_UNSUPERVISED if unsupervised else L.DMF_MODE_PARTIAL
                s = Solver(problem, u0, a0, mode)
                try:
                    if purity is not None and not unsupervised:
                        s.set_purity(purity)
                    s.step(args.iterations[0], args.iterations[1], args.termination)
                    s.cost_begin()  # cost_f_w recomputed per restart (demethify.py:169,199): taken while the next one is set up
                except BaseException:
                    s.close()
                    raise
                return s

            def solve_end(s, best_cost):
                with s:
                    cost = s.cost_end()
                    if not cost < best_cost and args.restart > 1:
                        return None, None, cost  # cannot win (strict '<', demethify.py:170,200): stays on the device
                    u, alpha, _, _ = s.get()
                return u, alpha, cost

            def solve_batch(ks):
                # this rank's restarts through the batch of the route taken: the initialisers are drawn one after the other,
                # as prepare draws them
                def stack(part):
                    inits = [draw_init(shard.restart_seed(args.seed, k)) for k in part]
                    return np.stack([u0 for u0, _ in inits]), np.stack([a0 for _, a0 in inits]), None

                mode = L.DMF_MODE_UNSUPERVISED if unsupervised else L.DMF_MODE_PARTIAL
                return batch.solve_chunked(problem, batch.family(restarts_row.family), (*meth_f.shape, K - n_u, n_u), ks, stack,
                                           (mode, args.iterations[0], args.iterations[1], args.termination),
                                           purity=None if unsupervised else purity)[:3]

            shapes = ((meth_f.shape[0], n_u), (K, meth_f.shape[1]))
            if restarts_row is not None:
                ref_estimate, proportions, _best, _costs = shard.sharded_restarts_batched(args.restart, solve_batch, shapes)
            else:
                ref_estimate, proportions, _best, _costs = shard.sharded_restarts(
                    args.restart, solve_one, shapes, prepare=prepare, solve_end=solve_end)
        unknown_header = ["unknown_cell_" + str(i + 1) for i in range(n_u)]
        header = unknown_header if unsupervised else header + unknown_header
    elif n_u == 0 and meth_f.shape[1] >= 1:
        ref_estimate = None
        if init_func.device_wls(meth_f.shape[0], meth_f.shape[1], ref.shape[1]):
            with Problem(get_context(), meth_f, counts, ref) as problem:
                proportions = problem.wls_intercept(None, "dv", host_arrays=(meth_f, counts, ref))
        else:
            proportions = np.concatenate(
                [wls_intercept(counts[:, k:k + 1] * meth_f[:, k:k + 1], counts[:, k:k + 1], ref)
                 for k in range(meth_f.shape[1])], axis=1)
    else:
        sys.exit(f'Invalid number of unknown value! : "{args.nbunknown}" ')

    if args.confidence and not args.ref:
        # no reference: the point estimate ran first and names the components -- the replicates' unknown types are matched
        # to ITS profiles, so the intervals speak about the rows celltypes_proportions.csv reports (and no solve runs twice)
        bootstrap(anchor=(ref_estimate, proportions))

    time_tot = time() - time_start

    if rank == 0:
        if ref_estimate is not None:
            pd.DataFrame(ref_estimate).to_csv(outdir + '/methylation_profile_estimate.csv', index=False,
                                              header=unknown_header)
        table = pd.DataFrame(proportions)
        table.index = header
        table.columns = args.methfreq
        table.index.name = "Cell types"
        table.to_csv(outdir + '/celltypes_proportions.csv', index=True)
        print("All demethified! Results in " + outdir)
        with open(os.path.join(outdir, 'log.log'), "w+") as f:
            f.write("Total execution time = " + str(time_tot) + " s" + '\n')
            if args.ic:
                f.write("Number of unknowns that minimises " + args.ic + " : " + str(ic_n_u))


if __name__ == "__main__":
    main()
