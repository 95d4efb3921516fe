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
    # DEMETHIFY_BATCH=1: bootstrap replicates and restarts of small problems through Problem.solve_many, where eligible
    batch_env = os.environ.get("DEMETHIFY_BATCH", "0")
    if batch_env not in ("0", "1"):
        sys.stderr.write(f'Error: DEMETHIFY_BATCH must be "0" or "1", got "{batch_env}".\n')
        sys.exit(1)
    # DEMETHIFY_BATCH_MID=1: where DEMETHIFY_BATCH's own route is not taken, replicates and restarts of mid-size problems go
    # through Problem.solve_many_mid (several workgroups per solve), where eligible
    batch_mid_env = os.environ.get("DEMETHIFY_BATCH_MID", "0")
    if batch_mid_env not in ("0", "1"):
        sys.stderr.write(f'Error: DEMETHIFY_BATCH_MID must be "0" or "1", got "{batch_mid_env}".\n')
        sys.exit(1)
    # DEMETHIFY_BATCH_MID_PURITY=1: where neither route above is taken, --purity replicates and restarts of mid-size problems go
    # through Problem.solve_many_mid(purity=...), where eligible and inside a gate of its own
    batch_mid_purity_env = os.environ.get("DEMETHIFY_BATCH_MID_PURITY", "0")
    if batch_mid_purity_env not in ("0", "1"):
        sys.stderr.write(f'Error: DEMETHIFY_BATCH_MID_PURITY must be "0" or "1", got "{batch_mid_purity_env}".\n')
        sys.exit(1)
    # DEMETHIFY_BATCH_MID_IC=1: where DEMETHIFY_BATCH's own --ic route is not taken, an --ic sweep of a mid-size problem goes
    # through evaluate_best_ic(batched=True, batch_kernel="mid"), for the measured criteria and inside a gate of its own
    batch_mid_ic_env = os.environ.get("DEMETHIFY_BATCH_MID_IC", "0")
    if batch_mid_ic_env not in ("0", "1"):
        sys.stderr.write(f'Error: DEMETHIFY_BATCH_MID_IC must be "0" or "1", got "{batch_mid_ic_env}".\n')
        sys.exit(1)
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
    from . import bootstrap as bootstrap_mod
    from .bootstrap import bt_ci
    from . import init_func
    from .deconvolution import _init_guard, _init_unsupervised, init_BSSMF_md, init_BSSMF_md_p, rd, set_seed
    from .device import Problem, Solver, get_context
    from .ic import evaluate_best_ic
    from .init_func import wls_intercept

    time_start = time()
    n_u = args.nbunknown[0]
    ic_n_u = None

    def batch_route(what, align=False, profile_rows="position"):
        """DEMETHIFY_BATCH=1: does `what` go through Problem.solve_many?  A one-line note says why not."""
        if batch_env != "1":
            return False
        n_rows, n_samples = meth_f.shape
        reason = bootstrap_mod.batched_ineligible(
            n_u, n_rows, n_samples, ref.shape[1] if args.ref else 0, args.init, args.purity,
            L.DMF_MODE_PARTIAL if args.ref else L.DMF_MODE_UNSUPERVISED, None, align, profile_rows, purity_batched=True)
        # (--purity has a gate of its own: its batched kernel was measured on its own)
        gate_name = "SMALL_BATCH_PURITY_MAX_ELEMENTS" if args.purity else "SMALL_BATCH_MAX_ELEMENTS"
        gate = getattr(bootstrap_mod, gate_name)
        if reason is None and n_rows * n_samples > gate:
            reason = f"{n_rows} x {n_samples} elements are more than {gate_name} = {gate}"
        if reason is not None and rank == 0:
            print(f"Note: DEMETHIFY_BATCH=1 is not used for {what}: {reason}; taking the per-solve path.")
        return reason is None

    def batch_mid_route(what, align=False, profile_rows="position"):
        """DEMETHIFY_BATCH_MID=1, asked after DEMETHIFY_BATCH's own route was not taken: does `what` go through
        Problem.solve_many_mid?  A one-line note says why not."""
        if batch_mid_env != "1" or (args.purity and batch_mid_purity_env == "1"):  # (the purity route speaks for itself)
            return False
        n_rows, n_samples = meth_f.shape
        reason = bootstrap_mod.batched_ineligible(
            n_u, n_rows, n_samples, ref.shape[1] if args.ref else 0, args.init, args.purity,
            L.DMF_MODE_PARTIAL if args.ref else L.DMF_MODE_UNSUPERVISED, None, align, profile_rows, kernel="mid")
        lo, hi = bootstrap_mod.MID_BATCH_MIN_ELEMENTS, bootstrap_mod.MID_BATCH_MAX_ELEMENTS
        if reason is None and not lo <= n_rows * n_samples <= hi:
            reason = (f"{n_rows} x {n_samples} elements are outside [MID_BATCH_MIN_ELEMENTS, MID_BATCH_MAX_ELEMENTS] = "
                      f"[{lo}, {hi}]" + (" (the gate is closed)" if lo > hi else ""))
        if reason is not None and rank == 0:
            print(f"Note: DEMETHIFY_BATCH_MID=1 is not used for {what}: {reason}; taking the per-solve path.")
        return reason is None

    def batch_mid_purity_route(what, align=False, profile_rows="position"):
        """DEMETHIFY_BATCH_MID_PURITY=1, asked last and for --purity runs only: does `what` go through
        Problem.solve_many_mid(purity=...)?  A one-line note says why not."""
        if batch_mid_purity_env != "1" or not args.purity:
            return False
        n_rows, n_samples = meth_f.shape
        reason = bootstrap_mod.batched_ineligible(
            n_u, n_rows, n_samples, ref.shape[1] if args.ref else 0, args.init, args.purity,
            L.DMF_MODE_PARTIAL if args.ref else L.DMF_MODE_UNSUPERVISED, None, align, profile_rows, kernel="mid", mid_purity=True)
        lo, hi = bootstrap_mod.MID_BATCH_PURITY_MIN_ELEMENTS, bootstrap_mod.MID_BATCH_PURITY_MAX_ELEMENTS
        if reason is None and not lo <= n_rows * n_samples <= hi:
            reason = (f"{n_rows} x {n_samples} elements are outside [MID_BATCH_PURITY_MIN_ELEMENTS, "
                      f"MID_BATCH_PURITY_MAX_ELEMENTS] = [{lo}, {hi}]" + (" (the gate is closed)" if lo > hi else ""))
        if reason is not None and rank == 0:
            print(f"Note: DEMETHIFY_BATCH_MID_PURITY=1 is not used for {what}: {reason}; taking the per-solve path.")
        return reason is None

    def bootstrap(anchor=None):
        align = not args.ref and n_u >= 2
        batched = batch_route("--confidence", align=align, profile_rows=ci_rows)
        if not batched and batch_mid_route("--confidence", align=align, profile_rows=ci_rows):
            bt_ci(args.confidence[0], args.confidence[1], n_u, meth_f, counts, ref, args.init, args.iterations[0],
                  args.iterations[1], args.termination, header if args.ref else [], outdir, args.methfreq, args.purity,
                  args.seed, materialize=False, anchor=anchor, profile_rows=ci_rows, batched=True, batch_kernel="mid")
            return
        if not batched and batch_mid_purity_route("--confidence", align=align, profile_rows=ci_rows):
            bt_ci(args.confidence[0], args.confidence[1], n_u, meth_f, counts, ref, args.init, args.iterations[0],
                  args.iterations[1], args.termination, header if args.ref else [], outdir, args.methfreq, args.purity,
                  args.seed, materialize=False, anchor=anchor, profile_rows=ci_rows, batched=True, batch_kernel="mid",
                  batched_mid_purity=True)
            return
        bt_ci(args.confidence[0], args.confidence[1], n_u, meth_f, counts, ref, args.init, args.iterations[0],
              args.iterations[1], args.termination, header if args.ref else [], outdir, args.methfreq, args.purity,
              args.seed, materialize=False, anchor=anchor, profile_rows=ci_rows, batched=batched,
              batched_purity=batched and bool(args.purity))

    if args.confidence and args.ref:
        bootstrap()
    elif args.confidence and n_u < 1:
        sys.exit(f'Invalid number of unknown value! : "{args.nbunknown}" ')

    def ic_batch_route():
        """DEMETHIFY_BATCH=1 with --ic: does the sweep go through evaluate_best_ic(batched=True)?  Candidates outside the
        kernel's envelope take the per-solve path inside it; the size gate is the measured one of ic.py."""
        if batch_env != "1":
            return False
        from . import ic as ic_mod

        reason = None
        if args.ic not in ic_mod.SMALL_BATCH_IC_CRITERIA:
            reason = f"{args.ic} was not measured faster through the batch (ic.SMALL_BATCH_IC_CRITERIA)"
        elif meth_f.size > ic_mod.SMALL_BATCH_IC_MAX_ELEMENTS:
            reason = (f"{meth_f.shape[0]} x {meth_f.shape[1]} elements are more than SMALL_BATCH_IC_MAX_ELEMENTS = "
                      f"{ic_mod.SMALL_BATCH_IC_MAX_ELEMENTS}")
        if reason is not None and rank == 0:
            print(f"Note: DEMETHIFY_BATCH=1 is not used for --ic: {reason}; taking the per-solve path.")
        return reason is None

    def ic_batch_mid_route():
        """DEMETHIFY_BATCH_MID_IC=1 with --ic, asked after DEMETHIFY_BATCH's own --ic route was not taken: does the sweep go
        through evaluate_best_ic(batched=True, batch_kernel="mid")?  Candidates outside the mid-size batch's envelope take
        the per-solve path inside it; the criteria and the size range are the measured ones of ic.py."""
        if batch_mid_ic_env != "1":
            return False
        from . import ic as ic_mod

        reason = None
        lo, hi = ic_mod.MID_BATCH_IC_MIN_ELEMENTS, ic_mod.MID_BATCH_IC_MAX_ELEMENTS
        if args.ic not in ic_mod.MID_BATCH_IC_CRITERIA:
            reason = f"{args.ic} was not measured faster through the mid-size batch (ic.MID_BATCH_IC_CRITERIA)"
        elif not lo <= meth_f.size <= hi:
            reason = (f"{meth_f.shape[0]} x {meth_f.shape[1]} elements are outside [MID_BATCH_IC_MIN_ELEMENTS, "
                      f"MID_BATCH_IC_MAX_ELEMENTS] = [{lo}, {hi}]" + (" (the gate is closed)" if lo > hi else ""))
        if reason is not None and rank == 0:
            print(f"Note: DEMETHIFY_BATCH_MID_IC=1 is not used for --ic: {reason}; taking the per-solve path.")
        return reason is None

    if args.ic:
        # (a keyword is passed only when its route is taken: without the switches the call is what it was)
        ic_kw = {"batched": True} if ic_batch_route() else {}
        if not ic_kw and ic_batch_mid_route():
            ic_kw = {"batched": True, "batch_kernel": "mid"}
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
        batch_restarts = args.restart > 1 and batch_route("--restart")
        mid_restarts = args.restart > 1 and not batch_restarts and (batch_mid_route("--restart")
                                                                    or batch_mid_purity_route("--restart"))
        with Problem(get_context(), meth_f, counts, None if unsupervised else ref) as problem:
            if args.restart > 1 and not batch_restarts and not mid_restarts:
                staging.reserve(((meth_f.shape[0], n_u), (K, meth_f.shape[1])), count=2)

            # --init uniform on a large problem: u0 is drawn on the host as init_BSSMF_md / init_BSSMF_md_p draw it (set_seed,
            # then rd.uniform: the same stream), alpha0 = wls_intercept per sample comes from the device, where the problem
            # already is (solve_one: the context is not to be used from the worker thread)
            device_init = (not unsupervised and args.init == "uniform" and n_u <= meth_f.shape[1]
                           and init_func.device_wls(meth_f.shape[0], meth_f.shape[1], K))

            def prepare(k):
                # the restart's initialisation (legacy-numpy draws, NNLS), drawn and uploaded one restart ahead of the
                # GPU by a worker thread (staging.Prefetcher)
                seed_k = shard.restart_seed(args.seed, k)
                if device_init:
                    set_seed(seed_k)
                    u0 = rd.uniform(size=(meth_f.shape[0], n_u))
                    return staging.to_device((u0,), problem.ctx)[0], u0
                if unsupervised:
                    u0, a0 = _init_unsupervised(args.init, meth_f, n_u, seed_k)
                elif purity is not None:
                    u0, _, a0 = init_BSSMF_md_p(args.init, meth_f, counts, ref, n_u, purity, rb_alg=wls_intercept,
                                                seed=seed_k, _stack=False)
                else:
                    u0, _, a0 = init_BSSMF_md(args.init, meth_f, counts, ref, n_u, rb_alg=wls_intercept, seed=seed_k, _stack=False)
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

            def solve_batch(ks, mid=False):
                # this rank's restarts, one workgroup each (mid: several each, Problem.solve_many_mid): the initialisers are
                # drawn one after the other, as prepare draws them
                mode = L.DMF_MODE_UNSUPERVISED if unsupervised else L.DMF_MODE_PARTIAL
                if mid:
                    chunk = bootstrap_mod.mid_batch_chunk(meth_f.shape[0], meth_f.shape[1], K - n_u, n_u)
                else:
                    chunk = bootstrap_mod.batch_chunk(meth_f.shape[0], n_u)
                parts = []
                for c0 in range(0, len(ks), chunk):
                    inits = []
                    for k in ks[c0:c0 + chunk]:
                        seed_k = shard.restart_seed(args.seed, k)
                        if unsupervised:
                            inits.append(_init_unsupervised(args.init, meth_f, n_u, seed_k))
                        elif purity is not None:
                            u0, _, a0 = init_BSSMF_md_p(args.init, meth_f, counts, ref, n_u, purity, rb_alg=wls_intercept,
                                                        seed=seed_k, _stack=False)
                            inits.append((u0, a0))
                        else:
                            u0, _, a0 = init_BSSMF_md(args.init, meth_f, counts, ref, n_u, rb_alg=wls_intercept, seed=seed_k,
                                                      _stack=False)
                            inits.append((u0, a0))
                    if mid:
                        # (a purity vector is passed only on the purity route: without it the call is what it was)
                        purity_kw = {} if unsupervised or purity is None else {"purity": purity}
                        parts.append(problem.solve_many_mid(np.stack([u0 for u0, _ in inits]), np.stack([a0 for _, a0 in inits]),
                                                            mode, args.iterations[0], args.iterations[1], args.termination,
                                                            **purity_kw)[:3])
                        continue
                    parts.append(problem.solve_many(np.stack([u0 for u0, _ in inits]), np.stack([a0 for _, a0 in inits]), mode,
                                                    args.iterations[0], args.iterations[1], args.termination,
                                                    purity=None if unsupervised else purity)[:3])
                return tuple(np.concatenate([part[j] for part in parts]) for j in range(3))

            shapes = ((meth_f.shape[0], n_u), (K, meth_f.shape[1]))
            if batch_restarts:
                ref_estimate, proportions, _best, _costs = shard.sharded_restarts_batched(args.restart, solve_batch, shapes)
            elif mid_restarts:
                ref_estimate, proportions, _best, _costs = shard.sharded_restarts_batched(
                    args.restart, lambda ks: solve_batch(ks, mid=True), shapes)
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
