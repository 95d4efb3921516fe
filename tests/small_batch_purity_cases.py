"""The cases of the batched purity-constrained solve (Problem.solve_many(purity=...) / dmf_solve_small_purity), shared by
tests/test_small_batch_purity_host.py (no GPU: the preconditions) and tests/test_gpu_small_batch_purity.py (the device
against these runs).  Every reference here is oracle/solver.py's f64 trajectory (solve_partial_purity), computed once per
process and handed out read-only.

Preconditions of a case, asserted before the device is asked and never skipped:
  * natural stops: no stop test is decided by less than MIN_MARGIN tol (stop_margin of tests/test_gpu_small_batch.py);
  * every Frank-Wolfe argmin is decided by at least GAP, relative (GAP of tests/test_gpu_purity.py, whose docstring says
    why 1e-9 is the smallest gap the device's G a - b gradient can be held to)."""
import functools
from collections import namedtuple

import numpy as np

from oracle import solver as osol

from conftest import load_toy
from test_gpu_purity import GAP
from test_gpu_small_batch import COST_RTOL, MIN_MARGIN, TIGHT, stop_margin

__all__ = ["GAP", "COST_RTOL", "MIN_MARGIN", "TIGHT", "TOL", "P", "EDGES", "Run", "toy_restarts", "toy_replicates", "edge_runs",
           "edge_purity", "qualifies", "check_preconditions"]

TOL = 1e-2
# the --purity list of the reference's README example (tests/golden/upstream/purity), in percent
P = np.array([60.0, 80.0, 90.0, 20.0, 50.0, 90.0, 100.0, 30.0, 50.0, 10.0])
P.setflags(write=False)

# (N, S, n_c, n_u, n_iter2): tol 0, three outer iterations, seeds 1..3 on synthetic_problem(seed=11, depth=30)
EDGES = [(64, 1, 1, 1, 7), (257, 3, 2, 1, 20), (65, 64, 1, 4, 2), (777, 33, 3, 3, 50), (2049, 17, 15, 1, 1),
         (1000, 64, 12, 4, 20), (300, 5, 1, 2, 500)]
EDGE_ITERS, EDGE_SEEDS = 3, (1, 2, 3)

# u0, a0: the starting point; u, alpha: the oracle's result; trace: cost after every outer iteration; cf_start: the cost of
# the starting point; gap: the smallest relative argmin gap over the whole solve (+inf where every block has one row)
Run = namedtuple("Run", "u0 a0 u alpha trace cf_start gap")


def _run(V, D, Rt, n_u, purity, seed, n_iter1, n_iter2, tol):
    u0, R, a0 = osol.init_partial_purity("uniform_", V, D, Rt, n_u, purity, seed=seed)
    trace, gaps = [], []
    cf_start = osol.weighted_cost(V, R, a0, D)
    u, alpha = osol.solve_partial_purity(u0.copy(), R, a0.copy(), V, D, Rt, n_u, purity, n_iter1, n_iter2, tol, trace=trace,
                                         gaps=gaps)
    for x in (u0, a0, u, alpha):
        x.setflags(write=False)
    return Run(u0, a0, u, alpha, trace, cf_start, min(gaps))


@functools.lru_cache(maxsize=None)
def toy_restarts():
    """The oracle's 16 purity restarts of the toy: seeds 1..16, purity 1 - P / 100 (what the command line passes to the point
    estimate), 100 x 500, tol 1e-2."""
    V, D, ref, _ = load_toy()
    return tuple(_run(V, D, ref, 1, 1 - P / 100, seed, 100, 500, TOL) for seed in range(1, 17))


@functools.lru_cache(maxsize=None)
def toy_replicates(n_iter2):
    """24 bootstrap replicates of the toy from seed 1 with purity P / 100 (what bt_ci uses; the sample at 1.0 has an unknown
    block of mass 0), 100 x n_iter2, tol 1e-2: this module's own loop over bootstrap_seeds / bootstrap_indices on
    V[idx], D[idx], ref[idx] -> (idx (24, N), runs)."""
    V, D, ref, _ = load_toy()
    seeds = osol.bootstrap_seeds(1, 24)
    idx = np.stack([osol.bootstrap_indices(s, V.shape[0]) for s in seeds])
    idx.setflags(write=False)
    runs = tuple(_run(V[i], D[i], ref[i], 1, P / 100, s, 100, n_iter2, TOL) for s, i in zip(seeds, idx))
    return idx, runs


def edge_purity(S):
    return np.random.RandomState(5).uniform(0.05, 0.95, S)


@functools.lru_cache(maxsize=None)
def edge_runs(N, S, n_c, n_u, n_iter2):
    """-> ((V, D, Rt), purity, runs) of one edge shape."""
    V, D, Rt = osol.synthetic_problem(N, S, n_c, n_u, seed=11, depth=30)
    purity = edge_purity(S)
    for x in (V, D, Rt, purity):
        x.setflags(write=False)
    return (V, D, Rt), purity, tuple(_run(V, D, Rt, n_u, purity, seed, EDGE_ITERS, n_iter2, 0.0) for seed in EDGE_SEEDS)


def qualifies(run, tol=TOL):
    """Both preconditions of a natural-stop run."""
    return stop_margin(run.cf_start, run.trace, tol) >= MIN_MARGIN and run.gap >= GAP


def check_preconditions(name, runs, tol):
    """Assert the preconditions of every run (the stop margin only where the stop is natural, tol > 0)."""
    for b, r in enumerate(runs):
        margin = stop_margin(r.cf_start, r.trace, tol) if tol > 0 else np.inf
        print(f"{name}[{b}]: oracle stops after {len(r.trace)}, stop margin {margin:.2e}, smallest argmin gap {r.gap:.2e}")
        assert margin >= MIN_MARGIN
        assert r.gap >= GAP
