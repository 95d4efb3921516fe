#!/usr/bin/env python3
"""Small problems: many solves per launch (Problem.solve_many, one workgroup per solve) against one solve at a time.

   python tools/small_batch_bench.py per-solve|batched [repetition]     one timing of every case on one leg
   python tools/small_batch_bench.py envelope                           one outer iteration at the envelope's largest shapes
   python tools/small_batch_bench.py purity-per-solve|purity-batched [repetition [case]]   the --purity legs (below)

Cases (tol 1e-2, 20 inner steps, initialiser uniform_):
  toy bt_ci 2500      bt_ci(95, 2500) on the reference's 350 x 10 example, 5 + 1 cell types
  toy restart 64      64 restarts of the same problem, the command line's restart loop
  1000x16 restart 64  synthetic_problem(1000, 16, 6, 2), 64 restarts, at most 200 outer iterations
  10000x64 restart 64 synthetic_problem(10000, 64, 12, 4), 64 restarts, at most 200 outer iterations
The per-solve leg is the command line's own loop (initialisers drawn and uploaded one restart ahead by a worker thread, the
streaming cost taken while the next restart is set up) and uses nothing this path added, so the same file runs on a
checkout of the commit before it; the batched leg draws the same initialisers and makes one solve_many call per chunk.
Run the legs in turn, five times each, append the output to one file and read it with tools/ab_median.py: every timing is
a line "launch <repetition>: <ms> ms" under its "== <case> | <leg>" heading.  A timing is a host clock around work that
ends in a device synchronise (every call here returns host arrays).

The --purity legs (purity-constrained solves, Frank-Wolfe alpha phase; tol 1e-2, the command line's 100 x 500 iterations):
  purity toy restart 64      64 restarts of the toy with purity 1 - P / 100, P the README example's --purity list
  purity 1000x16 restart 64  synthetic_problem(1000, 16, 6, 2), purity RandomState(5).uniform(0.05, 0.95, 16), 64 restarts
  purity toy bt_ci 2500      bt_ci(95, 2500) on the toy with purity P (bt_ci uses P / 100)
purity-per-solve uses only what the per-solve path had before the batched purity kernel (Solver.set_purity, bt_ci with a
purity list), so it runs on a checkout of the commit before it; purity-batched is solve_many(purity=...) and
bt_ci(batched=True, batched_purity=True).  A third argument keeps the cases whose name contains it.  `envelope` times the
purity variant too, with 500 inner steps."""
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np

from conftest import load_toy
from demethify_amd import _lib as L
from demethify_amd import shard, staging
from demethify_amd.bootstrap import bt_ci
from demethify_amd.deconvolution import init_BSSMF_md, init_BSSMF_md_p
from demethify_amd.device import Problem, Solver, get_context
from oracle.solver import synthetic_problem

TOL, T2 = 1e-2, 20
PURITY_ITERS = (100, 500)  # the command line's default with --purity
P = [60.0, 80.0, 90.0, 20.0, 50.0, 90.0, 100.0, 30.0, 50.0, 10.0]


def restarts_per_solve(problem, V, D, Rt, n_u, n_restarts, n_iter1):
    """demethify.main's restart loop (prepare / solve_one / solve_end through shard.sharded_restarts)."""
    K = Rt.shape[1] + n_u

    def prepare(k):
        u0, _, a0 = init_BSSMF_md("uniform_", V, D, Rt, n_u, seed=shard.restart_seed(1, k), _stack=False)
        return staging.to_device((u0, a0), problem.ctx)

    def solve_one(k, best_cost, prepared):
        s = Solver(problem, prepared[0], prepared[1], L.DMF_MODE_PARTIAL)
        try:
            s.step(n_iter1, T2, TOL)
            s.cost_begin()
        except BaseException:
            s.close()
            raise
        return s

    def solve_end(s, best_cost):
        with s:
            cost = s.cost_end()
            if not cost < best_cost:
                return None, None, cost
            u, alpha, _, _ = s.get()
        return u, alpha, cost

    staging.reserve(((V.shape[0], n_u), (K, V.shape[1])), count=2)
    return shard.sharded_restarts(n_restarts, solve_one, ((V.shape[0], n_u), (K, V.shape[1])), prepare=prepare,
                                  solve_end=solve_end)


def restarts_batched(problem, V, D, Rt, n_u, n_restarts, n_iter1):
    from demethify_amd.bootstrap import batch_chunk

    def solve_batch(ks):
        chunk = batch_chunk(V.shape[0], n_u)
        parts = []
        for c0 in range(0, len(ks), chunk):
            inits = [init_BSSMF_md("uniform_", V, D, Rt, n_u, seed=shard.restart_seed(1, k), _stack=False) for k in ks[c0:c0 + chunk]]
            parts.append(problem.solve_many(np.stack([i[0] for i in inits]), np.stack([i[2] for i in inits]), L.DMF_MODE_PARTIAL,
                                            n_iter1, T2, TOL)[:3])
        return tuple(np.concatenate([part[j] for part in parts]) for j in range(3))

    K = Rt.shape[1] + n_u
    return shard.sharded_restarts_batched(n_restarts, solve_batch, ((V.shape[0], n_u), (K, V.shape[1])))


def purity_restarts_per_solve(problem, V, D, Rt, n_u, purity, n_restarts):
    """demethify.main's restart loop under --purity: init_BSSMF_md_p, Solver.set_purity."""
    K = Rt.shape[1] + n_u
    shapes = ((V.shape[0], n_u), (K, V.shape[1]))

    def prepare(k):
        u0, _, a0 = init_BSSMF_md_p("uniform_", V, D, Rt, n_u, purity, seed=shard.restart_seed(1, k), _stack=False)
        return staging.to_device((u0, a0), problem.ctx)

    def solve_one(k, best_cost, prepared):
        s = Solver(problem, prepared[0], prepared[1], L.DMF_MODE_PARTIAL)
        try:
            s.set_purity(purity)
            s.step(PURITY_ITERS[0], PURITY_ITERS[1], TOL)
            s.cost_begin()
        except BaseException:
            s.close()
            raise
        return s

    def solve_end(s, best_cost):
        with s:
            cost = s.cost_end()
            if not cost < best_cost:
                return None, None, cost
            u, alpha, _, _ = s.get()
        return u, alpha, cost

    staging.reserve(shapes, count=2)
    return shard.sharded_restarts(n_restarts, solve_one, shapes, prepare=prepare, solve_end=solve_end)


def purity_restarts_batched(problem, V, D, Rt, n_u, purity, n_restarts):
    from demethify_amd.bootstrap import batch_chunk

    def solve_batch(ks):
        chunk = batch_chunk(V.shape[0], n_u)
        parts = []
        for c0 in range(0, len(ks), chunk):
            inits = [init_BSSMF_md_p("uniform_", V, D, Rt, n_u, purity, seed=shard.restart_seed(1, k), _stack=False)
                     for k in ks[c0:c0 + chunk]]
            parts.append(problem.solve_many(np.stack([i[0] for i in inits]), np.stack([i[2] for i in inits]), L.DMF_MODE_PARTIAL,
                                            PURITY_ITERS[0], PURITY_ITERS[1], TOL, purity=purity)[:3])
        return tuple(np.concatenate([part[j] for part in parts]) for j in range(3))

    K = Rt.shape[1] + n_u
    return shard.sharded_restarts_batched(n_restarts, solve_batch, ((V.shape[0], n_u), (K, V.shape[1])))


def run_purity_legs(leg, repetition, only=""):
    batched = leg == "purity-batched"
    toy = load_toy()
    ctx = get_context()
    samples = [f"s{i}" for i in range(10)]

    def toy_bt_ci(n):
        V, D, ref, header = toy
        with tempfile.TemporaryDirectory() as d:
            kw = {"batched": True, "batched_purity": True} if batched else {}
            out = bt_ci(95, n, 1, V, D, ref, "uniform_", PURITY_ITERS[0], PURITY_ITERS[1], TOL, header, d, samples, list(P), 1,
                        materialize=False, **kw)
        return float(np.sum(out[1][0]))

    def restart_case(V, D, Rt, n_u, purity, n_restarts):
        with Problem(ctx, V, D, Rt) as p:
            fn = purity_restarts_batched if batched else purity_restarts_per_solve
            _, _, best, costs = fn(p, V, D, Rt, n_u, purity, n_restarts)
        return float(costs[best])

    toy_purity = 1 - np.array(P) / 100
    V, D, Rt = synthetic_problem(1000, 16, 6, 2, seed=5, depth=30)
    purity16 = np.random.RandomState(5).uniform(0.05, 0.95, 16)
    cases = [("purity toy restart 64", lambda: restart_case(toy[0], toy[1], toy[2], 1, toy_purity, 64),
              lambda: restart_case(toy[0], toy[1], toy[2], 1, toy_purity, 2)),
             ("purity 1000x16 restart 64", lambda: restart_case(V, D, Rt, 2, purity16, 64),
              lambda: restart_case(V, D, Rt, 2, purity16, 2)),
             ("purity toy bt_ci 2500", lambda: toy_bt_ci(2500), lambda: toy_bt_ci(8))]
    for name, timed, warm in cases:
        if only not in name:
            continue
        warm()  # code objects, pools, pinned buffers
        ctx.synchronize()
        t0 = time.perf_counter()
        check = timed()
        ms = (time.perf_counter() - t0) * 1e3
        print(f"== {name} | {leg}")
        print(f"launch {repetition}: {ms:.3f} ms   (check {check:.9e})", flush=True)


def run_legs(leg, repetition):
    batched = leg == "batched"
    toy = load_toy()
    ctx = get_context()
    samples = [f"s{i}" for i in range(10)]

    def toy_bt_ci(n):
        V, D, ref, header = toy
        with tempfile.TemporaryDirectory() as d:
            kw = {"batched": True} if batched else {}
            out = bt_ci(95, n, 1, V, D, ref, "uniform_", 10000, T2, TOL, header, d, samples, None, 1, materialize=False, **kw)
        return float(np.sum(out[1][0]))

    def restart_case(V, D, Rt, n_u, n_restarts, n_iter1):
        with Problem(ctx, V, D, Rt) as p:
            fn = restarts_batched if batched else restarts_per_solve
            _, _, best, costs = fn(p, V, D, Rt, n_u, n_restarts, n_iter1)
        return float(costs[best])

    cases = [("toy bt_ci 2500", lambda: toy_bt_ci(2500), lambda: toy_bt_ci(8)),
             ("toy restart 64", lambda: restart_case(toy[0], toy[1], toy[2], 1, 64, 10000),
              lambda: restart_case(toy[0], toy[1], toy[2], 1, 2, 10000))]
    for N, S, n_c, n_u in ((1000, 16, 6, 2), (10000, 64, 12, 4)):
        V, D, Rt = synthetic_problem(N, S, n_c, n_u, seed=5, depth=30)
        cases.append((f"{N}x{S} restart 64", lambda a=(V, D, Rt, n_u): restart_case(*a, 64, 200),
                      lambda a=(V, D, Rt, n_u): restart_case(*a, 2, 3)))
    for name, timed, warm in cases:
        warm()  # code objects, pools, pinned buffers
        ctx.synchronize()
        t0 = time.perf_counter()
        check = timed()
        ms = (time.perf_counter() - t0) * 1e3
        print(f"== {name} | {leg}")
        print(f"launch {repetition}: {ms:.3f} ms   (check {check:.9e})", flush=True)


def envelope():
    """Device time of one outer iteration at the envelope's largest shapes (N S = 2^20, K = 16, n_u = 4, 20 inner steps):
    a solve_many call of 8 outer iterations in ONE launch minus a call of none (set-up only), alone and with every CU busy."""
    ctx = get_context()
    for N, S in ((16384, 64), (1 << 20, 1)):
        V, D, Rt = synthetic_problem(N, S, 12, 4, seed=3, depth=30)
        u0, _, a0 = init_BSSMF_md("uniform_", V, D, Rt, 4, seed=1, _stack=False)
        with Problem(ctx, V, D, Rt) as p:
            for B in (1, 256 if S == 64 else 16):
                u0s, a0s = np.repeat(u0[None], B, 0), np.repeat(a0[None], B, 0)
                times = {}
                for n1 in (0, 8, 0, 8, 0, 8):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    p.solve_many(u0s, a0s, L.DMF_MODE_PARTIAL, n1, T2, 0.0, iters_per_launch=8)
                    times.setdefault(n1, []).append((time.perf_counter() - t0) * 1e3)
                per_iter = (min(times[8]) - min(times[0])) / 8
                print(f"envelope {N} x {S}, 12 + 4 types, B = {B}: set-up call {min(times[0]):.2f} ms, 8 iterations "
                      f"{min(times[8]):.2f} ms -> {per_iter:.3f} ms per outer iteration", flush=True)
            # the purity variant with the command line's 500 inner steps: 2 outer iterations in one launch minus none
            purity = np.random.RandomState(5).uniform(0.05, 0.95, S)
            for B in (1, 256 if S == 64 else 16):
                u0s, a0s = np.repeat(u0[None], B, 0), np.repeat(a0[None], B, 0)
                times = {}
                for n1 in (0, 2, 0, 2, 0, 2):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    p.solve_many(u0s, a0s, L.DMF_MODE_PARTIAL, n1, PURITY_ITERS[1], 0.0, iters_per_launch=2, purity=purity)
                    times.setdefault(n1, []).append((time.perf_counter() - t0) * 1e3)
                per_iter = (min(times[2]) - min(times[0])) / 2
                print(f"envelope purity {N} x {S}, 12 + 4 types, {PURITY_ITERS[1]} inner steps, B = {B}: set-up call "
                      f"{min(times[0]):.2f} ms, 2 iterations {min(times[2]):.2f} ms -> {per_iter:.3f} ms per outer iteration",
                      flush=True)


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] not in ("per-solve", "batched", "envelope", "purity-per-solve", "purity-batched"):
        sys.exit(__doc__)
    if sys.argv[1] == "envelope":
        envelope()
    elif sys.argv[1].startswith("purity-"):
        run_purity_legs(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 0, sys.argv[3] if len(sys.argv) > 3 else "")
    else:
        run_legs(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 0)
