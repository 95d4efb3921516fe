#!/usr/bin/env python3
"""Purity-constrained solves of mid-size problems: many per call with several workgroups per solve
(Problem.solve_many_mid(purity=...)) against one solve at a time and against the one-launch batch
(Problem.solve_many(purity=...), one workgroup per solve).

   python tools/mid_batch_purity_bench.py per-solve|small|mid [repetition [case]]   one timing of every case on one leg
   python tools/mid_batch_purity_bench.py run PARENT OUT [first [last [case]]]      the legs in turn, repetitions first..last
   python tools/mid_batch_purity_bench.py summary FILE                              medians and validity of such output
   python tools/mid_batch_purity_bench.py events [case]                             event times of the mid leg's launches

Cases (100 x 500 iterations, tol 1e-2, initialiser uniform_, purities RandomState(5).uniform(0.05, 0.95, S)):
  1000x16 restart 64     synthetic_problem(1000, 16, 6, 2), 64 restarts
  4000x16 restart 64     synthetic_problem(4000, 16, 6, 2), 64 restarts
  10000x64 restart 64    synthetic_problem(10000, 64, 12, 4), 64 restarts
  32768x64 restart 64    synthetic_problem(32768, 64, 12, 4), 64 restarts
  10000x64 bt_ci 500     bt_ci(95, 500) on synthetic_problem(10000, 64, 6, 2)
Legs: `per-solve` is the command line's own restart loop with --purity (initialisers drawn and uploaded one restart ahead by
a worker thread, Solver.set_purity, the streaming cost taken while the next restart is set up) and plain bt_ci; it uses
nothing the mid-size purity batch added, so the same file runs on a checkout of the commit before it -- which is where it is
meant to run.  `small` draws the same initialisers and goes through solve_many(purity=...) /
bt_ci(batched=True, batched_purity=True); a case outside that kernel's envelope is skipped.  `mid` goes through
solve_many_mid(purity=...) / bt_ci(batched=True, batch_kernel="mid", batched_mid_purity=True).

Method: `run` takes the legs in turn, one process each (the per-solve leg with PARENT/tools/<this file>, a copy of this file
in a checkout of the parent commit with its library built), once per repetition, and appends the output to OUT; every
process runs under a time limit of its own, and the first one that fails or runs out of time ends the run.  Five
repetitions, then `summary`.  A timing is a host clock around work that ends in a device synchronise (every call returns
host arrays), after a warm-up of the same code on two restarts (eight replicates).  Every timing is a line
"launch <repetition>: <ms> ms   (check <value>)" under its "== <case> | <leg>" heading; the check is the winning cost of the
restarts (for bt_ci: the sum of the lower profile bounds).  `summary` prints per case the median of each leg and marks the
case INVALID unless every timing of every leg shows the same check to ten digits.

`events` runs the mid leg's 64 restarts of one case (default 10000x64) launch by launch, as dmf_solve_mid_purity enqueues
them, under `rocprofv3 --kernel-trace --stats` -- run it as
   rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mid_batch_purity_bench.py events
and read k_mid_rows against k_mid_alpha_fw in the kernel statistics."""
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

TOL, T1, T2 = 1e-2, 100, 500
RESTART_SHAPES = ((1000, 16, 6, 2), (4000, 16, 6, 2), (10000, 64, 12, 4), (32768, 64, 12, 4))
LEGS = ("per-solve", "small", "mid")
LEG_SECONDS = 900  # the time limit of one leg's process


def purities(S):
    import numpy as np

    return np.random.RandomState(5).uniform(0.05, 0.95, S)


def run_legs(leg, repetition, only=""):
    import numpy as np

    from demethify_amd import _lib as L
    from demethify_amd import bootstrap, shard, staging
    from demethify_amd.bootstrap import bt_ci
    from demethify_amd.deconvolution import init_BSSMF_md_p
    from demethify_amd.device import Problem, Solver, get_context, small_solve_supported
    from oracle.solver import synthetic_problem

    ctx = get_context()

    def restarts_per_solve(problem, V, D, Rt, n_u, purity, n_restarts, n_iter1):
        """demethify.main's restart loop with --purity (prepare / solve_one / solve_end through shard.sharded_restarts)."""
        shapes = ((V.shape[0], n_u), (Rt.shape[1] + n_u, V.shape[1]))

        def prepare(k):
            u0, _, a0 = init_BSSMF_md_p("uniform_", V, D, Rt, n_u, purity, seed=shard.restart_seed(1, k), _stack=False)
            return staging.to_device((u0, a0), problem.ctx)

        def solve_one(k, best_cost, prepared):
            s = Solver(problem, prepared[0], prepared[1], L.DMF_MODE_PARTIAL)
            try:
                s.set_purity(purity)
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

        staging.reserve(shapes, count=2)
        return shard.sharded_restarts(n_restarts, solve_one, shapes, prepare=prepare, solve_end=solve_end)

    def restarts_batched(problem, V, D, Rt, n_u, purity, n_restarts, n_iter1):
        mid = leg == "mid"
        if mid:
            chunk = bootstrap.mid_batch_chunk(V.shape[0], V.shape[1], Rt.shape[1], n_u)
        else:
            chunk = bootstrap.batch_chunk(V.shape[0], n_u)
        solve = problem.solve_many_mid if mid else problem.solve_many

        def solve_batch(ks):
            parts = []
            for c0 in range(0, len(ks), chunk):
                inits = [init_BSSMF_md_p("uniform_", V, D, Rt, n_u, purity, seed=shard.restart_seed(1, k), _stack=False)
                         for k in ks[c0:c0 + chunk]]
                parts.append(solve(np.stack([i[0] for i in inits]), np.stack([i[2] for i in inits]), L.DMF_MODE_PARTIAL,
                                   n_iter1, T2, TOL, purity=purity)[:3])
            return tuple(np.concatenate([part[j] for part in parts]) for j in range(3))

        return shard.sharded_restarts_batched(n_restarts, solve_batch, ((V.shape[0], n_u), (Rt.shape[1] + n_u, V.shape[1])))

    def restart_case(V, D, Rt, n_u, n_restarts, n_iter1):
        with Problem(ctx, V, D, Rt) as p:
            fn = restarts_per_solve if leg == "per-solve" else restarts_batched
            _, _, best, costs = fn(p, V, D, Rt, n_u, purities(V.shape[1]), n_restarts, n_iter1)
        return float(costs[best])

    def bt_ci_case(V, D, Rt, n_u, n):
        kw = {"per-solve": {}, "small": {"batched": True, "batched_purity": True},
              "mid": {"batched": True, "batch_kernel": "mid", "batched_mid_purity": True}}[leg]
        with tempfile.TemporaryDirectory() as d:
            out = bt_ci(95, n, n_u, V, D, Rt, "uniform_", T1, T2, TOL, [f"c{k}" for k in range(Rt.shape[1])], d,
                        [f"s{i}" for i in range(V.shape[1])], list(100 * purities(V.shape[1])), 1, materialize=False, **kw)
        return float(np.sum(out[1][0]))

    cases = []
    for N, S, n_c, n_u in RESTART_SHAPES:
        name = f"{N}x{S} restart 64"
        if only not in name or (leg == "small" and not small_solve_supported(N, S, n_c, n_u, L.DMF_MODE_PARTIAL)):
            continue
        a = synthetic_problem(N, S, n_c, n_u, seed=5, depth=30) + (n_u,)
        cases.append((name, lambda a=a: restart_case(*a, 64, T1), lambda a=a: restart_case(*a, 2, 3)))
    if only in "10000x64 bt_ci 500":
        b = synthetic_problem(10000, 64, 6, 2, seed=5, depth=30) + (2,)
        cases.append(("10000x64 bt_ci 500", lambda: bt_ci_case(*b, 500), lambda: bt_ci_case(*b, 8)))
    for name, timed, warm in cases:
        warm()  # code objects, pools, pinned buffers
        ctx.synchronize()
        t0 = time.perf_counter()
        check = timed()
        ms = (time.perf_counter() - t0) * 1e3
        print(f"== {name} | {leg}")
        print(f"launch {repetition}: {ms:.3f} ms   (check {check:.9e})", flush=True)


def events(only):
    """The mid leg's 64 restarts of one restart case, once after a warm-up, for a kernel trace to look at."""
    import numpy as np

    from demethify_amd import _lib as L
    from demethify_amd.deconvolution import init_BSSMF_md_p
    from demethify_amd.device import Problem, get_context
    from oracle.solver import synthetic_problem

    N, S, n_c, n_u = next(s for s in RESTART_SHAPES if only in f"{s[0]}x{s[1]}")
    V, D, Rt = synthetic_problem(N, S, n_c, n_u, seed=5, depth=30)
    purity = purities(S)
    inits = [init_BSSMF_md_p("uniform_", V, D, Rt, n_u, purity, seed=k + 1, _stack=False) for k in range(64)]
    u0s, a0s = np.stack([i[0] for i in inits]), np.stack([i[2] for i in inits])
    with Problem(get_context(), V, D, Rt) as p:
        p.solve_many_mid(u0s[:2], a0s[:2], L.DMF_MODE_PARTIAL, 3, T2, TOL, purity=purity)
        t0 = time.perf_counter()
        _, _, cost, iters = p.solve_many_mid(u0s, a0s, L.DMF_MODE_PARTIAL, T1, T2, TOL, purity=purity)
        ms = (time.perf_counter() - t0) * 1e3
    print(f"{N}x{S} ({n_c}+{n_u}), 64 restarts through solve_many_mid(purity=...): {ms:.1f} ms, {int(iters.sum())} solve-iterations, "
          f"at most {int(iters.max())} outer iterations, winning cost {cost.min():.9e}")


def run(parent, out, first, last, only):
    """The three legs in turn for repetitions first..last, one process each under its own time limit; the first failure ends
    the run.  The per-solve leg is PARENT's copy of this file."""
    this = Path(__file__).resolve()
    theirs = Path(parent).resolve() / "tools" / this.name
    if not theirs.exists():
        sys.exit(f"{theirs} is missing: copy this file into the parent checkout's tools/ and build its library")
    with open(out, "a") as log:
        for repetition in range(first, last + 1):
            for leg in LEGS:
                script = theirs if leg == "per-solve" else this
                cmd = ["timeout", "-k", "10", str(LEG_SECONDS), sys.executable, str(script), leg, str(repetition), only]
                proc = subprocess.run(cmd, cwd=script.parent.parent, capture_output=True, text=True)
                log.write(proc.stdout)
                log.flush()
                print(proc.stdout, end="", flush=True)
                if proc.returncode != 0:
                    sys.stderr.write(proc.stderr[-4000:])
                    sys.exit(f"leg {leg}, repetition {repetition} ended with status {proc.returncode}: the run stops here")


def summary(path):
    import re
    import statistics

    times, checks, order = {}, {}, []
    head = None
    for line in Path(path).read_text().splitlines():
        m = re.match(r"== (.+) \| (.+)$", line)
        if m:
            head = (m.group(1), m.group(2))
            if head[0] not in order:
                order.append(head[0])
            continue
        m = re.match(r"launch \d+: ([0-9.]+) ms\s+\(check (\S+)\)", line)
        if m and head is not None:
            times.setdefault(head, []).append(float(m.group(1)))
            checks.setdefault(head[0], set()).add(m.group(2))
    for case in order:
        med = {leg: statistics.median(times[(case, leg)]) for leg in LEGS if (case, leg) in times}
        n = {leg: len(times[(case, leg)]) for leg in med}
        text = "   ".join(f"{leg} {med[leg]:.1f} ms (n = {n[leg]})" for leg in med)
        valid = len(checks[case]) == 1
        wins = valid and "mid" in med and all(med["mid"] < v for leg, v in med.items() if leg != "mid")
        print(f"{case}: {text}   {'valid, check ' + next(iter(checks[case])) if valid else 'INVALID: checks ' + ', '.join(sorted(checks[case]))}"
              f"   {'mid wins' if wins else 'mid does not win'}")


if __name__ == "__main__":
    argv = sys.argv
    if len(argv) >= 3 and argv[1] == "summary":
        summary(argv[2])
    elif len(argv) >= 4 and argv[1] == "run":
        run(argv[2], argv[3], int(argv[4]) if len(argv) > 4 else 1, int(argv[5]) if len(argv) > 5 else 5,
            argv[6] if len(argv) > 6 else "")
    elif len(argv) >= 2 and argv[1] == "events":
        events(argv[2] if len(argv) > 2 else "10000x64")
    elif len(argv) >= 2 and argv[1] in LEGS:
        run_legs(argv[1], int(argv[2]) if len(argv) > 2 else 0, argv[3] if len(argv) > 3 else "")
    else:
        sys.exit(__doc__)
