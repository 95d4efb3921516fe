#!/usr/bin/env python3
"""Model-selection sweeps of small problems: evaluate_best_ic(batched=True) -- the restarts of CCC through
Problem.solve_many, the folds of BCV through Problem.solve_many_masked, AIC as a batch of one -- against one solve at a time.

   python tools/small_ic_bench.py per-solve|batched [repetition [case]]   one timing of every case on one leg
   python tools/small_ic_bench.py summary FILE                            medians per case and leg; the scores must agree

Cases (tol 1e-2, 20 inner steps, initialiser uniform_, seed 1, candidates n_u = 1..4):
  toy BCV 20 / toy CCC 20 / toy AIC     the reference's 350 x 10 example, 5 known types; 20 folds, 20 restarts, one solve
  1000x16 BCV 20 / 1000x16 CCC 20       synthetic_problem(1000, 16, 6, 2, seed=5, depth=30), at most 200 outer iterations
  10000x64 BCV 5                        synthetic_problem(10000, 64, 12, 4, seed=5, depth=30), at most 200 outer iterations
The per-solve leg calls evaluate_best_ic without the keyword and uses nothing the batched route added, so the same file runs
on a checkout of the commit before it (copy it there); the batched leg passes batched=True.  Run the legs in turn, five times
each, in processes of their own, append the output to one file and read it with `summary`: every timing is a line
"launch <repetition>: <ms> ms   (scores ...)" under its "== <case> | <leg>" heading, a host clock around a call that returns
host arrays (it ends in a device synchronise), after a warm-up call of the same case with three outer iterations.  `summary`
prints the medians and fails unless both legs return the same scores to ten digits.  A third argument keeps the cases
whose name contains it."""
import re
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

TOL, T2 = 1e-2, 20
CANDIDATES = (1, 2, 3, 4)


def run_leg(leg, repetition, only=""):
    import numpy as np

    from conftest import load_toy
    from demethify_amd.device import get_context
    from demethify_amd.ic import evaluate_best_ic
    from oracle.solver import synthetic_problem

    kw = {"batched": True} if leg == "batched" else {}
    ctx = get_context()
    toy = load_toy()
    mid = synthetic_problem(1000, 16, 6, 2, seed=5, depth=30)
    big = synthetic_problem(10000, 64, 12, 4, seed=5, depth=30)
    cases = [("toy BCV 20", toy[:3], "BCV", 20, 10000), ("toy CCC 20", toy[:3], "CCC", 20, 10000), ("toy AIC", toy[:3], "AIC", 1, 10000),
             ("1000x16 BCV 20", (mid[0], mid[1], mid[2]), "BCV", 20, 200), ("1000x16 CCC 20", (mid[0], mid[1], mid[2]), "CCC", 20, 200),
             ("10000x64 BCV 5", (big[0], big[1], big[2]), "BCV", 5, 200)]
    for name, (V, D, Rt), ic, n, n_iter1 in cases:
        if only not in name:
            continue
        evaluate_best_ic(V, Rt, D, "uniform_", ic, 1, 3, T2, TOL, n_restarts=n, n_u_values=CANDIDATES, **kw)  # warm-up
        ctx.synchronize()
        t0 = time.perf_counter()
        _, _, n_best, scores = evaluate_best_ic(V, Rt, D, "uniform_", ic, 1, n_iter1, T2, TOL, n_restarts=n, n_u_values=CANDIDATES, **kw)
        ms = (time.perf_counter() - t0) * 1e3
        print(f"== {name} | {leg}")
        print(f"launch {repetition}: {ms:.3f} ms   (scores {' '.join(f'{float(s):.9e}' for s in scores)} best {n_best})", flush=True)


def summary(path):
    times, scores, cur = {}, {}, None
    for line in open(path):
        line = line.strip()
        if line.startswith("== "):
            cur = line[3:]
        m = re.search(r"launch \d+: ([0-9.]+) ms   \(scores (.*)\)", line)
        if m and cur:
            times.setdefault(cur, []).append(float(m.group(1)))
            scores.setdefault(cur.split(" | ")[0], set()).add(m.group(2))
    for key, v in times.items():
        print(f"{key} median {statistics.median(v):.4f} min {min(v):.4f} max {max(v):.4f} n={len(v)}")
    differ = [case for case, s in scores.items() if len(s) != 1]
    print("scores: " + ("the legs agree to ten digits in every case" if not differ else f"THE LEGS DIFFER in {differ}"))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "summary":
        sys.exit(summary(sys.argv[2]))
    if len(sys.argv) < 2 or sys.argv[1] not in ("per-solve", "batched"):
        sys.exit(__doc__)
    run_leg(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 0, sys.argv[3] if len(sys.argv) > 3 else "")
