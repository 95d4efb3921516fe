#!/usr/bin/env python3
"""Model-selection sweeps of mid-size problems: evaluate_best_ic(batched=True, batch_kernel="mid") -- the restarts of CCC and
the one solve of AIC through Problem.solve_many_mid, the folds of BCV through Problem.solve_many_mid_masked, several
workgroups per solve -- against one solve at a time and against the one-launch batch (evaluate_best_ic(batched=True), one
workgroup per solve).

   python tools/mid_ic_bench.py per-solve|small|mid [repetition [case]]   one timing of every case on one leg
   python tools/mid_ic_bench.py summary FILE                              medians and validity of a file of such output

Cases (tol 1e-2, 20 inner steps, initialiser uniform_, seed 1, candidates n_u = 1..4, at most 200 outer iterations), each on
synthetic_problem(N, S, n_c, n_u, seed=5, depth=30):
  1000x16 (6 + 2), 4000x16 (6 + 2)         BCV 20 folds, CCC 20 restarts, AIC
  10000x64 (12 + 4), 32768x64 (12 + 4)     BCV 5 folds, CCC 20 restarts, AIC
Legs: `per-solve` calls evaluate_best_ic without a keyword and uses nothing the batched routes added, so the same file runs
on a checkout of the commit before the mid-size route -- which is where it is meant to run.  `small` passes batched=True; a
case outside the one-launch batch's envelope is skipped.  `mid` passes batched=True, batch_kernel="mid".

Method: run the legs in turn, one process each, five times, append the output to one file, then `summary`.  A timing is a
host clock around a call that returns host arrays (it ends in a device synchronise), after a warm-up call of the same case
with three outer iterations.  Every timing is a line "launch <repetition>: <ms> ms   (scores ...)" under its
"== <case> | <leg>" heading.  `summary` prints per case the median of each leg, marks the case INVALID unless every timing
of every leg shows the same scores to ten digits, and says whether the mid-size leg beats both others."""
import re
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

TOL, T2, MAX_OUTER = 1e-2, 20, 200
CANDIDATES = (1, 2, 3, 4)
SHAPES = ((1000, 16, 6, 2, 20), (4000, 16, 6, 2, 20), (10000, 64, 12, 4, 5), (32768, 64, 12, 4, 5))  # N, S, n_c, n_u, BCV folds
LEGS = ("per-solve", "small", "mid")


def run_leg(leg, repetition, only=""):
    from demethify_amd import _lib as L
    from demethify_amd.device import get_context, small_solve_supported
    from demethify_amd.ic import evaluate_best_ic
    from oracle.solver import synthetic_problem

    kw = {"per-solve": {}, "small": {"batched": True}, "mid": {"batched": True, "batch_kernel": "mid"}}[leg]
    ctx = get_context()
    for N, S, n_c, n_u, folds in SHAPES:
        if leg == "small" and not all(small_solve_supported(N, S, n_c, n, L.DMF_MODE_PARTIAL) for n in CANDIDATES):
            continue
        data = None
        for ic, n in (("BCV", folds), ("CCC", 20), ("AIC", 1)):
            name = f"{N}x{S} {ic}" + (f" {n}" if ic != "AIC" else "")
            if only not in name:
                continue
            if data is None:
                data = synthetic_problem(N, S, n_c, n_u, seed=5, depth=30)
            V, D, Rt = data
            evaluate_best_ic(V, Rt, D, "uniform_", ic, 1, 3, T2, TOL, n_restarts=n, n_u_values=CANDIDATES, **kw)  # warm-up
            ctx.synchronize()
            t0 = time.perf_counter()
            _, _, n_best, scores = evaluate_best_ic(V, Rt, D, "uniform_", ic, 1, MAX_OUTER, T2, TOL, n_restarts=n,
                                                    n_u_values=CANDIDATES, **kw)
            ms = (time.perf_counter() - t0) * 1e3
            print(f"== {name} | {leg}")
            print(f"launch {repetition}: {ms:.3f} ms   (scores {' '.join(f'{float(s):.9e}' for s in scores)} best {n_best})", flush=True)


def summary(path):
    times, scores, order, head = {}, {}, [], None
    for line in Path(path).read_text().splitlines():
        m = re.match(r"== (.+) \| (.+)$", line)
        if m:
            head = (m.group(1), m.group(2))
            if head[0] not in order:
                order.append(head[0])
            continue
        m = re.match(r"launch \d+: ([0-9.]+) ms\s+\(scores (.*)\)", line)
        if m and head is not None:
            times.setdefault(head, []).append(float(m.group(1)))
            scores.setdefault(head[0], set()).add(m.group(2))
    bad = 0
    for case in order:
        med = {leg: statistics.median(times[(case, leg)]) for leg in LEGS if (case, leg) in times}
        text = "   ".join(f"{leg} {med[leg]:.1f} ms (min {min(times[(case, leg)]):.1f} max {max(times[(case, leg)]):.1f} "
                          f"n = {len(times[(case, leg)])})" for leg in med)
        valid = len(scores[case]) == 1
        bad += not valid
        wins = valid and "mid" in med and len(med) > 1 and all(med["mid"] < v for leg, v in med.items() if leg != "mid")
        print(f"{case}: {text}   {'valid: the legs agree to ten digits' if valid else 'INVALID: scores ' + ' | '.join(sorted(scores[case]))}"
              f"   {'mid wins' if wins else 'mid does not win'}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "summary":
        sys.exit(summary(sys.argv[2]))
    elif len(sys.argv) >= 2 and sys.argv[1] in LEGS:
        run_leg(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 0, sys.argv[3] if len(sys.argv) > 3 else "")
    else:
        sys.exit(__doc__)
