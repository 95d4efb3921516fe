"""Bi-cross-validation folds, the loop as it was against the device-resident one, in one process.

5e5 CpG x 128 samples, unsupervised, n_u = 2..6, 5 folds, 50 outer iterations per fold (tol = 0).  Per n_u and repetition
three legs run one after the other (interleaved, medians over the repetitions):
  old     the loop bicross_validation replaced, with a timer around every piece of a fold: mask draw, the two host
          multiplies, upload + build of a fresh Problem, initialiser, solve, download, numpy error
  staged  the new fold's pieces one after the other on the calling thread: mask draw, initialiser, pack + upload of the
          bits, derive (Problem.masked), solve, error pass (Solver.holdout_error)
  new     bicross_validation itself on one resident Problem: the draws of fold k + 1 on the worker thread behind the
          solve of fold k -- wall time per fold only
   python tools/bcv_bench.py [repetitions] [n_u lo hi] [N]"""
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from demethify_amd import _lib as L
from demethify_amd.deconvolution import _init_unsupervised
from demethify_amd.device import Problem, Solver, get_context, pack_mask
from demethify_amd.ic import bicross_validation
from demethify_amd.staging import mask_to_device

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
LO, HI = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (2, 6)
N = int(sys.argv[4]) if len(sys.argv) > 4 else 500_000
S, K_true, FOLDS, T1, T2, SEED, FRACTION = 128, 4, 5, 50, 20, 1, 0.3

rs = np.random.RandomState(0)
R = rs.beta(0.5, 0.5, size=(N, K_true))
A = rs.dirichlet(np.ones(K_true), S).T
D = rs.poisson(50, (N, S)) + 1
V = rs.binomial(D, np.clip(R @ A, 0, 1)) / D
D = D.astype(np.int64)
del R, A
ctx = get_context()


class Clock:
    def __init__(self):
        self.t = {}

    def lap(self, name, t0):
        ctx.synchronize()
        t1 = time.perf_counter()
        self.t[name] = self.t.get(name, 0.0) + (t1 - t0)
        return t1


def old_leg(n_u):
    """ic.py:58-89 as this package ran it before: everything per fold from the host."""
    c = Clock()
    np.random.seed(SEED)
    total = 0.0
    for _ in range(FOLDS):
        t = time.perf_counter()
        train = np.random.rand(N, S) < FRACTION
        test = ~train
        t = c.lap("mask draw", t)
        Vm, Dm = V * train, D * train
        t = c.lap("multiply", t)
        p = Problem(ctx, Vm, Dm, None)
        t = c.lap("upload + build", t)
        u0, a0 = _init_unsupervised("uniform_", Vm, n_u, SEED)
        t = c.lap("initialiser", t)
        with Solver(p, u0, a0, L.DMF_MODE_UNSUPERVISED) as s:
            s.step(T1, T2, 0.0)
            t = c.lap("solve", t)
            u, alpha, _, _ = s.get()
        p.close()
        t = c.lap("download", t)
        total += np.linalg.norm((V - u @ alpha) * test, "fro") ** 2 / np.sum(test)
        t = c.lap("numpy error", t)
    return total, c.t


def staged_leg(n_u, full):
    c = Clock()
    np.random.seed(SEED)
    total = 0.0
    for _ in range(FOLDS):
        t = time.perf_counter()
        train = np.random.rand(N, S) < FRACTION
        t = c.lap("mask draw", t)
        u0, a0 = _init_unsupervised("uniform_", V, n_u, SEED)
        t = c.lap("initialiser", t)
        bits = mask_to_device(pack_mask(train), ctx)
        t = c.lap("pack + upload bits", t)
        p = full.masked(bits)
        t = c.lap("derive", t)
        with Solver(p, u0, a0, L.DMF_MODE_UNSUPERVISED) as s:
            s.step(T1, T2, 0.0)
            t = c.lap("solve", t)
            sum_sq, n_test = s.holdout_error(full)
            t = c.lap("error pass", t)
        p.close()
        bits.close()
        total += sum_sq / n_test
    return total, c.t


def med(xs):
    return float(np.median(xs))


print(f"bi-cross-validation at {N} x {S}, unsupervised, {FOLDS} folds x {T1} outer iterations (T2 = {T2}, tol = 0), "
      f"medians of {REPS} interleaved repetitions; seconds PER FOLD")
t0 = time.perf_counter()
full = Problem(ctx, V, D, None)
ctx.synchronize()
print(f"the one resident upload of the new path: {time.perf_counter() - t0:.3f} s (once per sweep, not per fold)")
old_leg(LO), staged_leg(LO, full)  # warm-up: page-locked staging buffers, the pool's blocks, code objects
for n_u in range(LO, HI + 1):
    olds, stgs, news, parts_old, parts_stg, agree = [], [], [], {}, {}, 0.0
    for _ in range(REPS):
        t = time.perf_counter()
        tot_old, po = old_leg(n_u)
        olds.append((time.perf_counter() - t) / FOLDS)
        t = time.perf_counter()
        tot_stg, ps = staged_leg(n_u, full)
        stgs.append((time.perf_counter() - t) / FOLDS)
        t = time.perf_counter()
        tot_new, _, _ = bicross_validation(V, n_u, D, T1, T2, 0.0, n_folds=FOLDS, seed=SEED, ref=None, problem=full)
        news.append((time.perf_counter() - t) / FOLDS)
        for k, v in po.items():
            parts_old.setdefault(k, []).append(v / FOLDS)
        for k, v in ps.items():
            parts_stg.setdefault(k, []).append(v / FOLDS)
        agree = max(agree, abs(tot_new - tot_old) / tot_old, abs(tot_stg - tot_old) / tot_old)
    draw = med(parts_stg["mask draw"]) + med(parts_stg["initialiser"])
    print(f"0+{n_u}: old {med(olds):.3f}  new {med(news):.3f} (x{med(olds) / med(news):.2f})  new without the worker thread "
          f"{med(stgs):.3f}   | press sums agree to {agree:.1e}")
    print("      old fold:    " + "  ".join(f"{k} {med(v):.4f}" for k, v in parts_old.items()))
    print("      new fold:    " + "  ".join(f"{k} {med(v):.4f}" for k, v in parts_stg.items()))
    print(f"      host draws (mask + initialiser) {draw:.4f} = {100 * draw / med(stgs):.0f} % of the unhidden new fold, "
          f"{100 * draw / med(news):.0f} % of the fold as run; device work of a fold "
          f"{med(stgs) - draw:.4f}; hidden by the worker thread: {med(stgs) - med(news):.4f}")
full.close()
