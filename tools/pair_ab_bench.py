#!/usr/bin/env python3
"""Diagnostic: the row pass's pair schedule against the one-block loop, per shape, in one process (level 0, X16 form).
   python tools/pair_ab_bench.py [iterations]
Per shape one problem; solvers with the context's pair switch off and on alternate three times each, and every line
reports the solver-loop time per outer iteration and how many of its row-pass launches ran the pair schedule."""
import statistics, sys, time
from pathlib import Path
import numpy as np
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
from bench import make_inputs_on_device
from demethify_amd import _lib as L
from demethify_amd.device import Context, Problem, Solver

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dev = torch.device("cuda", 0)
ctx = Context(0)
SHAPES = [(1_000_000, 256, 12, 4), (1_000_000, 192, 12, 4), (1_000_000, 128, 12, 4), (1_000_000, 128, 12, 3),
          (1_000_000, 96, 6, 2), (1_000_000, 65, 12, 4), (1_000_000, 65, 0, 1)]
for N, S, n_c, n_u in SHAPES:
    V, D, Rt = make_inputs_on_device(torch, dev, N, S, max(n_c, 1), n_u, seed=0)
    rs = np.random.RandomState(1)
    u0 = rs.uniform(size=(N, n_u)); a0 = rs.dirichlet(np.ones(n_c + n_u), S).T
    mode = L.DMF_MODE_PARTIAL if n_c else L.DMF_MODE_UNSUPERVISED
    times = {False: [], True: []}
    paired = {}
    with Problem(ctx, V, D, Rt if n_c else None) as p:
        for rep in range(3):
            for pair in (False, True):
                ctx.set_rowpass_pair(pair)
                with Solver(p, u0, a0, mode) as s:
                    s.step(2, 20, 0.0); ctx.synchronize()
                    t0 = time.perf_counter(); s.step(iters, 20, 0.0); ctx.synchronize()
                    times[pair].append((time.perf_counter() - t0) / iters * 1e3)
                    paired[pair] = s.rowpass_launches()
                    desc = s.describe(20)
        ctx.set_rowpass_pair(True)
    one, two = statistics.median(times[False]), statistics.median(times[True])
    print(f"N={N} S={S} {n_c}+{n_u}: one block {one:7.3f} ms/iter, pair switch on {two:7.3f} ms/iter ({(one / two - 1) * 100:+5.1f} %), "
          f"pair launches {paired[True][1]}/{paired[True][0]} (off: {paired[False][1]})   {desc}", flush=True)
    del V, D, Rt
