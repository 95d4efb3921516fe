"""Component matching of a bootstrap replicate: the device leg (Solver.match_components + the assignment +
Solver.copy_u_to(columns=...)) against the leg it replaces (Solver.get() of u, numpy ``u.T @ anchor[idx]`` on the host),
one process, the two legs alternating.

    python tools/component_match_bench.py [--out profiles/component_match.txt] [--reps 5] [--hbm-tbs 8.0] [--quick]

Per shape (N x S, 0 + n_u): a solver on a resident problem of that size (the data are placeholders: only u, the anchor and the
row draw are read here), an anchor of N x n_u in HBM, a row draw of N indices as the bootstrap uploads it.  Medians of --reps
after one warm-up.  Printed:
  k_match_gram + reduce     the library's own events (kernel family "gram"), next to its floor N (16 n_u + 8) bytes at --hbm-tbs
                            (default 8 TB/s, the card's data-sheet rate)
  k_copy_cols_permuted      the same clock, and the wall time of copy_u_to(columns=...) next to the plain copy_u_to
  what alignment adds       wall: match_components + assignment + permuted copy, minus the plain copy it replaces -- next to
                            the host leg: Solver.get() + numpy matmul + assignment (the re-upload of the permuted u the host
                            leg would also need is NOT counted)
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402  (the replicate stack is a CUDA tensor; torch brings up its HIP runtime first)

from demethify_amd import _lib as L  # noqa: E402
from demethify_amd.bootstrap import bootstrap_row_indices, match_components  # noqa: E402
from demethify_amd.device import Problem, Solver, get_context  # noqa: E402
from demethify_amd.staging import indices_to_device, to_device  # noqa: E402


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def clocked(ctx, fn, reps):
    """Per-call milliseconds of the "gram" family over `reps` calls of fn (after one warm-up call)."""
    fn()
    ctx.set_profiling(True, families=[L.KERNEL_GRAM])
    ctx.reset_kernel_time()
    for _ in range(reps):
        fn()
    ms, launches = ctx.kernel_time(L.KERNEL_GRAM)
    ctx.set_profiling(False)
    return ms / max(launches, 1)


def measure(ctx, N, S, n_u, args, say):
    rs = np.random.RandomState(1)
    V = rs.rand(N, S)
    D = np.full((N, S), 30, dtype=np.int64)
    u0 = rs.rand(N, n_u)
    a0 = rs.dirichlet(np.ones(n_u), S).T
    anchor = np.ascontiguousarray(u0[:, rs.permutation(n_u)] * 0.9 + 0.1 * rs.rand(N, n_u))
    idx = bootstrap_row_indices(7, N)
    with Problem(ctx, V, D, None) as p, Solver(p, u0, a0, L.DMF_MODE_UNSUPERVISED) as s:
        del V, D
        anchor_dev, = to_device((anchor,), ctx)
        idx_dev = indices_to_device(idx, ctx)
        row = torch.empty(N * n_u, dtype=torch.float64, device=torch.device("cuda", ctx.device))
        found = {}

        def device_leg():
            perm = match_components(s.match_components(anchor_dev, idx_dev))
            s.copy_u_to(row, columns=np.argsort(perm))
            found["device"] = perm

        def plain_copy():
            s.copy_u_to(row)

        def permuted_copy():
            s.copy_u_to(row, columns=np.arange(n_u)[::-1])

        def host_leg():
            u = s.get()[0]
            found["host"] = match_components(u.T @ anchor[idx])

        for fn in (device_leg, plain_copy, permuted_copy, host_leg):  # warm-up
            fn()
        assert found["device"].tolist() == found["host"].tolist(), found
        t = {name: [] for name in ("device", "plain", "permuted", "host")}
        for _ in range(args.reps):  # the legs alternate
            t["device"].append(wall(device_leg))
            t["host"].append(wall(host_leg))
            t["plain"].append(wall(plain_copy))
            t["permuted"].append(wall(permuted_copy))
        med = {k: statistics.median(v) * 1e3 for k, v in t.items()}
        ms_match = clocked(ctx, lambda: s.match_components(anchor_dev, idx_dev), args.reps)
        ms_copy = clocked(ctx, permuted_copy, args.reps)
    bytes_ = N * (16 * n_u + 8)
    floor = bytes_ / (args.hbm_tbs * 1e12) * 1e3
    say(f"{N:>8} x {S:<4} 0+{n_u:<2}  k_match_gram + reduce {ms_match:8.4f} ms  |  HBM floor {floor:7.4f} ms "
        f"({bytes_ / 1e6:.1f} MB at {args.hbm_tbs} TB/s)  floor / measured {floor / ms_match:5.2f}")
    say(f"{'':>8}   {'':<4} {'':<5} k_copy_cols_permuted {ms_copy:8.4f} ms  |  copy_u_to wall: plain {med['plain']:8.4f} ms  "
        f"columns=... {med['permuted']:8.4f} ms")
    say(f"{'':>8}   {'':<4} {'':<5} alignment per replicate, wall: device leg {med['device']:8.4f} ms - plain copy = "
        f"{med['device'] - med['plain']:8.4f} ms added  |  host leg (get + numpy) {med['host']:9.3f} ms  "
        f"host / device-added {med['host'] / max(med['device'] - med['plain'], 1e-9):7.1f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--quick", action="store_true", help="tiny shapes only (a rehearsal of the tool, not a measurement)")
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
        if args.out:  # (written as it goes: a run that is cut short keeps what it has)
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(lines) + "\n")

    ctx = get_context()
    say("# tools/component_match_bench.py: device = Solver.match_components + assignment + copy_u_to(columns=...), "
        f"host = Solver.get() + numpy u.T @ anchor[idx] + assignment; medians of {args.reps} after a warm-up, legs alternating, "
        "one process")
    shapes = [(3000, 8, 3), (2000, 6, 12)] if args.quick else [(1000000, 256, 4), (500000, 128, 12)]
    for shape in shapes:
        measure(ctx, *shape, args, say)


if __name__ == "__main__":
    main()
