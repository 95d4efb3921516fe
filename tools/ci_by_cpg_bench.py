"""Profile intervals by CpG against by resampled position (bt_ci's profile_rows): the two steps of
the bootstrap that differ between the modes, one process, the modes alternating.

    python tools/ci_by_cpg_bench.py [--out profiles/ci_by_cpg.txt] [--replicates 120] [--reps 5] [--hbm-tbs 8.0] [--quick]

One solver on a resident problem of N x S with n_c + n_u types (the data are placeholders: only u and the row draws are read
here) and two replicate stacks of --replicates x (N n_u) doubles in HBM.  Per replicate, with its own row draw as the
bootstrap uploads it, the store of the profiles into the stack: Solver.copy_u_to ("position") and Solver.copy_u_by_cpg ("cpg"),
one after the other; then, each replicate's row having received noise of its own (the solver is not stepped: without it a
column would hold 120 equal numbers), --reps rounds of the percentile pass over each stack, Context.percentile_axis0 and
Context.nanpercentile_axis0, alternating.  Printed:
  the store        the library's own events (kernel family "gram": k_first_fill + k_first_occurrence + k_copy_rows_first
                   for "cpg"; "position" without a column order is a device-to-device copy with no kernel, so only its wall
                   time is given) and the wall time of the call, medians over the replicates, next to the byte floors at
                   --hbm-tbs (default 8 TB/s, the card's data-sheet rate)
  the percentiles  wall time of the call on device arrays, which ends in a synchronise (the percentile entry points carry no
                   family clock), medians of --reps after a warm-up, next to the floor of reading the stack once
  what "cpg" adds  per replicate: store("cpg") - store("position") + (nanpercentile - percentile) / replicates
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402  (the replicate stacks are CUDA tensors; torch brings up its HIP runtime first)

from demethify_amd import _lib as L  # noqa: E402
from demethify_amd.bootstrap import bootstrap_row_indices, bootstrap_seed_sequence  # noqa: E402
from demethify_amd.device import Problem, Solver, get_context  # noqa: E402
from demethify_amd.staging import indices_to_device  # noqa: E402


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def measure(ctx, N, S, n_c, n_u, args, say):
    B = args.replicates
    rs = np.random.RandomState(1)
    V = rs.rand(N, S)
    D = np.full((N, S), 30, dtype=np.int64)
    Rt = rs.rand(N, n_c)
    u0 = rs.rand(N, n_u)
    a0 = rs.dirichlet(np.ones(n_c + n_u), S).T
    q = [2.5, 97.5]
    dev = torch.device("cuda", ctx.device)
    with Problem(ctx, V, D, Rt) as p, Solver(p, u0, a0, L.DMF_MODE_PARTIAL) as s:
        del V, D, Rt
        stack_pos = torch.empty((B, N * n_u), dtype=torch.float64, device=dev)
        stack_cpg = torch.empty((B, N * n_u), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        warm = indices_to_device(bootstrap_row_indices(0, N), ctx)
        s.copy_u_to(stack_pos[0])
        s.copy_u_by_cpg(stack_cpg[0], warm, N)
        t_pos, t_cpg, drawn = [], [], []
        ctx.set_profiling(True, families=[L.KERNEL_GRAM])
        ctx.reset_kernel_time()
        for j, seed in enumerate(bootstrap_seed_sequence(1, B)):  # the stores alternate, replicate by replicate
            idx = bootstrap_row_indices(seed, N)
            idx_dev = indices_to_device(idx, ctx)
            ctx.synchronize()
            t_pos.append(wall(lambda: s.copy_u_to(stack_pos[j])))
            t_cpg.append(wall(lambda: s.copy_u_by_cpg(stack_cpg[j], idx_dev, N)))
            if j < 8:
                drawn.append(np.unique(idx).size / N)
        ms_gram, launches = ctx.kernel_time(L.KERNEL_GRAM)
        ctx.set_profiling(False)
        ms_cpg_kernels = ms_gram / B  # (two clocked groups per call: the table's two kernels, then the copy)
        if launches != 2 * B:
            say(f"  (the gram clock counted {launches} groups, expected {2 * B}: something else was clocked)")
        present = float(np.mean(drawn))
        # the solver was not stepped, so every replicate stored the same u: give each its own values (the same noise in both
        # stacks; NaN stays NaN), or the kernels would meet 120 equal numbers per column and never insert after the first
        gen = torch.Generator(device=dev).manual_seed(1)
        for j in range(B):
            noise = torch.rand(N * n_u, dtype=torch.float64, device=dev, generator=gen)
            stack_pos[j] += noise
            stack_cpg[j] += noise
        torch.cuda.synchronize()

        ctx.percentile_axis0(stack_pos, q), ctx.nanpercentile_axis0(stack_cpg, q)  # warm-up
        p_pos, p_cpg = [], []
        for _ in range(args.reps):  # the passes alternate
            p_pos.append(wall(lambda: ctx.percentile_axis0(stack_pos, q)))
            p_cpg.append(wall(lambda: ctx.nanpercentile_axis0(stack_cpg, q)))
        nan_share = float(torch.isnan(stack_cpg[:8]).double().mean())
    med = statistics.median
    rate = args.hbm_tbs * 1e12
    row = 8 * n_u
    floor_pos = 2 * N * row / rate * 1e3
    # fill 8 N, read idx 8 N, one atomic per position 8 N, read the table 8 N, read the rows that are some CpG's first, write
    floor_cpg = (32 * N + (1 + present) * N * row) / rate * 1e3
    floor_pct = (B + 2) * N * row / rate * 1e3
    say(f"{N} x {S}, {n_c}+{n_u}, {B} replicates; a replicate draws {100 * present:.1f} % of the CpGs, "
        f"{100 * nan_share:.1f} % of the by-CpG stack is NaN")
    say(f"  store, position  copy_u_to            wall {med(t_pos):8.4f} ms (min {min(t_pos):.4f})  |  floor {floor_pos:.4f} ms "
        f"({2 * N * row / 1e6:.0f} MB at {args.hbm_tbs} TB/s)")
    say(f"  store, cpg       copy_u_by_cpg        wall {med(t_cpg):8.4f} ms (min {min(t_cpg):.4f})  |  its three kernels "
        f"{ms_cpg_kernels:.4f} ms  |  floor {floor_cpg:.4f} ms  floor / kernels {floor_cpg / ms_cpg_kernels:.2f}")
    say(f"  percentiles, position  percentile_axis0     wall {med(p_pos):9.3f} ms (min {min(p_pos):.3f})  |  floor {floor_pct:.3f} ms "
        f"({(B + 2) * N * row / 1e9:.2f} GB)  floor / wall {floor_pct / med(p_pos):.2f}")
    say(f"  percentiles, cpg       nanpercentile_axis0  wall {med(p_cpg):9.3f} ms (min {min(p_cpg):.3f})  |  floor {floor_pct:.3f} ms  "
        f"floor / wall {floor_pct / med(p_cpg):.2f}")
    added = med(t_cpg) - med(t_pos) + (med(p_cpg) - med(p_pos)) / B
    say(f"  \"cpg\" adds per replicate: store {med(t_cpg) - med(t_pos):+.4f} ms, percentiles {(med(p_cpg) - med(p_pos)) / B:+.4f} ms "
        f"-> {added:+.4f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--replicates", type=int, default=120)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--quick", action="store_true", help="a tiny shape only (a rehearsal of the tool, not a measurement)")
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
        if args.out:  # (written as it goes: a run that is cut short keeps what it has)
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(lines) + "\n")

    ctx = get_context()
    say("# tools/ci_by_cpg_bench.py: the store of a replicate's profiles and the percentile pass, profile_rows \"cpg\" against "
        f"\"position\"; one process, the modes alternating; percentile medians of {args.reps} after a warm-up")
    shape = (3000, 8, 3, 2) if args.quick else (1000000, 256, 12, 4)
    if args.quick:
        args.replicates = min(args.replicates, 12)
    measure(ctx, *shape, args, say)


if __name__ == "__main__":
    main()
