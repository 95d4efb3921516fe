"""The SVD initialiser: host route (S x init_func.wls_intercept, then scipy's SVD of the N x S residual inside
init_func.nndsvd_initialize) against device.Problem.nndsvd, one process.

    python tools/svd_init_bench.py [--out profiles/svd_init_bench.txt] [--reps 3] [--host-samples 2] [--host-svd-rows 100000]
                                   [--quick]

Per shape (synthetic_problem's recipe) two legs, timed separately because the host regression alone takes minutes at the
large shapes:
  regression   host = S host solves (at N * S > 2^22: --host-samples samples timed and scaled to S, said in the output);
               device = Problem.wls_intercept, problem resident
  SVD          host = nndsvd_initialize on the residual (above --host-svd-rows rows: timed on the first --host-svd-rows rows
               and scaled by N, the cost of a thin SVD at fixed S being linear in N; said in the output);
               device = dmf_svd_gram + numpy.linalg.eigh + dmf_svd_factor + dmf_svd_finish with H1 given, problem resident
and the whole call: Problem.nndsvd with the problem resident, and upload included (Problem creation from host arrays).
Medians of --reps after one warm-up, wall clock; device walls end in the host copy of u0.

k_svd_gram is also timed by the library's own events (kernel family "gram": k_svd_gram + its reduce) and printed next to its
two floors: N * S * 8 B of V plus N * n_c * 8 B of profiles at --hbm-tbs (default 8 TB/s, the card's data-sheet rate), and
N * S * (S + 16) / 2 * 2 flop of the upper 16 x 16 tiles plus the residual's N * S * 2 * n_c flop at --fp64-tflops (default
78.6, the data-sheet FP64 matrix rate).  The sweep at the bottom looks for the smallest power of two N * S at which the
device route, upload included, is at least twice as fast as the host route (6+2 types, 16 samples).
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from demethify_amd import _lib as L  # noqa: E402
from demethify_amd.device import Problem, get_context  # noqa: E402
from demethify_amd.init_func import nndsvd_initialize, wls_intercept  # noqa: E402
from oracle.solver import synthetic_problem  # noqa: E402


def median_wall(fn, reps):
    fn()  # warm-up
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def measure(ctx, N, S, n_c, n_u, args, say, detail=True):
    V, D, Rt = synthetic_problem(N, S, n_c, n_u, seed=1)
    if n_c == 0:
        Rt = None
    big = N * S > (1 << 22)
    reps_host = 1 if big else args.reps
    # ---- host legs
    t_host_wls, note_wls = 0.0, ""
    if n_c:
        n_host = min(S, args.host_samples) if big else S
        t_host_wls = median_wall(lambda: [wls_intercept(V[:, k:k + 1], D[:, k:k + 1], Rt) for k in range(n_host)],
                                 reps_host) * S / n_host
        if n_host != S:
            note_wls = f" ({n_host} samples timed, scaled to {S})"
    with Problem(ctx, V, D, Rt) as p:
        H1 = p.wls_intercept(None, "v", host_arrays=(V, D, Rt)) if n_c else None
        n_svd = min(N, args.host_svd_rows)
        Y = np.maximum(V[:n_svd] - Rt[:n_svd] @ H1, 1e-8) if n_c else V[:n_svd]
        t_host_svd = median_wall(lambda: nndsvd_initialize(Y, n_u), reps_host) * N / n_svd
        note_svd = "" if n_svd == N else f" ({n_svd} rows timed, scaled to {N})"
        del Y
        # ---- device legs, problem resident
        t_dev_wls = median_wall(lambda: p.wls_intercept(None, "v", host_arrays=(V, D, Rt)), args.reps) if n_c else 0.0
        inner = p.wls_intercept
        p.wls_intercept = lambda *a, **kw: H1  # (the SVD leg alone: H1 given)
        t_dev_svd = median_wall(lambda: p.nndsvd(n_u), args.reps)
        p.wls_intercept = inner
        t_resident = median_wall(lambda: p.nndsvd(n_u, host_arrays=(V, D, Rt)), args.reps)
        if detail:
            ctx.set_profiling(True, families=[L.KERNEL_GRAM])
            ctx.reset_kernel_time()
            for _ in range(args.reps):
                p.svd_gram(H1)
            ms, launches = ctx.kernel_time(L.KERNEL_GRAM)
            ctx.set_profiling(False)
            t_gram = ms / max(launches, 1) * 1e-3

    def with_upload():
        with Problem(ctx, V, D, Rt) as q:
            q.nndsvd(n_u, host_arrays=(V, D, Rt))

    t_upload = median_wall(with_upload, args.reps)
    t_host = t_host_wls + t_host_svd
    say(f"{N:>8} x {S:<4} {n_c}+{n_u}  host regression {t_host_wls * 1e3:11.2f} ms{note_wls}  host SVD {t_host_svd * 1e3:10.2f} ms"
        f"{note_svd}  |  device regression {t_dev_wls * 1e3:8.3f} ms  device SVD {t_dev_svd * 1e3:8.3f} ms  "
        f"nndsvd resident {t_resident * 1e3:8.3f} ms  with upload {t_upload * 1e3:9.2f} ms  host/upload {t_host / t_upload:8.1f}x")
    if detail:
        bytes_ = N * S * 8 + N * n_c * 8
        flop = N * S * (S + 16) / 2 * 2 + N * S * 2 * n_c
        say(f"{'':>8}   {'':<4} k_svd_gram + reduce {t_gram * 1e3:8.3f} ms  |  HBM floor {bytes_ / (args.hbm_tbs * 1e12) * 1e3:7.3f} ms "
            f"({bytes_ / 1e9:.3f} GB at {args.hbm_tbs} TB/s)  FP64 matrix floor {flop / (args.fp64_tflops * 1e12) * 1e3:7.3f} ms "
            f"({flop / 1e9:.1f} Gflop at {args.fp64_tflops} Tflop/s)")
    return t_host, t_upload


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-samples", type=int, default=2)
    ap.add_argument("--host-svd-rows", type=int, default=100000)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--fp64-tflops", type=float, default=78.6)
    ap.add_argument("--quick", action="store_true", help="tiny shapes only (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--no-sweep", action="store_true")
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
        if args.out:  # (written as it goes: a run that is cut short keeps what it has)
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(lines) + "\n")

    ctx = get_context()
    say("# tools/svd_init_bench.py: host = S x init_func.wls_intercept + init_func.nndsvd_initialize, device = Problem.nndsvd; "
        f"medians of {args.reps} after a warm-up, wall clock, one process")
    shapes = [(2000, 8, 6, 2), (3000, 9, 0, 4)] if args.quick else \
        [(100000, 64, 6, 2), (1000000, 256, 12, 4), (500000, 128, 0, 4)]
    for shape in shapes:
        measure(ctx, *shape, args, say)
    if args.no_sweep:
        return
    say("# crossover sweep, 6+2 types, S = 16: smallest power of two N * S where host / (device with upload) >= 2")
    found = None  # (the smallest size from which EVERY larger size of the sweep meets the bar)
    for e in (range(10, 13) if args.quick else range(10, 21)):
        n_elem = 1 << e
        t_host, t_upload = measure(ctx, n_elem // 16, 16, 6, 2, args, say, detail=False)
        if t_host < 2.0 * t_upload:
            found = None
        elif found is None:
            found = n_elem
    say(f"# crossover: {'2^%d = %d' % (found.bit_length() - 1, found) if found else 'not reached in the sweep'}")


if __name__ == "__main__":
    main()
