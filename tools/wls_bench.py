"""Reference-based regression: S host solves (init_func.wls_intercept, what the callers run below
init_func.DEVICE_WLS_MIN_ELEMENTS) against device.Problem.wls_intercept, one process.

    python tools/wls_bench.py [--out profiles/wls_bench.txt] [--reps 5] [--host-samples 4] [--quick]

Per shape (synthetic_problem's recipe): the host time, the device time with the problem resident (regression launches
only), and the device time upload included (Problem creation from host arrays + regression), medians of --reps after one
warm-up each; host walls end in numpy results, device walls in the copy of the result to the host.  At the larger shapes the
host leg times --host-samples samples and scales to S (said in the output).  The sweep at the bottom looks for the smallest
power of two N * S at which the device, upload included, is at least twice as fast as the host.
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from demethify_amd.device import Problem, get_context  # noqa: E402
from demethify_amd.init_func import wls_intercept  # noqa: E402
from oracle.solver import synthetic_problem  # noqa: E402


def median_wall(fn, reps):
    fn()  # warm-up
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def host_leg(V, D, R_full, target, samples):
    for k in samples:
        x = D[:, k:k + 1] * V[:, k:k + 1] if target == "dv" else V[:, k:k + 1]
        wls_intercept(x, D[:, k:k + 1], R_full)


def measure(ctx, N, S, n_c, n_u, target, reps, host_samples, say):
    V, D, Rt = synthetic_problem(N, S, n_c, n_u, seed=1)
    u = np.random.RandomState(9).uniform(size=(N, n_u)) if n_u else None
    R_full = np.c_[Rt, u] if n_u else Rt
    n_host = min(S, host_samples) if N * S > (1 << 22) else S
    t_host = median_wall(lambda: host_leg(V, D, R_full, target, range(n_host)), max(1, reps if n_host == S else 1)) * S / n_host

    def with_upload():
        with Problem(ctx, V, D, Rt) as p:
            p.wls_intercept(u, target)

    t_upload = median_wall(with_upload, reps)
    with Problem(ctx, V, D, Rt) as p:
        got = p.wls_intercept(u, target)
        status = p.wls_status
        t_resident = median_wall(lambda: p.wls_intercept(u, target), reps)
    want = np.concatenate([wls_intercept(D[:, k:k + 1] * V[:, k:k + 1] if target == "dv" else V[:, k:k + 1], D[:, k:k + 1], R_full)
                           for k in range(min(S, 2))], axis=1)
    err = float(np.abs(got[:, :want.shape[1]] - want).max())
    say(f"{N:>8} x {S:<4} {n_c}+{n_u} target={target:<2}  host {t_host * 1e3:10.2f} ms"
        f"{'' if n_host == S else f' ({n_host} samples timed, scaled to {S})'}  device resident {t_resident * 1e3:8.3f} ms  "
        f"device with upload {t_upload * 1e3:9.2f} ms  host/upload {t_host / t_upload:7.1f}x  "
        f"status!=0: {int((status != 0).sum())}  max abs diff (2 samples) {err:.1e}")
    return t_host, t_upload


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-samples", type=int, default=4)
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
    say("# tools/wls_bench.py: host = S x init_func.wls_intercept, device = Problem.wls_intercept; medians of "
        f"{args.reps} after a warm-up, wall clock, one process")
    shapes = [(2000, 8, 6, 0, "dv"), (2000, 8, 6, 2, "v")] if args.quick else \
        [(100000, 64, 6, 0, "dv"), (1000000, 256, 12, 0, "dv"), (1000000, 256, 12, 4, "v")]
    for N, S, n_c, n_u, target in shapes:
        measure(ctx, N, S, n_c, n_u, target, args.reps, args.host_samples, say)
    say("# crossover sweep, 12+0 target=dv, S = 16: smallest power of two N * S where host / (device with upload) >= 2")
    found = None  # (the smallest size from which EVERY larger size of the sweep meets the bar)
    for e in (range(10, 14) if args.quick else range(12, 23)):
        n_elem = 1 << e
        t_host, t_upload = measure(ctx, n_elem // 16, 16, 12, 0, "dv", args.reps, args.host_samples, say)
        if t_host < 2.0 * t_upload:
            found = None
        elif found is None:
            found = n_elem
    say(f"# crossover: {'2^%d = %d' % (found.bit_length() - 1, found) if found else 'not reached in the sweep'}")


if __name__ == "__main__":
    main()
