"""The hold-out mask of a bi-cross-validation fold, drawn on the host against drawn on the device, in one process.

Per shape three legs, alternating, medians of the repetitions (seconds per mask):
  host       np.random.rand(N, S) < fraction, the count of ones, pack_mask, mask_to_device -- what a fold did before
  one-wg     np.random.get_state, dmf_mask_draw_segments with blocks_per_segment = -1 (ONE persistent workgroup, the kernel
             before the jump-ahead), np.random.set_state
  segmented  the same with blocks_per_segment = 0: the plan's segments (dmf_mask_draw_plan), one workgroup each, their keys
             by jump-ahead rounds on the device
All start from the same generator state every time; the counts and the generator afterwards are compared.
Reported apart: the one-time set-up of a shape's jump polynomials (the first segmented draw of the shape in the process,
less the median of the later ones) and the per-draw jump launches -- measured on a draw with as many segments as the plan's but
64 blocks each (long enough for every jump polynomial to be dense, short enough for the draw itself to be 64 regenerations per
workgroup), less a draw of ONE such segment through the same entry.
Then a sweep of the segment count at the large shapes (what the plan's constants are read from), and one
bicross_validation call (uniform_, 4 known + 2 unknown types, 3 folds x 20 outer iterations, tol = 0) per large shape with
ic.DEVICE_MASK_MIN_ELEMENTS forced off and on, on one resident Problem.
   python tools/mask_draw_bench.py [repetitions]"""
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from demethify_amd import _lib as L
from demethify_amd import ic
from demethify_amd.device import Problem, get_context, pack_mask
from demethify_amd.staging import draw_mask, mask_to_device

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
SHAPES = [(350, 10), (10_000, 64), (100_000, 64), (1_000_000, 256)]
SWEEP_SHAPES = [(10_000, 64), (100_000, 64), (1_000_000, 256)]
SWEEP_SEGMENTS = [2, 4, 8, 16, 32, 64, 128, 256, 512, 1024]
BCV_SHAPES = [(100_000, 64), (1_000_000, 256)]
FRACTION, SEED, N_C, N_U, FOLDS, T1, T2 = 0.3, 1, 4, 2, 3, 20, 20
ctx = get_context()


def host_leg(shape):
    t = time.perf_counter()
    mask = np.random.rand(*shape) < FRACTION
    kept = int(np.sum(mask))
    bits = mask_to_device(pack_mask(mask), ctx)
    dt = time.perf_counter() - t
    bits.close()
    return dt, kept


def device_leg(shape, blocks_per_segment):
    t = time.perf_counter()
    bits, kept = draw_mask(shape, FRACTION, ctx, blocks_per_segment)
    dt = time.perf_counter() - t
    bits.close()
    return dt, kept


def med(xs):
    return float(np.median(xs))


def plan(shape):
    segments, blocks = C.c_int64(), C.c_int64()
    L.check(ctx._lib.dmf_mask_draw_plan(shape[0], shape[1], C.byref(segments), C.byref(blocks)), "dmf_mask_draw_plan")
    return segments.value, blocks.value


def blocks_of(shape):
    return (2 * shape[0] * shape[1] + 624 + 623) // 624


def timed(shape, start, blocks_per_segment, reps):
    out = []
    for _ in range(reps):
        np.random.set_state(start)
        out.append(device_leg(shape, blocks_per_segment)[0])
    return med(out)


def synthetic(n, s):
    rs = np.random.RandomState(0)
    R = rs.beta(0.5, 0.5, size=(n, N_C + N_U))
    A = rs.dirichlet(np.ones(N_C + N_U), s).T
    D = rs.randint(1, 100, size=(n, s)).astype(np.int64)
    V = np.rint(D * np.clip(R @ A, 0, 1)) / D
    return V, D, np.ascontiguousarray(R[:, :N_C])


print(f"hold-out mask draw, fraction {FRACTION}: host leg (rand, compare, count, pack_mask, mask_to_device) against the one-workgroup "
      f"device leg (get_state, dmf_mask_draw_segments -1, set_state) and the segmented device leg (the plan's segments); medians of "
      f"{REPS} alternating runs in one process, seconds per mask")
np.random.seed(SEED)
start = np.random.get_state()
PROXY_BLOCKS = 64
device_leg((PROXY_BLOCKS - 1, 312), PROXY_BLOCKS)  # the code objects, the copy stream
one = timed((PROXY_BLOCKS - 1, 312), start, PROXY_BLOCKS, REPS)  # one segment through the segmented kernel: no jump
faster = {}
for shape in SHAPES:
    segments, blocks = plan(shape)
    np.random.set_state(start)
    first = device_leg(shape, 0)[0]  # (the first segmented draw of the shape: its polynomials are made here)
    host_leg(shape), device_leg(shape, -1)  # warm-up: page-locked staging buffers, the pool's blocks
    hs, os_, ss, same = [], [], [], True
    for _ in range(REPS):
        states, kepts = [], []
        for leg, ts in ((host_leg, hs), (lambda sh: device_leg(sh, -1), os_), (lambda sh: device_leg(sh, 0), ss)):
            np.random.set_state(start)
            dt, kept = leg(shape)
            ts.append(dt), kepts.append(kept), states.append(np.random.get_state())
        same = same and kepts[0] == kepts[1] == kepts[2] and all(
            np.array_equal(states[0][1], s[1]) and states[0][2:] == s[2:] for s in states[1:])
    n = shape[0] * shape[1]
    faster[n] = med(ss) < med(hs)
    line = (f"{shape[0]:>8} x {shape[1]:<4} ({n:>10} elements), plan {segments} x {blocks} blocks: host {med(hs):.6f}  one-wg "
            f"{med(os_):.6f}  segmented {med(ss):.6f}  host / segmented {med(hs) / med(ss):.2f}  one-wg / segmented "
            f"{med(os_) / med(ss):.2f}  ({1e9 * med(ss) / n:.3f} ns per element segmented, {1e9 * med(hs) / n:.2f} on the host)")
    if segments > 1:
        proxy = (PROXY_BLOCKS * segments - 1, 312)  # `segments` segments of PROXY_BLOCKS blocks
        assert blocks_of(proxy) == PROXY_BLOCKS * segments
        device_leg(proxy, PROXY_BLOCKS)
        jumps = timed(proxy, start, PROXY_BLOCKS, REPS) - one
        line += (f"; set-up once {max(first - med(ss), 0.0):.6f}, jump launches per draw {jumps:.6f} "
                 f"(a draw of one segment of {PROXY_BLOCKS} blocks {one:.6f})")
    else:
        line += "; one segment: no polynomial, no jump launch (the segmented leg is the one-workgroup kernel)"
    print(line + f"; counts and generator state {'equal' if same else 'DIFFER'}")
sizes = sorted(faster)
gate = next((n for i, n in enumerate(sizes) if all(faster[m] for m in sizes[i:])), None)
if gate is None:
    print(f"the device leg is the faster one at no measured size from which it stays so: the gate belongs above {sizes[-1]}")
else:
    print(f"smallest measured size from which the device leg is the faster one at every larger measured size: {gate}")

print(f"segment count sweep (dmf_mask_draw_segments with blocks_per_segment = ceil(blocks / segments)); medians of {REPS}, seconds per "
      f"mask, polynomials made beforehand")
for shape in SWEEP_SHAPES:
    cells = []
    for w in SWEEP_SEGMENTS:
        c = (blocks_of(shape) + w - 1) // w
        if c < 1 or (blocks_of(shape) + c - 1) // c > L.MASK_DRAW_MAX_SEGMENTS:
            continue
        np.random.set_state(start)
        device_leg(shape, c)
        cells.append(f"{(blocks_of(shape) + c - 1) // c} x {c}: {timed(shape, start, c, REPS):.6f}")
    print(f"{shape[0]:>8} x {shape[1]:<4} ({blocks_of(shape)} blocks)  " + "  ".join(cells))

for n, s in BCV_SHAPES:
    V, D, ref = synthetic(n, s)
    with Problem(ctx, V, D, ref) as problem:
        ctx.synchronize()
        out = {}
        for name, value in (("warm-up", 1 << 62), ("host draw", 1 << 62), ("device draw", 0)):
            ic.DEVICE_MASK_MIN_ELEMENTS = value
            t = time.perf_counter()
            total, u, alpha = ic.bicross_validation(V, N_U, D, T1, T2, 0.0, n_folds=FOLDS, seed=SEED, ref=ref,
                                                    init_option="uniform_", fraction=FRACTION, problem=problem)
            out[name] = (time.perf_counter() - t, total, u, alpha)
        (th, ph, uh, ah), (td, pd_, ud, ad) = out["host draw"], out["device draw"]
        same = ph == pd_ and np.array_equal(uh, ud) and np.array_equal(ah, ad)
        print(f"bicross_validation at {n} x {s}, {N_C}+{N_U} types, {FOLDS} folds x {T1} outer iterations: host draw {th:.3f} s "
              f"({th / FOLDS:.3f} per fold)  device draw {td:.3f} s ({td / FOLDS:.3f} per fold)  host / device {th / td:.2f}; "
              f"press sum and best factors {'equal' if same else 'DIFFER'}")
    del V, D, ref
