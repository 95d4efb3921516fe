"""The hold-out mask of a bi-cross-validation fold, drawn on the host against drawn on the device, in one process.

Per shape two legs, alternating, medians of the repetitions (seconds per mask):
  host    np.random.rand(N, S) < fraction, the count of ones, pack_mask, mask_to_device -- what a fold did before
  device  np.random.get_state, dmf_mask_draw, np.random.set_state (staging.draw_mask)
Both start from the same generator state every time; the counts and the generator afterwards are compared.
Then one bicross_validation call (uniform_, 4 known + 2 unknown types, 3 folds x 20 outer iterations, tol = 0) per large
shape with ic.DEVICE_MASK_MIN_ELEMENTS forced off and on, on one resident Problem.
   python tools/mask_draw_bench.py [repetitions]"""
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from demethify_amd import ic
from demethify_amd.device import Problem, get_context, pack_mask
from demethify_amd.staging import draw_mask, mask_to_device

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
SHAPES = [(350, 10), (10_000, 64), (100_000, 64), (1_000_000, 256)]
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


def device_leg(shape):
    t = time.perf_counter()
    bits, kept = draw_mask(shape, FRACTION, ctx)
    dt = time.perf_counter() - t
    bits.close()
    return dt, kept


def med(xs):
    return float(np.median(xs))


def synthetic(n, s):
    rs = np.random.RandomState(0)
    R = rs.beta(0.5, 0.5, size=(n, N_C + N_U))
    A = rs.dirichlet(np.ones(N_C + N_U), s).T
    D = rs.randint(1, 100, size=(n, s)).astype(np.int64)
    V = np.rint(D * np.clip(R @ A, 0, 1)) / D
    return V, D, np.ascontiguousarray(R[:, :N_C])


print(f"hold-out mask draw, fraction {FRACTION}: host leg (rand, compare, count, pack_mask, mask_to_device) against device leg "
      f"(get_state, dmf_mask_draw, set_state); medians of {REPS} alternating runs in one process, seconds per mask")
faster = {}
for shape in SHAPES:
    np.random.seed(SEED)
    start = np.random.get_state()
    host_leg(shape), device_leg(shape)  # warm-up: page-locked staging buffers, the pool's blocks, the code object
    hs, ds, same = [], [], True
    for _ in range(REPS):
        np.random.set_state(start)
        th, kh = host_leg(shape)
        sh = np.random.get_state()
        np.random.set_state(start)
        td, kd = device_leg(shape)
        sd = np.random.get_state()
        hs.append(th), ds.append(td)
        same = same and kh == kd and np.array_equal(sh[1], sd[1]) and sh[2:] == sd[2:]
    n = shape[0] * shape[1]
    faster[n] = med(ds) < med(hs)
    print(f"{shape[0]:>8} x {shape[1]:<4} ({n:>10} elements): host {med(hs):.6f}  device {med(ds):.6f}  host / device "
          f"{med(hs) / med(ds):.2f}  ({1e9 * med(ds) / n:.2f} ns per element on the device, {1e9 * med(hs) / n:.2f} on the host); "
          f"counts and generator state {'equal' if same else 'DIFFER'}")
sizes = sorted(faster)
gate = next((n for i, n in enumerate(sizes) if all(faster[m] for m in sizes[i:])), None)
if gate is None:
    print(f"the device leg is the faster one at no measured size from which it stays so: the gate belongs above {sizes[-1]}")
else:
    print(f"smallest measured size from which the device leg is the faster one at every larger measured size: {gate}")

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
