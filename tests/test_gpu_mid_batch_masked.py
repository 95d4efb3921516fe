"""Hold-out masks in the mid-size batch (Problem.solve_many_mid_masked / dmf_solve_mid_masked, several workgroups per fold)
against the numpy oracle on (V * m, D * m) -- never against another device path.  Bars: those of
tests/test_gpu_small_batch_masked.py (u and alpha max-abs 1e-8, cost relative 1e-9, stop iteration equal, the hold-out sum
against numpy on the RETURNED iterate to 1e-11 relative, the fold error against the oracle's to conftest.PARITY_RTOL, n_test
equal).  Every natural-stop case first shows on the oracle's own cost trace that no stop test is decided by less than
1e-4 tol, and that at least one solve's kept maximum count differs from the full one.

Mask b is RandomState(1000 + b).rand(N, S) < f_b with f_b cycling (0.3, 0.5, 0.9); the init is uniform_ with seed 1 + b,
tol 1e-2, 20 inner steps; the data are osol.synthetic_problem(N, S, n_c, n_u, seed=3).  The shapes are the smallest that
reach each edge at the default 256 rows per workgroup."""
import functools

import numpy as np
import pandas as pd
import pytest

from oracle import drivers as odrv
from oracle import solver as osol

from conftest import PARITY_RTOL, UPSTREAM

pytestmark = pytest.mark.gpu

TIGHT = 1e-8
COST_RTOL = 1e-9
HOLDOUT_RTOL = 1e-11
TOL, T2 = 1e-2, 20
MIN_MARGIN = 1e-4
FAST = osol.simplex_project_columns_fast
FRACTIONS = (0.3, 0.5, 0.9)
PARTIAL, UNSUPERVISED = 0, 1

CASES = {  # name -> ((N, S), n_c, n_u, B, the slabs W at 256 rows, the oracle's iterations)
    "300x9 6+1": ((300, 9), 6, 1, 3, 2, (72, 52, 54)),          # W = 2, a ragged slab of 44 rows
    "770x13 3+2": ((770, 13), 3, 2, 3, 4, (90, 96, 66)),        # W = 4, a two-row last slab, two mask bytes, padding bits
    "520x64 12+4": ((520, 64), 12, 4, 3, 3, (351, 173, 203)),   # K = 16, S = 64, 8 mask bytes per row, W = 3
    "1030x7 0+3": ((1030, 7), 0, 3, 3, 5, (71, 97, 75)),        # unsupervised, W = 5
    "600x10 5+2 empty slab": ((600, 10), 5, 2, 3, 3, (149, 116, 94)),  # rows 256..511 held out in every mask: slab 1 keeps nothing
    "4100x5 2+1": ((4100, 5), 2, 1, 2, 17, (80, 44)),           # W = 17: more slabs than a slab-sum loop is likely to unroll
}
SMALL = "300x9 6+1"  # the problem of the bit-for-bit properties


def stop_margin(cf_start, trace, tol):
    """min_j ||cf_j - cf_{j-1}| - tol| / tol over the oracle's stop tests."""
    cf = np.concatenate([[cf_start], trace])
    return float(np.min(np.abs(np.abs(np.diff(cf)) - tol)) / tol)


def masks_for(N, S, B, first=0):
    return np.stack([np.random.RandomState(1000 + b).rand(N, S) < FRACTIONS[b % 3] for b in range(first, first + B)])


def holdout_numpy(V, Rt, u, alpha, m):
    R = np.hstack((Rt, u)) if Rt is not None else u
    return float(np.linalg.norm((V - R @ alpha) * ~m, "fro") ** 2)


def init_on(V, D, Rt, n_u, m, seed):
    """(u0, R or None, alpha0) of the fold: uniform_ on the masked data."""
    if Rt is not None:
        return osol.init_partial("uniform_", V * m, D * m, Rt, n_u, seed=seed)
    u0, a0 = osol.init_unsupervised("uniform_", V * m, n_u, seed=seed)
    return u0, None, a0


def oracle_run(V, D, Rt, n_u, m, seed, n_iter1, tol):
    """The oracle on (V * m, D * m) -> dict(u0, a0, u, alpha, trace, cf_start, sum_sq): one fold of ic.py:58-89."""
    Vm, Dm = V * m, D * m
    trace = []
    u0, R, a0 = init_on(V, D, Rt, n_u, m, seed)
    if Rt is not None:
        cf_start = osol.weighted_cost(Vm, R, a0, Dm)
        u, alpha = osol.solve_partial(u0.copy(), R, a0.copy(), Vm, Dm, Rt, n_u, n_iter1, T2, tol, project=FAST, trace=trace)
    else:
        cf_start = osol.weighted_cost(Vm, u0, a0, Dm)
        u, alpha = osol.solve_unsupervised(Vm, n_u, Dm, "uniform_", n_iter1, T2, tol, init=(u0.copy(), a0.copy()), project=FAST,
                                           trace=trace)
    out = dict(u0=u0, a0=a0, u=u, alpha=alpha, trace=trace, cf_start=cf_start, sum_sq=holdout_numpy(V, Rt, u, alpha, m))
    for x in (u0, a0, u, alpha):
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def data(name):
    (N, S), n_c, n_u, B, _, _ = CASES[name]
    V, D, Rt = osol.synthetic_problem(N, S, n_c, n_u, seed=3)
    Rt = Rt if n_c else None
    masks = masks_for(N, S, B)
    if "empty slab" in name:
        masks[:, 256:512, :] = False
    for x in (V, D, masks) + ((Rt,) if Rt is not None else ()):
        x.setflags(write=False)
    return V, D, Rt, masks


@functools.lru_cache(maxsize=None)
def natural_runs(name):
    """The oracle's runs of a case to their natural stop, computed once and shared."""
    V, D, Rt, masks = data(name)
    return [oracle_run(V, D, Rt, CASES[name][2], masks[b], 1 + b, 10000, TOL) for b in range(len(masks))]


def mode_of(Rt):
    return PARTIAL if Rt is not None else UNSUPERVISED


def each(out, b):
    return tuple(x[b] for x in out)


def same(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x, y))


def hold(got, V, Rt, m, run):
    u, alpha, cost, iters, sum_sq, n_test = got
    want_cost, want_iters = run["trace"][-1], len(run["trace"])
    mine = holdout_numpy(V, Rt, u, alpha, m)
    n_zero = int((~m).sum())
    print(f"max|u - oracle| = {np.abs(u - run['u']).max():.3e}  max|alpha - oracle| = {np.abs(alpha - run['alpha']).max():.3e}  "
          f"cost rel = {abs(cost - want_cost) / want_cost:.3e}  iterations {iters} / {want_iters}  "
          f"hold-out vs numpy on the returned iterate rel = {abs(sum_sq - mine) / mine:.3e}  "
          f"fold error vs oracle rel = {abs(sum_sq - run['sum_sq']) / run['sum_sq']:.3e}  n_test {n_test} / {n_zero}")
    assert int(iters) == want_iters
    assert np.abs(u - run["u"]).max() <= TIGHT
    assert np.abs(alpha - run["alpha"]).max() <= TIGHT
    assert float(cost) == pytest.approx(want_cost, rel=COST_RTOL)
    assert int(n_test) == n_zero
    assert float(sum_sq) == pytest.approx(mine, rel=HOLDOUT_RTOL)
    assert float(sum_sq) / int(n_test) == pytest.approx(run["sum_sq"] / n_zero, rel=PARITY_RTOL)


def bits_with_padding_set(masks):
    """pack_mask's layout with every padding bit set to 1: the library must ignore them."""
    bits = np.packbits(masks, axis=2, bitorder="little")
    S = masks.shape[2]
    if S % 8:
        bits[:, :, -1] |= np.uint8((0xFF << (S % 8)) & 0xFF)
    return bits


def stacked(runs):
    # (C order: alpha0 is a transposed Dirichlet draw, and np.stack keeps its inputs' memory order)
    return np.ascontiguousarray(np.stack([r["u0"] for r in runs])), np.ascontiguousarray(np.stack([r["a0"] for r in runs]))


# ---- 1. the cases against the oracle ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_masked_solves_match_the_oracle(ctx, name):
    from demethify_amd.device import Problem, mid_solve_plan

    V, D, Rt, masks = data(name)
    runs = natural_runs(name)
    for b, r in enumerate(runs):
        margin = stop_margin(r["cf_start"], r["trace"], TOL)
        kept_max = int((D * masks[b]).max())
        print(f"solve {b}: oracle stops after {len(r['trace'])}, margin {margin:.2e}, kept max count {kept_max} / {int(D.max())}")
        assert margin >= MIN_MARGIN
    assert tuple(len(r["trace"]) for r in runs) == CASES[name][5]
    assert any(int((D * m).max()) != int(D.max()) for m in masks)  # d is the maximum over the KEPT elements
    assert mid_solve_plan(V.shape[0], V.shape[1])[:2] == (256, CASES[name][4])
    if "empty slab" in name:
        assert not masks[:, 256:512].any() and masks[:, :256].any() and masks[:, 512:].any()
    u0s, a0s = stacked(runs)
    with Problem(ctx, V, D, Rt) as p:
        out = p.solve_many_mid_masked(u0s, a0s, bits_with_padding_set(masks), mode_of(Rt), 10000, T2, TOL)
    for b, r in enumerate(runs):
        hold(each(out, b), V, Rt, masks[b], r)


@pytest.mark.parametrize("name,rows", [(name, 0) for name in CASES] + [("770x13 3+2", 512)])
def test_first_solve_with_fixed_work(ctx, name, rows):
    """n_iter1 = 7, tol = 0: the stop test is never met, exactly 7 outer iterations on both sides.  Once more at 770 x 13 with
    512 rows per workgroup (W = 2)."""
    from demethify_amd.device import Problem, mid_solve_plan

    V, D, Rt, masks = data(name)
    run = oracle_run(V, D, Rt, CASES[name][2], masks[0], 1, 7, 0.0)
    assert len(run["trace"]) == 7
    if rows:
        assert mid_solve_plan(V.shape[0], V.shape[1], rows)[:2] == (512, 2)
    with Problem(ctx, V, D, Rt) as p:
        out = p.solve_many_mid_masked(run["u0"][None], run["a0"][None], bits_with_padding_set(masks[:1]), mode_of(Rt), 7, T2, 0.0,
                                      rows_per_workgroup=rows)
    hold(each(out, 0), V, Rt, masks[0], run)


# ---- 2. properties, bit for bit, on 300 x 9 -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_problem(ctx):
    from demethify_amd.device import Problem

    V, D, Rt, _ = data(SMALL)
    with Problem(ctx, V, D, Rt) as p:
        yield p


def test_all_ones_masks_are_the_unmasked_solves_bit_for_bit(small_problem):
    V, D, Rt, _ = data(SMALL)
    inits = [osol.init_partial("uniform_", V, D, Rt, 1, seed=s) for s in (1, 2, 3)]
    u0s, a0s = np.ascontiguousarray(np.stack([i[0] for i in inits])), np.ascontiguousarray(np.stack([i[2] for i in inits]))
    plain = small_problem.solve_many_mid(u0s, a0s, PARTIAL, 10000, T2, TOL)
    masked = small_problem.solve_many_mid_masked(u0s, a0s, np.ones((3,) + V.shape, dtype=bool), PARTIAL, 10000, T2, TOL)
    assert same(plain, masked[:4])
    assert all(int(i) > 1 for i in plain[3])
    assert np.array_equal(masked[4], np.zeros(3)) and np.array_equal(masked[5], np.zeros(3, dtype=np.int64))


def test_a_masked_solve_depends_on_nothing_but_itself(small_problem):
    """Alone, and in slots 0, 7 and 39 of 40 among other masks and starts; with the stop flags read every 1, every 7 and by
    default; and once more: the same bits."""
    V, D, Rt, masks = data(SMALL)
    run = natural_runs(SMALL)[0]
    u0, a0, m = run["u0"][None], run["a0"][None], masks[:1]
    alone = small_problem.solve_many_mid_masked(u0, a0, m, PARTIAL, 10000, T2, TOL)
    assert int(alone[3][0]) == CASES[SMALL][5][0]
    others = masks_for(V.shape[0], V.shape[1], 40, first=50)
    starts = [init_on(V, D, Rt, 1, others[b], 51 + b) for b in range(40)]
    u0s = np.ascontiguousarray(np.stack([s[0] for s in starts]))
    a0s = np.ascontiguousarray(np.stack([s[2] for s in starts]))
    for slot in (0, 7, 39):
        u0s[slot], a0s[slot], others[slot] = u0[0], a0[0], m[0]
    among = small_problem.solve_many_mid_masked(u0s, a0s, others, PARTIAL, 10000, T2, TOL)
    for slot in (0, 7, 39):
        assert same(each(alone, 0), each(among, slot))
    assert not np.array_equal(among[0][0], among[0][1])  # (the other slots are other solves)
    for every in (1, 7):
        assert same(alone, small_problem.solve_many_mid_masked(u0, a0, m, PARTIAL, 10000, T2, TOL, check_every=every))
    assert same(among, small_problem.solve_many_mid_masked(u0s, a0s, others, PARTIAL, 10000, T2, TOL))


def raw_call(problem, B, bits, u0s, a0s, n_u, mode, n_iter1, flags, out_u, out_alpha, cost, iters, sum_sq, n_test):
    from demethify_amd.device import _ptr

    return problem._lib.dmf_solve_mid_masked(problem.ctx._h, problem._h, B, _ptr(bits), _ptr(u0s), _ptr(a0s), n_u, mode, n_iter1,
                                             T2, TOL, 0, 0, flags, _ptr(out_u), _ptr(out_alpha), _ptr(cost), _ptr(iters),
                                             _ptr(sum_sq), _ptr(n_test))


def test_device_pointers_give_the_host_routes_bits(small_problem):
    import torch
    from demethify_amd import _lib as L

    V, _, _, masks = data(SMALL)
    u0s, a0s = stacked(natural_runs(SMALL))
    want = small_problem.solve_many_mid_masked(u0s, a0s, masks, PARTIAL, 10000, T2, TOL)
    dev = torch.device("cuda", small_problem.ctx.device)
    bits = torch.from_numpy(np.packbits(masks, axis=2, bitorder="little")).to(dev)
    d_u0, d_a0 = torch.from_numpy(u0s).to(dev), torch.from_numpy(a0s).to(dev)
    d_u = torch.empty((3, V.shape[0], 1), dtype=torch.float64, device=dev)
    alpha, cost, iters = np.empty_like(a0s), np.empty(3), np.empty(3, dtype=np.int64)
    sum_sq, n_test = np.empty(3), np.empty(3, dtype=np.int64)
    torch.cuda.synchronize(dev)
    status = raw_call(small_problem, 3, bits, d_u0, d_a0, 1, PARTIAL, 10000, L.DMF_PTR_DEVICE, d_u, alpha, cost, iters, sum_sq, n_test)
    assert status == L.DMF_OK
    small_problem.ctx.synchronize()
    assert same(want, (d_u.cpu().numpy(), alpha, cost, iters, sum_sq, n_test))
    assert np.array_equal(d_u0.cpu().numpy(), u0s) and np.array_equal(d_a0.cpu().numpy(), a0s)  # inputs are never written


# ---- 3. refusals -------------------------------------------------------------------------------------------------------

def test_a_mask_that_keeps_nothing_is_refused_before_any_solve_starts(small_problem):
    from demethify_amd import _lib as L

    V, _, _, masks = data(SMALL)
    u0s, a0s = stacked(natural_runs(SMALL))
    m = masks.copy()
    m[1] = False
    bits = bits_with_padding_set(m)  # (the padding bits of the empty mask are 1: they are not kept elements)
    outs = [np.full((3, V.shape[0], 1), -7.0), np.full(a0s.shape, -7.0), np.full(3, -7.0), np.full(3, -7, dtype=np.int64),
            np.full(3, -7.0), np.full(3, -7, dtype=np.int64)]
    status = raw_call(small_problem, 3, bits, u0s, a0s, 1, PARTIAL, 10000, 0, *outs)
    assert status == L.DMF_ERR_BAD_ARG
    assert all(np.all(x == -7) for x in outs)  # the sentinel: no output was touched
    with pytest.raises(L.DemethifyHipError) as e:
        small_problem.solve_many_mid_masked(u0s, a0s, m, PARTIAL, 10000, T2, TOL)
    assert e.value.status == L.DMF_ERR_BAD_ARG
    # a null train_bits
    status = raw_call(small_problem, 3, None, u0s, a0s, 1, PARTIAL, 10000, 0, *outs)
    assert status == L.DMF_ERR_BAD_ARG and all(np.all(x == -7) for x in outs)


def test_a_masked_problem_and_a_shape_outside_the_envelope_are_refused(small_problem):
    from demethify_amd import _lib as L

    V, _, _, masks = data(SMALL)
    u0s, a0s = stacked(natural_runs(SMALL)[:2])
    with small_problem.masked(masks[0]) as held:
        with pytest.raises(L.DemethifyHipError) as e:
            held.solve_many_mid_masked(u0s, a0s, masks[:2], PARTIAL, 5, T2, 0.0)
    assert e.value.status == L.DMF_ERR_BAD_ARG
    with pytest.raises(L.DemethifyHipError) as e:  # n_u = 5
        small_problem.solve_many_mid_masked(np.full((1, V.shape[0], 5), 0.5), np.full((1, 11, V.shape[1]), 0.1), masks[:1], PARTIAL,
                                            5, T2, 0.0)
    assert e.value.status == L.DMF_ERR_UNSUPPORTED


# ---- 4. drivers (uniform_, tol 1e-2, 20 inner steps) on the 300 x 9 and 770 x 13 data ------------------------------------

DRIVER_DATA = ("300x9 6+1", "770x13 3+2")


@functools.lru_cache(maxsize=None)
def oracle_fold(name, n_u, mask_bytes, seed):
    """One fold on the oracle, remembered by its mask: upstream's reseeding makes most folds the same one."""
    V, D, Rt, _ = data(name)
    return oracle_run(V, D, Rt, n_u, np.frombuffer(mask_bytes, dtype=bool).reshape(V.shape), seed, 10000, TOL)


def oracle_bicross_validation(name, n_u, n_folds, seed, fraction=0.3):
    """ic.py:58-89 restated on the oracle solver -> (total_press, u, alpha, winning fold among the folds that ran, per-fold
    errors, margins, folds skipped)."""
    V, D, Rt, _ = data(name)
    np.random.seed(seed)
    total, best, min_error, errors, margins, skipped = 0, (None, None, None), float("inf"), [], [], 0
    for _ in range(n_folds):
        m = np.random.rand(*V.shape) < fraction
        if np.sum(~m) == 0 or np.sum(m) == 0:
            skipped += 1
            continue
        # the initialiser reseeds, as upstream's, and the next mask follows its draws: it runs for every fold, the solve
        # only for a mask not seen before
        osol.init_partial("uniform_", V * m, D * m, Rt, n_u, seed=seed)
        r = oracle_fold(name, n_u, m.tobytes(), seed)
        margins.append(stop_margin(r["cf_start"], r["trace"], TOL))
        error = r["sum_sq"] / np.sum(~m)
        if error < min_error:
            min_error, best = error, (r["u"], r["alpha"], len(errors))
        errors.append(error)
        total += error
    return total, best[0], best[1], best[2], errors, margins, skipped


def skip_second_mask(monkeypatch, shape):
    """np.random.rand gives all ones on the second draw of a mask's shape: that fold keeps nothing and is skipped, on the
    oracle's side and on the driver's alike (both draw their masks through it)."""
    real, seen = np.random.rand, []

    def rand(*dims):
        if dims == tuple(shape):
            seen.append(dims)
            if len(seen) == 2:
                return np.ones(dims)
        return real(*dims)

    monkeypatch.setattr(np.random, "rand", rand)
    return seen


@pytest.mark.parametrize("name", DRIVER_DATA)
def test_bicross_validation_mid_matches_the_restated_loop(ctx, name, monkeypatch):
    from demethify_amd import ic
    from demethify_amd.device import Problem

    V, D, Rt, _ = data(name)
    n_u = CASES[name][2]
    with monkeypatch.context() as mp:
        skip_second_mask(mp, V.shape)
        want_total, want_u, want_alpha, winner, errors, margins, skipped = oracle_bicross_validation(name, n_u, 5, 1)
    print(f"{name}: oracle fold errors {[f'{e:.6f}' for e in errors]}, winner {winner}, margins {min(margins):.2e}, skipped {skipped}")
    assert min(margins) >= MIN_MARGIN
    # fold 1 is skipped; upstream's reseeding initialiser makes folds 2..4 one mask, so their errors are equal and the first
    # strict minimum is the first of them or fold 0
    assert skipped == 1 and len(errors) == 4 and errors[1] == errors[2] == errors[3]
    assert winner == (0 if errors[0] < errors[1] else 1)
    seen = []
    real = Problem.solve_many_mid_masked

    def spy(self, *a, **k):
        out = real(self, *a, **k)
        seen.append(out)
        return out

    monkeypatch.setattr(Problem, "solve_many_mid_masked", spy)
    monkeypatch.setattr(Problem, "solve_many_masked", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the one-launch batch")))
    draws = skip_second_mask(monkeypatch, V.shape)
    total, u, alpha = ic.bicross_validation(V, n_u, D, 10000, T2, TOL, n_folds=5, seed=1, ref=Rt, init_option="uniform_",
                                            fraction=0.3, batched=True, batch_kernel="mid")
    assert len(draws) == 5 and len(seen) == 1 and len(seen[0][0]) == 4
    got_errors = seen[0][4] / seen[0][5]
    print(f"device fold errors {[f'{e:.6f}' for e in got_errors]}, total rel {abs(total - want_total) / want_total:.3e}")
    assert total == pytest.approx(want_total, rel=PARITY_RTOL)
    for b in (2, 3):  # the equal folds come out with equal bits
        assert same(each(seen[0], 1), each(seen[0], b))
    assert int(np.argmin(got_errors)) == winner  # (argmin: the first of equal minima, as the strict '<')
    assert np.array_equal(u, seen[0][0][winner]) and np.array_equal(alpha, seen[0][1][winner])
    assert np.abs(u - want_u).max() <= TIGHT and np.abs(alpha - want_alpha).max() <= TIGHT


def test_bicross_validation_mid_with_every_fold_skipped_and_a_bad_kernel_name(ctx, monkeypatch):
    from demethify_amd import ic
    from demethify_amd.device import Problem

    V, D, Rt, _ = data(SMALL)
    monkeypatch.setattr(Problem, "solve_many_mid_masked", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a solve")))
    # fraction 1: every mask keeps everything, upstream skips every fold and returns its initial values
    assert ic.bicross_validation(V, 1, D, 10000, T2, TOL, n_folds=3, seed=1, ref=Rt, fraction=1.0, batched=True,
                                 batch_kernel="mid") == (0, None, None)
    with pytest.raises(ValueError, match="batch_kernel"):
        ic.bicross_validation(V, 1, D, 10000, T2, TOL, n_folds=3, seed=1, ref=Rt, batched=True, batch_kernel="large")


@pytest.mark.parametrize("name", DRIVER_DATA)
def test_evaluate_best_ic_mid_ccc_scores_are_the_oracles(ctx, name, monkeypatch):
    from demethify_amd import ic
    from demethify_amd.device import Problem

    V, D, Rt, _ = data(name)
    want = []
    for n_u in (1, 2):
        runs = [odrv.run_one(V, D, Rt, n_u, "uniform_", 1 + r, 10000, T2, TOL, project=FAST)[2] for r in range(4)]
        for a in runs:  # no dominant cell type is a near tie: the labels, and so the score, are exactly the oracle's
            top = np.sort(a, axis=0)
            assert (top[-1] - top[-2]).min() >= 1e-6
        want.append(-ic.compute_ccc(runs))
    calls = []
    real = Problem.solve_many_mid
    monkeypatch.setattr(Problem, "solve_many_mid", lambda self, *a, **k: calls.append(len(a[0])) or real(self, *a, **k))
    monkeypatch.setattr(Problem, "solve_many", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the one-launch batch")))
    monkeypatch.setattr(ic, "Solver", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a per-solve Solver")))
    u, alpha, n_best, scores = ic.evaluate_best_ic(V, Rt, D, "uniform_", "CCC", 1, 10000, T2, TOL, n_restarts=4,
                                                   n_u_values=(1, 2), batched=True, batch_kernel="mid")
    assert calls == [4, 4]
    print(f"CCC scores {scores} oracle {want}")
    assert list(scores) == want
    assert n_best == (1, 2)[int(np.argmin(want))] and u.shape == (V.shape[0], n_best)


def test_evaluate_best_ic_mid_bcv_goes_through_the_masked_entry(ctx, monkeypatch):
    from demethify_amd import ic
    from demethify_amd.device import Problem

    V, D, Rt, _ = data(SMALL)
    want = [oracle_bicross_validation(SMALL, n_u, 4, 1) for n_u in (1, 2)]
    assert min(min(w[5]) for w in want) >= MIN_MARGIN
    calls = []
    real = Problem.solve_many_mid_masked
    monkeypatch.setattr(Problem, "solve_many_mid_masked", lambda self, *a, **k: calls.append(len(a[0])) or real(self, *a, **k))
    monkeypatch.setattr(Problem, "solve_many_masked", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the one-launch batch")))
    monkeypatch.setattr(Problem, "masked", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a masked problem per fold")))
    u, alpha, n_best, scores = ic.evaluate_best_ic(V, Rt, D, "uniform_", "BCV", 1, 10000, T2, TOL, n_restarts=4,
                                                   n_u_values=(1, 2), batched=True, batch_kernel="mid")
    assert calls == [4, 4]
    print(f"BCV scores {scores} oracle {[w[0] for w in want]}")
    for got, w in zip(scores, want):
        assert got == pytest.approx(w[0], rel=PARITY_RTOL)
    best = int(np.argmin([w[0] for w in want]))
    assert n_best == (1, 2)[best]
    assert np.abs(u - want[best][1]).max() <= TIGHT and np.abs(alpha - want[best][2]).max() <= TIGHT


def test_evaluate_best_ic_mid_aic_and_the_candidate_outside_the_envelope(ctx, monkeypatch, capsys):
    from demethify_amd import ic
    from demethify_amd.device import Problem

    V, D, Rt, _ = data(SMALL)
    values = (1, 2, 3, 4, 5)
    _, _, per_solve_best, per_solve = ic.evaluate_best_ic(V, Rt, D, "uniform_", "AIC", 1, 10000, T2, TOL, n_u_values=values)
    _, _, want_best, want = odrv.ic_sweep(V, Rt, D, "uniform_", "AIC", 1, 10000, T2, TOL, n_u_values=values, project=FAST)
    capsys.readouterr()
    batch, solvers = [], []
    real_many, real_solver = Problem.solve_many_mid, ic.Solver
    monkeypatch.setattr(Problem, "solve_many_mid", lambda self, *a, **k: batch.append(a[0].shape) or real_many(self, *a, **k))
    monkeypatch.setattr(Problem, "solve_many", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the one-launch batch")))

    def solver(problem, u0, a0, mode):
        solvers.append(np.asarray(u0).reshape(V.shape[0], -1).shape[1])
        return real_solver(problem, u0, a0, mode)

    monkeypatch.setattr(ic, "Solver", solver)
    u, alpha, n_best, scores = ic.evaluate_best_ic(V, Rt, D, "uniform_", "AIC", 1, 10000, T2, TOL, n_u_values=values, batched=True,
                                                   batch_kernel="mid")
    print(f"AIC scores {scores} per-solve {per_solve} oracle {want}")
    assert sorted(s[2] for s in batch) == [1, 2, 3, 4] and all(s[0] == 1 for s in batch)  # batches of one
    assert solvers == [5]  # candidate 5 took the per-solve path
    out = capsys.readouterr().out
    assert out.count("take the per-solve path") == 1 and "n_u = [5]" in out and "mid-size batch's envelope" in out
    for got, w, o in zip(scores, per_solve, want):
        assert got == pytest.approx(w, rel=1e-9)
        assert got == pytest.approx(o, rel=1e-9)
    assert n_best == per_solve_best == want_best


def test_command_line_mid_ic_reaches_the_masked_entry(tmp_path, monkeypatch):
    """DEMETHIFY_BATCH_MID_IC=1 --ic BCV 5 1 2 on the reference's example (350 x 10: two slabs) with the gates opened: the folds
    go through solve_many_mid_masked and the tables are those of the run without the variable, to 1e-8."""
    from demethify_amd import demethify, ic
    from demethify_amd.device import Problem

    monkeypatch.setattr(ic, "MID_BATCH_IC_MIN_ELEMENTS", 1)
    monkeypatch.setattr(ic, "MID_BATCH_IC_MAX_ELEMENTS", 1 << 23)
    monkeypatch.setattr(ic, "MID_BATCH_IC_CRITERIA", ("BCV",))
    calls = []
    real = Problem.solve_many_mid_masked
    monkeypatch.setattr(Problem, "solve_many_mid_masked", lambda self, *a, **k: calls.append(len(a[0])) or real(self, *a, **k))
    monkeypatch.delenv("DEMETHIFY_BATCH", raising=False)
    monkeypatch.delenv("DEMETHIFY_BATCH_MID", raising=False)
    samples = [str(UPSTREAM / "output_gen" / f"sample{i}.bed") for i in range(1, 11)]
    results = {}
    for name, value in (("plain", None), ("mid", "1")):
        if value is None:
            monkeypatch.delenv("DEMETHIFY_BATCH_MID_IC", raising=False)
        else:
            monkeypatch.setenv("DEMETHIFY_BATCH_MID_IC", value)
        out = tmp_path / name
        demethify.main(["--ref", str(UPSTREAM / "output_gen" / "ref_matrix.bed"), "--methfreq", *samples, "--bedmethyl",
                        "--noprint", "--ic", "BCV", "5", "1", "2", "--outdir", str(out)])  # (defaults: uniform_, 1e-2, 10000 x 20)
        results[name] = [pd.read_csv(out / "celltypes_proportions.csv", index_col=0, float_precision="round_trip").values,
                         pd.read_csv(out / "methylation_profile_estimate.csv", float_precision="round_trip").values]
        if value is None:
            assert calls == []
    assert calls == [5, 5]
    for plain, mid in zip(results["plain"], results["mid"]):
        assert plain.shape == mid.shape
        assert np.abs(plain - mid).max() <= TIGHT
