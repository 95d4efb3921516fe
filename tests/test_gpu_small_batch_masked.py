"""Hold-out masks in the one-launch batch (Problem.solve_many_masked / dmf_solve_small_masked, one workgroup per fold)
against the numpy oracle on (V * m, D * m) -- never against the per-solve device path.  Bars: those of
tests/test_gpu_small_batch.py (u and alpha max-abs 1e-8, cost relative 1e-9, stop iteration equal); the hold-out sum against
numpy on the RETURNED iterate to 1e-11 relative (the bar of test_gpu_kat.py::test_cost_matches_oracle: it isolates
k_small_holdout), the fold error against the oracle's to conftest.PARITY_RTOL (the iterate's 1e-8 allows about 3e-6 on
residuals of about 0.09 rms).  Every natural-stop case first shows on the oracle's own cost trace that no stop test is
decided by less than 1e-4 tol.

Mask b is RandomState(1000 + b).rand(N, S) < f_b with f_b cycling (0.3, 0.5, 0.9); the init is uniform_ with seed 1 + b,
tol 1e-2, 20 inner steps.  The kept maximum count differs from the full one in most solves, so a kernel that takes d from
the unmasked counts fails these."""
import functools

import numpy as np
import pandas as pd
import pytest

from oracle import drivers as odrv
from oracle import solver as osol

from conftest import PARITY_RTOL, UPSTREAM, load_toy

pytestmark = pytest.mark.gpu

TIGHT = 1e-8
COST_RTOL = 1e-9
HOLDOUT_RTOL = 1e-11
TOL, T2 = 1e-2, 20
MIN_MARGIN = 1e-4
FAST = osol.simplex_project_columns_fast
FRACTIONS = (0.3, 0.5, 0.9)
PARTIAL, UNSUPERVISED = 0, 1

CASES = {  # name -> (data, n_c, n_u, B, the oracle's iterations)
    "toy 5+1": ("toy", 5, 1, 6, (80, 53, 34, 117, 67, 34)),
    "toy 5+2": ("toy", 5, 2, 6, (186, 162, 109, 123, 218, 123)),
    "toy 0+4": ("toy", 0, 4, 3, (106, 143, 102)),
    "77x13 3+2": ((77, 13), 3, 2, 3, (66, 74, 45)),        # S no multiple of 8: two bytes per row, three padding bits
    "40x64 12+4": ((40, 64), 12, 4, 3, (207, 238, 174)),   # K = 16, S = 64: the largest LDS layout, 8 mask bytes per row
    "1030x7 0+3": ((1030, 7), 0, 3, 3, (71, 97, 75)),      # more than 4 x 256 rows: trips and tail of the rows-in-flight loops
    "300x9 6+1": ((300, 9), 6, 1, 3, (72, 52, 54)),        # 16 rows of 16 samples per 256 threads
}
SYNTHETIC = [name for name, c in CASES.items() if c[0] != "toy"]


def stop_margin(cf_start, trace, tol):
    """min_j ||cf_j - cf_{j-1}| - tol| / tol over the oracle's stop tests."""
    cf = np.concatenate([[cf_start], trace])
    return float(np.min(np.abs(np.abs(np.diff(cf)) - tol)) / tol)


def masks_for(N, S, B):
    return np.stack([np.random.RandomState(1000 + b).rand(N, S) < FRACTIONS[b % 3] for b in range(B)])


def holdout_numpy(V, Rt, u, alpha, m):
    R = np.hstack((Rt, u)) if Rt is not None else u
    return float(np.linalg.norm((V - R @ alpha) * ~m, "fro") ** 2)


def oracle_run(V, D, Rt, n_u, m, seed, n_iter1, tol):
    """The oracle on (V * m, D * m) -> dict(u0, a0, u, alpha, trace, cf_start, sum_sq): one fold of ic.py:58-89."""
    Vm, Dm = V * m, D * m
    trace = []
    if Rt is not None:
        u0, R, a0 = osol.init_partial("uniform_", Vm, Dm, Rt, n_u, seed=seed)
        cf_start = osol.weighted_cost(Vm, R, a0, Dm)
        u, alpha = osol.solve_partial(u0.copy(), R, a0.copy(), Vm, Dm, Rt, n_u, n_iter1, T2, tol, project=FAST, trace=trace)
    else:
        u0, a0 = osol.init_unsupervised("uniform_", Vm, n_u, seed=seed)
        cf_start = osol.weighted_cost(Vm, u0, a0, Dm)
        u, alpha = osol.solve_unsupervised(Vm, n_u, Dm, "uniform_", n_iter1, T2, tol, init=(u0.copy(), a0.copy()), project=FAST,
                                           trace=trace)
    out = dict(u0=u0, a0=a0, u=u, alpha=alpha, trace=trace, cf_start=cf_start, sum_sq=holdout_numpy(V, Rt, u, alpha, m))
    for x in (u0, a0, u, alpha):
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def data(name):
    source, n_c, n_u, B, _ = CASES[name]
    if source == "toy":
        V, D, ref, _ = load_toy()
        Rt = ref if n_c else None
    else:
        V, D, Rt = osol.synthetic_problem(source[0], source[1], n_c, n_u, seed=3)
        Rt = Rt if n_c else None
    masks = masks_for(V.shape[0], V.shape[1], B)
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
    from demethify_amd.device import Problem

    V, D, Rt, masks = data(name)
    runs = natural_runs(name)
    for b, r in enumerate(runs):
        margin = stop_margin(r["cf_start"], r["trace"], TOL)
        kept_max = int((D * masks[b]).max())
        print(f"solve {b}: oracle stops after {len(r['trace'])}, margin {margin:.2e}, kept max count {kept_max} / {int(D.max())}")
        assert margin >= MIN_MARGIN
    assert tuple(len(r["trace"]) for r in runs) == CASES[name][4]
    assert any(int((D * m).max()) != int(D.max()) for m in masks)  # d is the maximum over the KEPT elements
    u0s, a0s = stacked(runs)
    # the synthetic cases pass packed bits whose padding bits are 1, the toy cases bool masks
    form = bits_with_padding_set(masks) if name in SYNTHETIC else masks
    with Problem(ctx, V, D, Rt) as p:
        out = p.solve_many_masked(u0s, a0s, form, mode_of(Rt), 10000, T2, TOL)
    for b, r in enumerate(runs):
        hold(each(out, b), V, Rt, masks[b], r)


@pytest.mark.parametrize("name", SYNTHETIC)
def test_first_solve_with_fixed_work(ctx, name):
    """n_iter1 = 7, tol = 0: the stop test is never met, exactly 7 outer iterations on both sides."""
    from demethify_amd.device import Problem

    V, D, Rt, masks = data(name)
    run = oracle_run(V, D, Rt, CASES[name][2], masks[0], 1, 7, 0.0)
    assert len(run["trace"]) == 7
    with Problem(ctx, V, D, Rt) as p:
        out = p.solve_many_masked(run["u0"][None], run["a0"][None], bits_with_padding_set(masks[:1]), mode_of(Rt), 7, T2, 0.0)
    hold(each(out, 0), V, Rt, masks[0], run)


# ---- 2. properties, on toy 5+1 -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def toy_problem(ctx):
    from demethify_amd.device import Problem

    V, D, Rt, _ = data("toy 5+1")
    with Problem(ctx, V, D, Rt) as p:
        yield p


def same(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x, y))


def test_all_ones_masks_are_the_unmasked_solves_bit_for_bit(toy_problem):
    V, D, Rt, _ = data("toy 5+1")
    inits = [osol.init_partial("uniform_", V, D, Rt, 1, seed=s) for s in (1, 2, 3)]
    u0s, a0s = np.stack([i[0] for i in inits]), np.stack([i[2] for i in inits])
    plain = toy_problem.solve_many(u0s, a0s, PARTIAL, 10000, T2, TOL)
    masked = toy_problem.solve_many_masked(u0s, a0s, np.ones((3,) + V.shape, dtype=bool), PARTIAL, 10000, T2, TOL)
    assert same(plain, masked[:4])
    assert int(plain[3][0]) == 54  # (the reference's example stops where it always did)
    assert np.array_equal(masked[4], np.zeros(3)) and np.array_equal(masked[5], np.zeros(3, dtype=np.int64))


def test_a_masked_solve_depends_on_nothing_but_itself(toy_problem):
    """As B = 6, in reversed slots, each alone, and with 1, 7 and the default number of iterations per launch: the same bits."""
    _, _, _, masks = data("toy 5+1")
    u0s, a0s = stacked(natural_runs("toy 5+1"))
    want = toy_problem.solve_many_masked(u0s, a0s, masks, PARTIAL, 10000, T2, TOL)
    assert [int(i) for i in want[3]] == list(CASES["toy 5+1"][4])
    back = toy_problem.solve_many_masked(u0s[::-1], a0s[::-1], masks[::-1], PARTIAL, 10000, T2, TOL)
    assert same(want, [x[::-1] for x in back])
    for b in range(6):
        alone = toy_problem.solve_many_masked(u0s[b:b + 1], a0s[b:b + 1], masks[b:b + 1], PARTIAL, 10000, T2, TOL)
        assert same(each(want, b), each(alone, 0))
    for per_launch in (1, 7):
        cut = toy_problem.solve_many_masked(u0s, a0s, masks, PARTIAL, 10000, T2, TOL, iters_per_launch=per_launch)
        assert same(want, cut)


def raw_call(problem, B, bits, u0s, a0s, n_u, mode, n_iter1, flags, out_u, out_alpha, cost, iters, sum_sq, n_test):
    from demethify_amd.device import _ptr

    return problem._lib.dmf_solve_small_masked(problem.ctx._h, problem._h, B, _ptr(bits), _ptr(u0s), _ptr(a0s), n_u, mode, n_iter1,
                                               T2, TOL, 0, flags, _ptr(out_u), _ptr(out_alpha), _ptr(cost), _ptr(iters),
                                               _ptr(sum_sq), _ptr(n_test))


def test_device_pointers_give_the_host_routes_bits(toy_problem):
    import torch
    from demethify_amd import _lib as L

    V, _, _, masks = data("toy 5+1")
    u0s, a0s = stacked(natural_runs("toy 5+1"))
    want = toy_problem.solve_many_masked(u0s, a0s, masks, PARTIAL, 10000, T2, TOL)
    dev = torch.device("cuda", toy_problem.ctx.device)
    bits = torch.from_numpy(np.packbits(masks, axis=2, bitorder="little")).to(dev)
    d_u0, d_a0 = torch.from_numpy(u0s).to(dev), torch.from_numpy(a0s).to(dev)
    d_u = torch.empty((6, V.shape[0], 1), dtype=torch.float64, device=dev)
    alpha, cost, iters = np.empty_like(a0s), np.empty(6), np.empty(6, dtype=np.int64)
    sum_sq, n_test = np.empty(6), np.empty(6, dtype=np.int64)
    torch.cuda.synchronize(dev)
    status = raw_call(toy_problem, 6, bits, d_u0, d_a0, 1, PARTIAL, 10000, L.DMF_PTR_DEVICE, d_u, alpha, cost, iters, sum_sq, n_test)
    assert status == L.DMF_OK
    toy_problem.ctx.synchronize()
    assert same(want, (d_u.cpu().numpy(), alpha, cost, iters, sum_sq, n_test))
    assert np.array_equal(d_u0.cpu().numpy(), u0s) and np.array_equal(d_a0.cpu().numpy(), a0s)  # inputs are never written


# ---- 3. refusals -------------------------------------------------------------------------------------------------------

def test_a_mask_that_keeps_nothing_is_refused_before_any_solve_starts(toy_problem):
    from demethify_amd import _lib as L

    V, _, _, masks = data("toy 5+1")
    u0s, a0s = stacked(natural_runs("toy 5+1")[:3])
    m = masks[:3].copy()
    m[1] = False
    bits = np.packbits(m, axis=2, bitorder="little")
    outs = [np.full((3, V.shape[0], 1), -7.0), np.full(a0s.shape, -7.0), np.full(3, -7.0), np.full(3, -7, dtype=np.int64),
            np.full(3, -7.0), np.full(3, -7, dtype=np.int64)]
    status = raw_call(toy_problem, 3, bits, u0s, a0s, 1, PARTIAL, 10000, 0, *outs)
    assert status == L.DMF_ERR_BAD_ARG
    assert all(np.all(x == -7) for x in outs)  # the sentinel: no output was touched
    with pytest.raises(L.DemethifyHipError) as e:
        toy_problem.solve_many_masked(u0s, a0s, m, PARTIAL, 10000, T2, TOL)
    assert e.value.status == L.DMF_ERR_BAD_ARG
    # a null train_bits
    status = raw_call(toy_problem, 3, None, u0s, a0s, 1, PARTIAL, 10000, 0, *outs)
    assert status == L.DMF_ERR_BAD_ARG and all(np.all(x == -7) for x in outs)


def test_a_masked_problem_and_a_shape_outside_the_envelope_are_refused(toy_problem):
    from demethify_amd import _lib as L

    V, _, _, masks = data("toy 5+1")
    u0s, a0s = stacked(natural_runs("toy 5+1")[:2])
    with toy_problem.masked(masks[0]) as held:
        with pytest.raises(L.DemethifyHipError) as e:
            held.solve_many_masked(u0s, a0s, masks[:2], PARTIAL, 5, T2, 0.0)
    assert e.value.status == L.DMF_ERR_BAD_ARG
    with pytest.raises(L.DemethifyHipError) as e:
        toy_problem.solve_many_masked(np.full((1, V.shape[0], 5), 0.5), np.full((1, 10, V.shape[1]), 0.1), masks[:1], PARTIAL, 5, T2,
                                      0.0)
    assert e.value.status == L.DMF_ERR_UNSUPPORTED


# ---- 4. drivers (toy, uniform_, tol 1e-2, 20 inner steps) ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle_fold(n_u, mask_bytes, seed):
    """One fold of the toy on the oracle, remembered by its mask: upstream's reseeding makes most folds the same one."""
    V, D, Rt, _ = data("toy 5+1")
    return oracle_run(V, D, Rt, n_u, np.frombuffer(mask_bytes, dtype=bool).reshape(V.shape), seed, 10000, TOL)


def oracle_bicross_validation(V, n_u, D, n_folds, seed, Rt, fraction=0.3):
    """ic.py:58-89 restated on the oracle solver -> (total_press, u, alpha, winning fold, per-fold errors, margins)."""
    np.random.seed(seed)
    total, best, min_error, errors, margins = 0, (None, None, None), float("inf"), [], []
    for fold in range(n_folds):
        m = np.random.rand(*V.shape) < fraction
        if np.sum(~m) == 0 or np.sum(m) == 0:
            continue
        # the initialiser reseeds, as upstream's, and the next mask follows its draws: it runs for every fold, the solve
        # only for a mask not seen before
        osol.init_partial("uniform_", V * m, D * m, Rt, n_u, seed=seed)
        r = oracle_fold(n_u, m.tobytes(), seed)
        margins.append(stop_margin(r["cf_start"], r["trace"], TOL))
        error = r["sum_sq"] / np.sum(~m)
        errors.append(error)
        total += error
        if error < min_error:
            min_error, best = error, (r["u"], r["alpha"], fold)
    return total, best[0], best[1], best[2], errors, margins


@pytest.mark.parametrize("n_u", [1, 2])
def test_bicross_validation_batched_matches_the_restated_loop(ctx, n_u, monkeypatch):
    from demethify_amd import ic
    from demethify_amd.device import Problem

    V, D, Rt, _ = data("toy 5+1")
    want_total, want_u, want_alpha, winner, errors, margins = oracle_bicross_validation(V, n_u, D, 5, 1, Rt)
    print(f"n_u = {n_u}: oracle fold errors {[f'{e:.6f}' for e in errors]}, winner fold {winner}, margins {min(margins):.2e}")
    assert min(margins) >= MIN_MARGIN
    # upstream's reseeding initialiser makes every fold after the first draw the same mask: folds 1..4 are one solve, and the
    # first strict minimum is fold 1
    assert errors[1] == errors[2] == errors[3] == errors[4]
    if n_u == 1:
        assert [round(e, 6) for e in errors[:2]] == [0.009564, 0.008390] and winner == 1
    seen = []
    real = Problem.solve_many_masked

    def spy(self, *a, **k):
        out = real(self, *a, **k)
        seen.append(out)
        return out

    monkeypatch.setattr(Problem, "solve_many_masked", spy)
    total, u, alpha = ic.bicross_validation(V, n_u, D, 10000, T2, TOL, n_folds=5, seed=1, ref=Rt, init_option="uniform_",
                                            fraction=0.3, batched=True)
    assert len(seen) == 1 and len(seen[0][0]) == 5
    got_errors = seen[0][4] / seen[0][5]
    print(f"device fold errors {[f'{e:.6f}' for e in got_errors]}, total rel {abs(total - want_total) / want_total:.3e}")
    assert total == pytest.approx(want_total, rel=PARITY_RTOL)
    for b in (2, 3, 4):  # the four equal folds come out with equal bits
        assert same(each(seen[0], 1), each(seen[0], b))
    assert int(np.argmin(got_errors)) == winner  # (argmin: the first of equal minima, as the strict '<')
    assert np.array_equal(u, seen[0][0][winner]) and np.array_equal(alpha, seen[0][1][winner])
    assert np.abs(u - want_u).max() <= TIGHT and np.abs(alpha - want_alpha).max() <= TIGHT


def oracle_ccc_runs(V, D, Rt, n_u, seeds):
    return [odrv.run_one(V, D, Rt, n_u, "uniform_", s, 10000, T2, TOL, project=FAST)[2] for s in seeds]


def test_evaluate_best_ic_batched_ccc_scores_are_the_oracles(ctx, monkeypatch):
    from demethify_amd import ic
    from demethify_amd.device import Problem

    V, D, Rt, _ = data("toy 5+1")
    want = []
    for n_u in (1, 2, 3):
        runs = oracle_ccc_runs(V, D, Rt, n_u, [1 + r for r in range(4)])
        for a in runs:  # no dominant cell type is a near tie: the labels, and so the score, are exactly the oracle's
            top = np.sort(a, axis=0)
            assert (top[-1] - top[-2]).min() >= 1e-6
        want.append(-ic.compute_ccc(runs))
    calls = []
    real = Problem.solve_many
    monkeypatch.setattr(Problem, "solve_many", lambda self, *a, **k: calls.append(len(a[0])) or real(self, *a, **k))
    monkeypatch.setattr(ic, "Solver", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a per-solve Solver")))
    u, alpha, n_best, scores = ic.evaluate_best_ic(V, Rt, D, "uniform_", "CCC", 1, 10000, T2, TOL, n_restarts=4,
                                                   n_u_values=(1, 2, 3), batched=True)
    assert calls == [4, 4, 4]
    print(f"CCC scores {scores} oracle {want}")
    assert list(scores) == want
    assert n_best == (1, 2, 3)[int(np.argmin(want))] and u.shape == (V.shape[0], n_best)


def test_evaluate_best_ic_batched_bcv_goes_through_the_masked_batch(ctx, monkeypatch):
    from demethify_amd import ic
    from demethify_amd.device import Problem

    V, D, Rt, _ = data("toy 5+1")
    want = [oracle_bicross_validation(V, n_u, D, 4, 1, Rt) for n_u in (1, 2, 3)]
    assert min(min(w[5]) for w in want) >= MIN_MARGIN
    calls = []
    real = Problem.solve_many_masked
    monkeypatch.setattr(Problem, "solve_many_masked", lambda self, *a, **k: calls.append(len(a[0])) or real(self, *a, **k))
    monkeypatch.setattr(Problem, "masked", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a masked problem per fold")))
    u, alpha, n_best, scores = ic.evaluate_best_ic(V, Rt, D, "uniform_", "BCV", 1, 10000, T2, TOL, n_restarts=4,
                                                   n_u_values=(1, 2, 3), batched=True)
    assert calls == [4, 4, 4]
    print(f"BCV scores {scores} oracle {[w[0] for w in want]}")
    for got, w in zip(scores, want):
        assert got == pytest.approx(w[0], rel=PARITY_RTOL)
    best = int(np.argmin([w[0] for w in want]))
    assert n_best == (1, 2, 3)[best]
    assert np.abs(u - want[best][1]).max() <= TIGHT and np.abs(alpha - want[best][2]).max() <= TIGHT


def test_evaluate_best_ic_batched_aic_and_the_candidate_outside_the_envelope(ctx, monkeypatch, capsys):
    from demethify_amd import ic
    from demethify_amd.device import Problem

    V, D, Rt, _ = data("toy 5+1")
    values = (1, 2, 3, 4, 5)
    _, _, want_best, want = odrv.ic_sweep(V, Rt, D, "uniform_", "AIC", 1, 10000, T2, TOL, n_u_values=values, project=FAST)
    batch, solvers = [], []
    real_many, real_solver = Problem.solve_many, ic.Solver
    monkeypatch.setattr(Problem, "solve_many", lambda self, *a, **k: batch.append(a[0].shape) or real_many(self, *a, **k))

    def solver(problem, u0, a0, mode):
        solvers.append(np.asarray(u0).reshape(V.shape[0], -1).shape[1])
        return real_solver(problem, u0, a0, mode)

    monkeypatch.setattr(ic, "Solver", solver)
    u, alpha, n_best, scores = ic.evaluate_best_ic(V, Rt, D, "uniform_", "AIC", 1, 10000, T2, TOL, n_u_values=values, batched=True)
    print(f"AIC scores {scores} oracle {want}")
    assert sorted(s[2] for s in batch) == [1, 2, 3, 4] and all(s[0] == 1 for s in batch)  # batches of one
    assert solvers == [5]  # candidate 5 took the per-solve path
    assert "n_u = [5]" in capsys.readouterr().out
    for got, w in zip(scores, want):
        assert got == pytest.approx(w, rel=1e-9)
    assert n_best == want_best == values[int(np.argmin(want))]


def test_command_line_batched_bcv_reaches_the_masked_batch(tmp_path, monkeypatch):
    """DEMETHIFY_BATCH=1 --ic BCV 5 1 2 on the toy: the folds go through solve_many_masked and the proportions are those of
    the run without the variable, to 1e-8."""
    from demethify_amd import demethify, ic
    from demethify_amd.device import Problem

    V = data("toy 5+1")[0]
    if ic.SMALL_BATCH_IC_MAX_ELEMENTS < V.size:  # (the measured gate may sit below the toy)
        monkeypatch.setattr(ic, "SMALL_BATCH_IC_MAX_ELEMENTS", V.size)
    calls = []
    real = Problem.solve_many_masked
    monkeypatch.setattr(Problem, "solve_many_masked", lambda self, *a, **k: calls.append(len(a[0])) or real(self, *a, **k))
    samples = [str(UPSTREAM / "output_gen" / f"sample{i}.bed") for i in range(1, 11)]
    results = {}
    for name, value in (("plain", None), ("batched", "1")):
        if value is None:
            monkeypatch.delenv("DEMETHIFY_BATCH", raising=False)
        else:
            monkeypatch.setenv("DEMETHIFY_BATCH", value)
        out = tmp_path / name
        demethify.main(["--ref", str(UPSTREAM / "output_gen" / "ref_matrix.bed"), "--methfreq", *samples, "--bedmethyl",
                        "--noprint", "--ic", "BCV", "5", "1", "2", "--outdir", str(out)])  # (defaults: uniform_, 1e-2, 10000 x 20)
        results[name] = pd.read_csv(out / "celltypes_proportions.csv", index_col=0, float_precision="round_trip").values
        if value is None:
            assert calls == []
    assert calls == [5, 5]
    assert results["plain"].shape == results["batched"].shape
    assert np.abs(results["plain"] - results["batched"]).max() <= TIGHT
