"""The mid-size batch (Problem.solve_many_mid / dmf_solve_mid, several workgroups per solve, three launches per outer
iteration) against the numpy oracle -- never against another device path.  Bars: those of tests/test_gpu_small_batch.py
(u and alpha max-abs 1e-8, cost relative 1e-9, stop iteration equal).  Every natural-stop case first shows on the oracle's
own cost trace that no stop test is decided by less than 1e-4 tol."""
import re

import numpy as np
import pandas as pd
import pytest

from oracle import drivers as odrv
from oracle import solver as osol

from conftest import read_profile, read_props
from test_gpu_small_batch import (MIN_MARGIN, T2, TIGHT, TOL, each, hold, oracle_partial, oracle_unsupervised, stop_margin,
                                  toy_problem, toy_replicates, toy_restarts)  # noqa: F401  (the last three are fixtures)

pytestmark = pytest.mark.gpu


def show_margins(runs):
    for seed, r in enumerate(runs, 1):
        margin = stop_margin(r[5], r[4], TOL)
        print(f"seed {seed}: oracle stops after {len(r[4])}, margin {margin:.2e}")
        assert margin >= MIN_MARGIN


def stacks(runs):
    return np.stack([r[0] for r in runs]), np.stack([r[1] for r in runs])


@pytest.fixture(scope="module")
def mid_1000(ctx):
    """synthetic_problem(1000, 16, 6, 2, seed=3) resident, with the oracle's solves from seeds 1..4."""
    from demethify_amd.device import Problem

    V, D, Rt = osol.synthetic_problem(1000, 16, 6, 2, seed=3)
    runs = [oracle_partial(V, D, Rt, 2, seed, 10000, T2, TOL) for seed in range(1, 5)]
    for r in runs:
        for a in r[:4]:
            a.setflags(write=False)
    with Problem(ctx, V, D, Rt) as p:
        yield p, runs


# ---- 1, 2. toy restarts, W = 2 with a ragged slab of 94 rows -----------------------------------------------------------

def test_toy_partial_restarts_in_one_call(toy_problem, toy_restarts):
    from demethify_amd import _lib as L
    from demethify_amd.device import mid_solve_plan

    show_margins(toy_restarts)
    assert mid_solve_plan(350, 10, 256)[:2] == (256, 2)
    out = toy_problem.solve_many_mid(*stacks(toy_restarts), L.DMF_MODE_PARTIAL, 10000, T2, TOL, rows_per_workgroup=256)
    for b, r in enumerate(toy_restarts):
        hold(each(out, b), r[2], r[3], r[4][-1], len(r[4]))
    assert len(set(int(i) for i in out[3])) > 4  # (finished solves sit beside running ones)
    assert int(out[3][0]) == 54
    assert np.abs(out[1][0] - read_props("output_partial_ref")).max() <= TIGHT
    assert np.abs(out[0][0] - read_profile("output_partial_ref")).max() <= TIGHT


def test_toy_unsupervised_restarts_in_one_call(ctx, toy):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem

    V, D, _, _ = toy
    runs = [oracle_unsupervised(V, D, 4, seed, 10000, T2, TOL) for seed in range(1, 5)]
    show_margins(runs)
    with Problem(ctx, V, D, None) as p:
        out = p.solve_many_mid(*stacks(runs), L.DMF_MODE_UNSUPERVISED, 10000, T2, TOL, rows_per_workgroup=256)
    for b, r in enumerate(runs):
        hold(each(out, b), r[2], r[3], r[4][-1], len(r[4]))
    assert np.abs(out[1][0] - read_props("unsupervised")).max() <= TIGHT


# ---- 3. toy bootstrap through idx --------------------------------------------------------------------------------------

def test_toy_bootstrap_replicates_through_idx(toy, toy_problem, toy_replicates):
    from demethify_amd import _lib as L

    V, D, ref, _ = toy
    us, alphas, traces, starts = toy_replicates
    B = 24
    seeds = osol.bootstrap_seeds(1, B)
    idx = np.stack([osol.bootstrap_indices(s, V.shape[0]) for s in seeds])
    inits = [osol.init_partial("uniform_", V[:1].repeat(V.shape[0], 0), D, ref, 1, seed=s) for s in seeds]
    for b in range(B):
        margin = stop_margin(starts[b], traces[b], TOL)
        print(f"replicate {b}: oracle stops after {len(traces[b])}, margin {margin:.2e}")
        assert margin >= MIN_MARGIN
    out = toy_problem.solve_many_mid(np.stack([i[0] for i in inits]), np.stack([i[2] for i in inits]), L.DMF_MODE_PARTIAL,
                                     10000, T2, TOL, idx=idx, rows_per_workgroup=256)
    for b in range(B):
        hold(each(out, b), us[b], alphas[b], traces[b][-1], len(traces[b]))


# ---- 4, 5, 6. synthetic problems with several slabs --------------------------------------------------------------------

def test_700_by_7_with_three_slabs(ctx):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, mid_solve_plan

    assert mid_solve_plan(700, 7, 256)[:2] == (256, 3) and 700 - 2 * 256 == 188
    V, D, Rt = osol.synthetic_problem(700, 7, 3, 2, seed=3)
    runs = [oracle_partial(V, D, Rt, 2, seed, 10000, T2, TOL) for seed in range(1, 5)]
    show_margins(runs)
    with Problem(ctx, V, D, Rt) as p:
        out = p.solve_many_mid(*stacks(runs), L.DMF_MODE_PARTIAL, 10000, T2, TOL, rows_per_workgroup=256)
    for b, r in enumerate(runs):
        hold(each(out, b), r[2], r[3], r[4][-1], len(r[4]))


@pytest.mark.parametrize("rows", [256, 512])
def test_1000_by_16_at_two_slab_sizes(mid_1000, rows):
    from demethify_amd import _lib as L

    p, runs = mid_1000
    show_margins(runs)
    out = p.solve_many_mid(*stacks(runs), L.DMF_MODE_PARTIAL, 10000, T2, TOL, rows_per_workgroup=rows)
    for b, r in enumerate(runs):
        hold(each(out, b), r[2], r[3], r[4][-1], len(r[4]))


def test_900_by_9_unsupervised(ctx):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, mid_solve_plan

    assert mid_solve_plan(900, 9)[:2] == (256, 4)
    V, D, _ = osol.synthetic_problem(900, 9, 0, 3, seed=3)
    runs = [oracle_unsupervised(V, D, 3, seed, 10000, T2, TOL) for seed in range(1, 5)]
    show_margins(runs)
    with Problem(ctx, V, D, None) as p:
        out = p.solve_many_mid(*stacks(runs), L.DMF_MODE_UNSUPERVISED, 10000, T2, TOL)
    for b, r in enumerate(runs):
        hold(each(out, b), r[2], r[3], r[4][-1], len(r[4]))


# ---- 7. fixed work -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,S,n_c,n_u,rows,B", [(600, 64, 12, 4, 256, 2), (10000, 64, 12, 4, 0, 4), (513, 1, 2, 1, 0, 3)])
def test_fixed_work_three_iterations(ctx, N, S, n_c, n_u, rows, B):
    """tol = 0 never satisfies the stop test: exactly 3 outer iterations on both sides.  600 x 64 with 12 + 4 types is the
    LDS-largest instance of the alpha launch, 10 000 x 64 runs the default plan (40 slabs), S = 1 puts 256 row slices on one
    sample."""
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem

    V, D, Rt = osol.synthetic_problem(N, S, n_c, n_u, seed=3)
    runs = [oracle_partial(V, D, Rt, n_u, seed, 3, T2, 0.0) for seed in range(1, B + 1)]
    assert all(len(r[4]) == 3 for r in runs)
    with Problem(ctx, V, D, Rt) as p:
        out = p.solve_many_mid(*stacks(runs), L.DMF_MODE_PARTIAL, 3, T2, 0.0, rows_per_workgroup=rows)
    for b, r in enumerate(runs):
        hold(each(out, b), r[2], r[3], r[4][-1], 3)


# ---- 8. bit for bit ----------------------------------------------------------------------------------------------------

def test_a_solve_does_not_depend_on_its_slot_or_its_neighbours(toy_problem, toy_restarts):
    """The same solve alone and in slots 0, 7 and 39 of B = 40, the other slots holding other solves: bit-identical."""
    from demethify_amd import _lib as L

    u0, a0 = toy_restarts[0][0], toy_restarts[0][1]
    alone = toy_problem.solve_many_mid(u0[None], a0[None], L.DMF_MODE_PARTIAL, 10000, T2, TOL, rows_per_workgroup=256)
    assert int(alone[3][0]) == len(toy_restarts[0][4])
    B = 40
    u0s = np.stack([toy_restarts[b % 15 + 1][0] for b in range(B)])
    a0s = np.stack([toy_restarts[b % 15 + 1][1] for b in range(B)])
    for slot in (0, 7, 39):
        u0s[slot], a0s[slot] = u0, a0
    many = toy_problem.solve_many_mid(u0s, a0s, L.DMF_MODE_PARTIAL, 10000, T2, TOL, rows_per_workgroup=256)
    for slot in (0, 7, 39):
        for x, y in zip(each(alone, 0), each(many, slot)):
            assert np.array_equal(x, y)
    assert int(many[3][1]) == len(toy_restarts[2][4])  # (slot 1 is seed 3's solve, stopping where the oracle's does)


def test_results_do_not_depend_on_check_every_or_on_the_call(toy, toy_problem, toy_restarts):
    from demethify_amd import _lib as L

    u0s, a0s = stacks(toy_restarts[:4])
    want = toy_problem.solve_many_mid(u0s, a0s, L.DMF_MODE_PARTIAL, 10000, T2, TOL, rows_per_workgroup=256)
    assert [int(i) for i in want[3]] == [len(r[4]) for r in toy_restarts[:4]]
    again = toy_problem.solve_many_mid(u0s, a0s, L.DMF_MODE_PARTIAL, 10000, T2, TOL, rows_per_workgroup=256)
    through = toy_problem.solve_many_mid(u0s, a0s, L.DMF_MODE_PARTIAL, 10000, T2, TOL, rows_per_workgroup=256,
                                         idx=np.tile(np.arange(toy[0].shape[0]), (4, 1)))
    others = [again, through]
    for every in (1, 7):
        others.append(toy_problem.solve_many_mid(u0s, a0s, L.DMF_MODE_PARTIAL, 10000, T2, TOL, rows_per_workgroup=256,
                                                 check_every=every))
    for got in others:
        for x, y in zip(want, got):
            assert np.array_equal(x, y)


# ---- 9. one slab -------------------------------------------------------------------------------------------------------

def test_one_workgroup_per_solve(toy_problem, toy_restarts, mid_1000):
    from demethify_amd import _lib as L
    from demethify_amd.device import mid_solve_plan

    assert mid_solve_plan(350, 10, 512)[1] == 1 and mid_solve_plan(1000, 16, 1024)[1] == 1
    out = toy_problem.solve_many_mid(*stacks(toy_restarts[:4]), L.DMF_MODE_PARTIAL, 10000, T2, TOL, rows_per_workgroup=512)
    for b, r in enumerate(toy_restarts[:4]):
        hold(each(out, b), r[2], r[3], r[4][-1], len(r[4]))
    p, runs = mid_1000
    out = p.solve_many_mid(*stacks(runs[:2]), L.DMF_MODE_PARTIAL, 10000, T2, TOL, rows_per_workgroup=1024)
    for b, r in enumerate(runs[:2]):
        hold(each(out, b), r[2], r[3], r[4][-1], len(r[4]))


# ---- 10. refusals before any solve -------------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable(ctx, toy, toy_problem, toy_restarts):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, mid_solve_supported

    V, D, ref, _ = toy
    N = V.shape[0]
    u0s, a0s = stacks(toy_restarts[:2])
    want = [len(r[4]) for r in toy_restarts[:2]]

    def good_call():
        out = toy_problem.solve_many_mid(u0s, a0s, L.DMF_MODE_PARTIAL, 10000, T2, TOL, rows_per_workgroup=256)
        assert [int(i) for i in out[3]] == want
        hold(each(out, 1), toy_restarts[1][2], toy_restarts[1][3], toy_restarts[1][4][-1], want[1])

    # a shape outside the envelope
    assert not mid_solve_supported(100, 65, 2, 1, L.DMF_MODE_PARTIAL)
    with Problem(ctx, np.full((100, 65), 0.5), np.full((100, 65), 3, dtype=np.int64), np.full((100, 2), 0.5)) as wide:
        with pytest.raises(L.DemethifyHipError) as e:
            wide.solve_many_mid(np.full((1, 100, 1), 0.5), np.full((1, 3, 65), 1.0 / 3), L.DMF_MODE_PARTIAL, 2, 2, 0.0)
    assert e.value.status == L.DMF_ERR_UNSUPPORTED
    with pytest.raises(L.DemethifyHipError) as e:  # five unknown types on the toy
        toy_problem.solve_many_mid(np.full((1, N, 5), 0.5), np.full((1, 10, 10), 0.1), L.DMF_MODE_PARTIAL, 2, 2, 0.0)
    assert e.value.status == L.DMF_ERR_UNSUPPORTED
    good_call()

    # a masked problem
    mask = np.ones(V.shape, dtype=bool)
    mask[::7, 3] = False
    with toy_problem.masked(mask) as held:
        with pytest.raises(L.DemethifyHipError) as e:
            held.solve_many_mid(u0s, a0s, L.DMF_MODE_PARTIAL, 5, T2, 0.0)
    assert e.value.status == L.DMF_ERR_BAD_ARG
    good_call()

    # an index equal to N, in the second solve; the inputs stay what they were
    idx = np.tile(np.arange(N), (2, 1))
    idx[1, N - 1] = N
    keep = [x.copy() for x in (u0s, a0s, idx)]
    with pytest.raises(L.DemethifyHipError) as e:
        toy_problem.solve_many_mid(u0s, a0s, L.DMF_MODE_PARTIAL, 5, T2, 0.0, idx=idx)
    assert e.value.status == L.DMF_ERR_BAD_ARG
    for got, kept in zip((u0s, a0s, idx), keep):
        assert np.array_equal(got, kept)
    good_call()

    # a slab size the plan refuses
    with pytest.raises(L.DemethifyHipError) as e:
        toy_problem.solve_many_mid(u0s, a0s, L.DMF_MODE_PARTIAL, 5, T2, 0.0, rows_per_workgroup=100)
    assert e.value.status == L.DMF_ERR_BAD_ARG
    good_call()


# ---- 11. the bootstrap driver ------------------------------------------------------------------------------------------

def read_interval_csv(path, **kw):
    """A CSV of "(lo, hi)" cells -> (lower, upper) arrays."""
    table = pd.read_csv(path, **kw)
    number = r"(?:np\.float64\()?([-+0-9.e]+|nan)\)?"
    cells = [[re.fullmatch(rf"\({number}, {number}\)", cell).groups() for cell in table[col]] for col in table.columns]
    both = np.array(cells, dtype=np.float64)  # (columns, rows, 2)
    return both[:, :, 0].T, both[:, :, 1].T


def test_bt_ci_through_the_mid_batch_matches_the_oracle_bounds(tmp_path, toy, toy_replicates, monkeypatch):
    from demethify_amd import bootstrap
    from demethify_amd.device import Problem

    V, D, ref, header = toy
    us, alphas, traces, starts = toy_replicates
    for b in range(24):
        assert stop_margin(starts[b], traces[b], TOL) >= MIN_MARGIN
    calls = []
    real = Problem.solve_many_mid
    monkeypatch.setattr(Problem, "solve_many_mid", lambda self, *a, **k: calls.append(len(a[0])) or real(self, *a, **k))
    monkeypatch.setattr(Problem, "solve_many", lambda *a, **k: calls.append("solve_many"))
    samples = [f"s{k}" for k in range(V.shape[1])]
    props, (lower_u, upper_u) = bootstrap.bt_ci(95, 24, 1, V, D, ref, "uniform_", 10000, T2, TOL, header, str(tmp_path), samples,
                                                None, 1, materialize=False, batched=True, batch_kernel="mid")
    assert calls == [24]
    lo_a, hi_a = odrv.percentile_bounds(alphas, 95)
    lo_u, hi_u = odrv.percentile_bounds(us, 95)
    got = np.array([[cell for cell in props[col]] for col in props.columns])  # (S, K, 2)
    assert np.abs(got[:, :, 0].T - lo_a).max() <= TIGHT and np.abs(got[:, :, 1].T - hi_a).max() <= TIGHT
    assert np.abs(lower_u - lo_u).max() <= TIGHT and np.abs(upper_u - hi_u).max() <= TIGHT
    # ... and the two files hold the same numbers
    file_lo, file_hi = read_interval_csv(tmp_path / "confidence_interval_celltypes_proportions.csv", index_col=0)
    assert np.abs(file_lo - lo_a).max() <= TIGHT and np.abs(file_hi - hi_a).max() <= TIGHT
    file_lo, file_hi = read_interval_csv(tmp_path / "confidence_interval_methylation_estimate.csv")
    assert np.abs(file_lo - lo_u).max() <= TIGHT and np.abs(file_hi - hi_u).max() <= TIGHT
