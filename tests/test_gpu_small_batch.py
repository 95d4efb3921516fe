"""Many small solves in one launch (Problem.solve_many / dmf_solve_small, one workgroup per solve) against the numpy
oracle -- never against the per-solve device path.  Bars: those of tests/test_gpu_solver.py (u and alpha max-abs 1e-8,
cost relative 1e-9, stop iteration equal).  Every natural-stop case first shows on the oracle's own cost trace that no
stop test is decided by less than 1e-4 tol."""
import numpy as np
import pandas as pd
import pytest

from oracle import drivers as odrv
from oracle import solver as osol

from conftest import UPSTREAM, read_profile, read_props

pytestmark = pytest.mark.gpu

TIGHT = 1e-8
COST_RTOL = 1e-9
TOL, T2 = 1e-2, 20
MIN_MARGIN = 1e-4
FAST = osol.simplex_project_columns_fast


def stop_margin(cf_start, trace, tol):
    """min_j ||cf_j - cf_{j-1}| - tol| / tol over the oracle's stop tests."""
    cf = np.concatenate([[cf_start], trace])
    return float(np.min(np.abs(np.abs(np.diff(cf)) - tol)) / tol)


def oracle_partial(V, D, Rt, n_u, seed, n_iter1, n_iter2, tol, option="uniform_"):
    u0, R, a0 = osol.init_partial(option, V, D, Rt, n_u, seed=seed)
    trace = []
    cf_start = osol.weighted_cost(V, R, a0, D)
    u, alpha = osol.solve_partial(u0.copy(), R, a0.copy(), V, D, Rt, n_u, n_iter1, n_iter2, tol, project=FAST, trace=trace)
    return u0, a0, u, alpha, trace, cf_start


def oracle_unsupervised(V, D, n_u, seed, n_iter1, n_iter2, tol):
    u0, a0 = osol.init_unsupervised("uniform_", V, n_u, seed=seed)
    trace = []
    cf_start = osol.weighted_cost(V, u0, a0, D)
    u, alpha = osol.solve_unsupervised(V, n_u, D, "uniform_", n_iter1, n_iter2, tol, init=(u0.copy(), a0.copy()), project=FAST,
                                       trace=trace)
    return u0, a0, u, alpha, trace, cf_start


def hold(got, want_u, want_alpha, want_cost, want_iters):
    u, alpha, cost, iters = got
    print(f"max|u - oracle| = {np.abs(u - want_u).max():.3e}  max|alpha - oracle| = {np.abs(alpha - want_alpha).max():.3e}  "
          f"cost rel = {abs(cost - want_cost) / want_cost:.3e}  iterations {iters} / {want_iters}")
    assert iters == want_iters
    assert np.abs(u - want_u).max() <= TIGHT
    assert np.abs(alpha - want_alpha).max() <= TIGHT
    assert cost == pytest.approx(want_cost, rel=COST_RTOL)


def each(out, b):
    return out[0][b], out[1][b], float(out[2][b]), int(out[3][b])


@pytest.fixture(scope="module")
def toy_problem(ctx, toy):
    from demethify_amd.device import Problem

    V, D, ref, _ = toy
    with Problem(ctx, V, D, ref) as p:
        yield p


@pytest.fixture(scope="module")
def toy_restarts(toy):
    """The oracle's 16 partial-reference restarts of the toy (seeds 1..16), each with its stop margin."""
    V, D, ref, _ = toy
    runs = [oracle_partial(V, D, ref, 1, seed, 10000, T2, TOL) for seed in range(1, 17)]
    for r in runs:
        for a in r[:4]:
            a.setflags(write=False)
    return runs


@pytest.fixture(scope="module")
def toy_replicates(toy):
    """oracle.drivers.bootstrap_replicates on the toy, 24 replicates from seed 1, with every replicate's cost trace (its
    solver is asked for the trace and given the vectorised projection: the same arithmetic per column)."""
    V, D, ref, _ = toy
    traces, starts = [], []
    plain = osol.solve_partial

    def traced(u, R, alpha, Vb, Db, Rb, n_u, n_iter1, n_iter2, tol):
        starts.append(osol.weighted_cost(Vb, R, alpha, Db))
        traces.append([])
        return plain(u, R, alpha, Vb, Db, Rb, n_u, n_iter1, n_iter2, tol, project=FAST, trace=traces[-1])

    osol.solve_partial = traced
    try:
        us, alphas = odrv.bootstrap_replicates(24, 1, V, D, ref, "uniform_", 10000, T2, TOL, 1)
    finally:
        osol.solve_partial = plain
    us.setflags(write=False)
    alphas.setflags(write=False)
    return us, alphas, traces, starts


# ---- 1. toy restarts ---------------------------------------------------------------------------------------------------

def test_toy_partial_restarts_in_one_call(toy, toy_problem, toy_restarts):
    from demethify_amd import _lib as L

    for seed, r in enumerate(toy_restarts, 1):
        margin = stop_margin(r[5], r[4], TOL)
        print(f"seed {seed}: oracle stops after {len(r[4])}, margin {margin:.2e}")
        assert margin >= MIN_MARGIN
    out = toy_problem.solve_many(np.stack([r[0] for r in toy_restarts]), np.stack([r[1] for r in toy_restarts]),
                                 L.DMF_MODE_PARTIAL, 10000, T2, TOL)
    for b, r in enumerate(toy_restarts):
        hold(each(out, b), r[2], r[3], r[4][-1], len(r[4]))
    assert int(out[3][0]) == 54
    assert np.abs(out[1][0] - read_props("output_partial_ref")).max() <= TIGHT
    assert np.abs(out[0][0] - read_profile("output_partial_ref")).max() <= TIGHT


def test_toy_unsupervised_restarts_in_one_call(ctx, toy):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem

    V, D, _, _ = toy
    runs = [oracle_unsupervised(V, D, 4, seed, 10000, T2, TOL) for seed in range(1, 5)]
    for seed, r in enumerate(runs, 1):
        margin = stop_margin(r[5], r[4], TOL)
        print(f"seed {seed}: oracle stops after {len(r[4])}, margin {margin:.2e}")
        assert margin >= MIN_MARGIN
    with Problem(ctx, V, D, None) as p:
        out = p.solve_many(np.stack([r[0] for r in runs]), np.stack([r[1] for r in runs]), L.DMF_MODE_UNSUPERVISED, 10000, T2, TOL)
    for b, r in enumerate(runs):
        hold(each(out, b), r[2], r[3], r[4][-1], len(r[4]))
    assert np.abs(out[1][0] - read_props("unsupervised")).max() <= TIGHT


# ---- 2. toy bootstrap --------------------------------------------------------------------------------------------------

def test_toy_bootstrap_replicates_through_idx(toy, toy_problem, toy_replicates):
    from demethify_amd import _lib as L

    V, D, ref, _ = toy
    us, alphas, traces, starts = toy_replicates
    B = 16
    seeds = osol.bootstrap_seeds(1, B)
    idx = np.stack([osol.bootstrap_indices(s, V.shape[0]) for s in seeds])
    inits = [osol.init_partial("uniform_", V[:1].repeat(V.shape[0], 0), D, ref, 1, seed=s) for s in seeds]
    for b in range(B):
        margin = stop_margin(starts[b], traces[b], TOL)
        print(f"replicate {b}: oracle stops after {len(traces[b])}, margin {margin:.2e}")
        assert margin >= MIN_MARGIN
    out = toy_problem.solve_many(np.stack([i[0] for i in inits]), np.stack([i[2] for i in inits]), L.DMF_MODE_PARTIAL,
                                 10000, T2, TOL, idx=idx)
    for b in range(B):
        hold(each(out, b), us[b], alphas[b], traces[b][-1], len(traces[b]))


# ---- 3. edge shapes ----------------------------------------------------------------------------------------------------

EDGES = [  # (N, S, n_c, n_u, n_iter1)
    (64, 1, 1, 1, 5), (257, 3, 2, 1, 5), (65, 64, 0, 4, 3), (777, 33, 0, 3, 3), (2049, 17, 15, 1, 3), (1000, 64, 12, 4, 2),
]


def edge_case(ctx, N, S, n_c, n_u, n_iter1, n_iter2, tol, seeds=(1, 2, 3)):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem

    V, D, Rt = osol.synthetic_problem(N, S, n_c, n_u, seed=11, depth=30)
    if n_c:
        runs = [oracle_partial(V, D, Rt, n_u, seed, n_iter1, n_iter2, tol) for seed in seeds]
        mode = L.DMF_MODE_PARTIAL
    else:
        runs = [oracle_unsupervised(V, D, n_u, seed, n_iter1, n_iter2, tol) for seed in seeds]
        mode = L.DMF_MODE_UNSUPERVISED
    with Problem(ctx, V, D, Rt if n_c else None) as p:
        out = p.solve_many(np.stack([r[0] for r in runs]), np.stack([r[1] for r in runs]), mode, n_iter1, n_iter2, tol)
    for b, r in enumerate(runs):
        hold(each(out, b), r[2], r[3], r[4][-1], len(r[4]))
    return runs


@pytest.mark.parametrize("N,S,n_c,n_u,n_iter1", EDGES)
def test_edge_shapes_fixed_iterations(ctx, N, S, n_c, n_u, n_iter1):
    """tol = 0 never satisfies the stop test: exactly n_iter1 outer iterations on both sides."""
    runs = edge_case(ctx, N, S, n_c, n_u, n_iter1, T2, 0.0)
    assert all(len(r[4]) == n_iter1 for r in runs)


@pytest.mark.parametrize("n_iter2", [1, 50])
def test_edge_inner_iteration_counts(ctx, n_iter2):
    edge_case(ctx, 257, 3, 2, 1, 4, n_iter2, 0.0)


def test_iteration_cap_hits_before_the_tolerance(ctx):
    runs = edge_case(ctx, 777, 33, 0, 3, 5, T2, TOL)
    for r in runs:  # the cap decides, not a near tie: no stop test of these five iterations comes close to tol
        assert len(r[4]) == 5 and stop_margin(r[5], r[4], TOL) >= MIN_MARGIN
        assert np.all(np.abs(np.diff(np.concatenate([[r[5]], r[4]]))) > TOL)


# ---- 4. independence ---------------------------------------------------------------------------------------------------

def test_a_solve_does_not_depend_on_its_slot_or_its_neighbours(toy, toy_problem, toy_restarts):
    """The same solve alone and in slots 0, 7 and 1099 of B = 1100 (more workgroups than are resident at once), the other
    slots holding other solves: bit-identical."""
    from demethify_amd import _lib as L

    u0, a0 = toy_restarts[0][0], toy_restarts[0][1]
    alone = toy_problem.solve_many(u0[None], a0[None], L.DMF_MODE_PARTIAL, 10000, T2, TOL)
    B = 1100
    u0s = np.stack([toy_restarts[b % 15 + 1][0] for b in range(B)])
    a0s = np.stack([toy_restarts[b % 15 + 1][1] for b in range(B)])
    for slot in (0, 7, 1099):
        u0s[slot], a0s[slot] = u0, a0
    many = toy_problem.solve_many(u0s, a0s, L.DMF_MODE_PARTIAL, 10000, T2, TOL)
    for slot in (0, 7, 1099):
        for x, y in zip(each(alone, 0), each(many, slot)):
            assert np.array_equal(x, y)
    assert int(many[3][1]) == len(toy_restarts[2][4])  # (slot 1 is seed 3's solve, stopping where the oracle's does)


def test_identity_index_equals_no_index(toy, toy_problem, toy_restarts):
    from demethify_amd import _lib as L

    V = toy[0]
    u0s = np.stack([r[0] for r in toy_restarts[:3]])
    a0s = np.stack([r[1] for r in toy_restarts[:3]])
    plain = toy_problem.solve_many(u0s, a0s, L.DMF_MODE_PARTIAL, 10000, T2, TOL)
    through = toy_problem.solve_many(u0s, a0s, L.DMF_MODE_PARTIAL, 10000, T2, TOL, idx=np.tile(np.arange(V.shape[0]), (3, 1)))
    for x, y in zip(plain, through):
        assert np.array_equal(x, y)


def test_results_do_not_depend_on_iterations_per_launch(toy_problem, toy_restarts):
    from demethify_amd import _lib as L

    u0s = np.stack([r[0] for r in toy_restarts[:4]])
    a0s = np.stack([r[1] for r in toy_restarts[:4]])
    want = toy_problem.solve_many(u0s, a0s, L.DMF_MODE_PARTIAL, 10000, T2, TOL)
    assert [int(i) for i in want[3]] == [len(r[4]) for r in toy_restarts[:4]]
    for per_launch in (1, 7):
        got = toy_problem.solve_many(u0s, a0s, L.DMF_MODE_PARTIAL, 10000, T2, TOL, iters_per_launch=per_launch)
        for x, y in zip(want, got):
            assert np.array_equal(x, y)


# ---- 5. refusals and non-mutation --------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,S,n_c,n_u", [(100, 65, 2, 1), (100, 8, 13, 4), (100, 8, 0, 5), (16385, 64, 0, 1)])
def test_shapes_outside_the_envelope_are_unsupported(ctx, N, S, n_c, n_u):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, small_solve_supported

    assert N * S == (1 << 20) + 64 or N == 100
    assert not small_solve_supported(N, S, n_c, n_u, L.DMF_MODE_PARTIAL)
    V = np.full((N, S), 0.5)
    D = np.full((N, S), 3, dtype=np.int64)
    Rt = np.full((N, n_c), 0.5) if n_c else None
    with Problem(ctx, V, D, Rt) as p:
        with pytest.raises(L.DemethifyHipError) as e:
            p.solve_many(np.full((1, N, n_u), 0.5), np.full((1, n_c + n_u, S), 1.0 / (n_c + n_u)), L.DMF_MODE_PARTIAL, 2, 2, 0.0)
    assert e.value.status == L.DMF_ERR_UNSUPPORTED


def test_bad_arguments_and_untouched_inputs(toy, toy_problem, toy_restarts):
    from demethify_amd import _lib as L

    V, D, ref, _ = toy
    N = V.shape[0]
    u0s = np.stack([r[0] for r in toy_restarts[:2]])
    a0s = np.stack([r[1] for r in toy_restarts[:2]])
    idx = np.tile(np.arange(N), (2, 1))
    idx[1, N - 1] = N  # one past the last row, in the second solve
    keep = [x.copy() for x in (u0s, a0s, idx)]
    with pytest.raises(L.DemethifyHipError) as e:
        toy_problem.solve_many(u0s, a0s, L.DMF_MODE_PARTIAL, 5, T2, 0.0, idx=idx)
    assert e.value.status == L.DMF_ERR_BAD_ARG
    with pytest.raises(L.DemethifyHipError) as e:
        toy_problem.solve_many(u0s[:0], a0s[:0], L.DMF_MODE_PARTIAL, 5, T2, 0.0)
    assert e.value.status == L.DMF_ERR_BAD_ARG
    mask = np.ones(V.shape, dtype=bool)
    mask[::7, 3] = False
    with toy_problem.masked(mask) as held:
        with pytest.raises(L.DemethifyHipError) as e:
            held.solve_many(u0s, a0s, L.DMF_MODE_PARTIAL, 5, T2, 0.0)
    assert e.value.status == L.DMF_ERR_BAD_ARG
    idx[1, N - 1] = 0
    keep[2] = idx.copy()
    before = {name: toy_problem.copy_out(name) for name in ("V", "D", "Rt")}
    toy_problem.solve_many(u0s, a0s, L.DMF_MODE_PARTIAL, 5, T2, 0.0, idx=idx)
    for got, want in zip((u0s, a0s, idx), keep):
        assert np.array_equal(got, want)
    for name, want in before.items():
        assert np.array_equal(toy_problem.copy_out(name), want)


# ---- 6. drivers --------------------------------------------------------------------------------------------------------

def test_bt_ci_batched_matches_the_oracle_bounds(tmp_path, toy, toy_replicates, monkeypatch):
    from demethify_amd import bootstrap
    from demethify_amd.device import Problem

    V, D, ref, header = toy
    us, alphas, traces, starts = toy_replicates
    for b in range(24):
        assert stop_margin(starts[b], traces[b], TOL) >= MIN_MARGIN
    calls = []
    real = Problem.solve_many
    monkeypatch.setattr(Problem, "solve_many", lambda self, *a, **k: calls.append(len(a[0])) or real(self, *a, **k))
    samples = [f"s{k}" for k in range(V.shape[1])]
    props, (lower_u, upper_u) = bootstrap.bt_ci(95, 24, 1, V, D, ref, "uniform_", 10000, T2, TOL, header, str(tmp_path), samples,
                                                None, 1, materialize=False, batched=True)
    assert calls == [24]
    lo_a, hi_a = odrv.percentile_bounds(alphas, 95)
    lo_u, hi_u = odrv.percentile_bounds(us, 95)
    got = np.array([[cell for cell in props[col]] for col in props.columns])  # (S, K, 2)
    assert np.abs(got[:, :, 0].T - lo_a).max() <= TIGHT and np.abs(got[:, :, 1].T - hi_a).max() <= TIGHT
    assert np.abs(lower_u - lo_u).max() <= TIGHT and np.abs(upper_u - hi_u).max() <= TIGHT
    assert (tmp_path / "confidence_interval_celltypes_proportions.csv").exists()
    assert (tmp_path / "confidence_interval_methylation_estimate.csv").exists()


def test_command_line_batched_restarts_pick_the_oracle_winner(tmp_path, toy, toy_restarts, monkeypatch):
    """DEMETHIFY_BATCH=1 --restart 8 on the toy (below the size gate: the restarts do go through solve_many): the winner
    is oracle.drivers.restart_pick's for seeds 1..8, its proportions within 1e-8."""
    from demethify_amd import bootstrap, demethify
    from demethify_amd.device import Problem

    V, D, ref, _ = toy
    for r in toy_restarts[:8]:
        assert stop_margin(r[5], r[4], TOL) >= MIN_MARGIN
    plain = osol.solve_partial
    osol.solve_partial = lambda *a, **k: plain(*a, **{**k, "project": FAST})
    try:
        want_u, want_alpha, want_k, costs = odrv.restart_pick(V, D, ref, 1, "uniform_", list(range(1, 9)), 10000, T2, TOL)
    finally:
        osol.solve_partial = plain
    ordered = np.sort(costs)
    assert (ordered[1] - ordered[0]) / ordered[0] > 1e-6  # the pick is not a near tie
    calls = []
    real = Problem.solve_many
    monkeypatch.setattr(Problem, "solve_many", lambda self, *a, **k: calls.append(len(a[0])) or real(self, *a, **k))
    assert V.size <= bootstrap.SMALL_BATCH_MAX_ELEMENTS
    monkeypatch.setenv("DEMETHIFY_BATCH", "1")
    out = tmp_path / "out"
    samples = [str(UPSTREAM / "output_gen" / f"sample{i}.bed") for i in range(1, 11)]
    demethify.main(["--ref", str(UPSTREAM / "output_gen" / "ref_matrix.bed"), "--methfreq", *samples, "--bedmethyl", "--noprint",
                    "--nbunknown", "1", "--restart", "8", "--outdir", str(out)])
    assert calls == [8]
    got_alpha = pd.read_csv(out / "celltypes_proportions.csv", index_col=0, float_precision="round_trip").values
    got_u = pd.read_csv(out / "methylation_profile_estimate.csv", float_precision="round_trip").values
    assert np.abs(got_alpha - want_alpha).max() <= TIGHT and np.abs(got_u - want_u).max() <= TIGHT
    others = [r[3] for k, r in enumerate(toy_restarts[:8]) if k != want_k]
    assert min(np.abs(got_alpha - o).max() for o in others) > 1e-6  # (no other restart's proportions would pass)
