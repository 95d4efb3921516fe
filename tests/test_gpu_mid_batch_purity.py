"""Purity-constrained solves in the mid-size batch (Problem.solve_many_mid(purity=...) / dmf_solve_mid_purity: k_mid_rows,
k_mid_alpha_fw, k_mid_cost per outer iteration) against oracle/solver.py::solve_partial_purity -- never against another
device path.  Bars: u and alpha max-abs 1e-8, cost relative 1e-9, stop iteration equal, block masses to 1e-12.  The cases
and their cached oracle runs are those of tests/small_batch_purity_cases.py; each test asserts the preconditions of its
cases (stop margin, argmin gap) on the oracle's trajectory before it asks the device."""
import numpy as np
import pandas as pd
import pytest

import small_batch_purity_cases as cases
from conftest import UPSTREAM, read_profile, read_props
from oracle import drivers as odrv
from small_batch_purity_cases import COST_RTOL, P, TIGHT, TOL

pytestmark = pytest.mark.gpu

MASS_TOL = 1e-12
ROWS = 256  # rows per slab of the toy and edge cases: the toy's 350 rows are two slabs, the second of 94 rows


def hold(got, run, n_c, purity):
    """One solve against its oracle run at the bars, and the block masses of its alpha."""
    u, alpha, cost, iters = got
    want_cost = run.trace[-1]
    print(f"max|u - oracle| = {np.abs(u - run.u).max():.3e}  max|alpha - oracle| = {np.abs(alpha - run.alpha).max():.3e}  "
          f"cost rel = {abs(cost - want_cost) / want_cost:.3e}  iterations {iters} / {len(run.trace)}")
    assert iters == len(run.trace)
    assert np.abs(u - run.u).max() <= TIGHT
    assert np.abs(alpha - run.alpha).max() <= TIGHT
    assert cost == pytest.approx(want_cost, rel=COST_RTOL)
    # every column's known rows carry purity[s], its unknown rows 1 - purity[s]
    assert np.abs(alpha[:n_c].sum(axis=0) - purity).max() <= MASS_TOL
    assert np.abs(alpha[n_c:].sum(axis=0) - (1 - purity)).max() <= MASS_TOL
    assert alpha.min() >= 0.0 and alpha.max() <= 1.0


def each(out, b):
    return out[0][b], out[1][b], float(out[2][b]), int(out[3][b])


def same(x, y):
    for a, b in zip(x, y):
        assert np.array_equal(a, b)


def stacks(runs):
    return np.stack([r.u0 for r in runs]), np.stack([r.a0 for r in runs])


@pytest.fixture(scope="module")
def toy_problem(ctx, toy):
    from demethify_amd.device import Problem

    V, D, ref, _ = toy
    with Problem(ctx, V, D, ref) as p:
        yield p


# ---- 1. toy restarts: W = 2 with a ragged slab, S = 10 leaves six sample rows of the last wave idle --------------------

def test_toy_purity_restarts_in_one_call(toy_problem):
    from demethify_amd import _lib as L
    from demethify_amd.device import mid_solve_plan

    runs = cases.toy_restarts()
    cases.check_preconditions("toy restart", runs, TOL)
    assert mid_solve_plan(350, 10, ROWS)[:2] == (256, 2)
    purity = 1 - P / 100
    out = toy_problem.solve_many_mid(*stacks(runs), L.DMF_MODE_PARTIAL, 100, 500, TOL, rows_per_workgroup=ROWS, purity=purity)
    for b, r in enumerate(runs):
        hold(each(out, b), r, 5, purity)
    assert int(out[3][0]) == len(runs[0].trace) == 7
    assert np.abs(out[1][0] - read_props("purity")).max() <= TIGHT
    assert np.abs(out[0][0] - read_profile("purity")).max() <= TIGHT


# ---- 2. toy bootstrap replicates through idx ---------------------------------------------------------------------------

@pytest.mark.parametrize("n_iter2", [20, 500])
def test_toy_purity_bootstrap_replicates_through_idx(toy_problem, n_iter2):
    """Purity P / 100 (what bt_ci uses): the sample at 1.0 has an unknown block of mass 0.  At 100 x 20 all 24 replicates
    meet the preconditions; at 100 x 500 those of the first 24 that do are taken, and at least 12 must (15 on record)."""
    from demethify_amd import _lib as L

    idx, runs = cases.toy_replicates(n_iter2)
    chosen = list(range(24)) if n_iter2 == 20 else [b for b in range(24) if cases.qualifies(runs[b])]
    print(f"replicates taken: {chosen}")
    assert len(chosen) >= 12
    runs = [runs[b] for b in chosen]
    cases.check_preconditions(f"toy replicate 100 x {n_iter2}", runs, TOL)
    purity = P / 100
    assert purity[6] == 1.0
    out = toy_problem.solve_many_mid(*stacks(runs), L.DMF_MODE_PARTIAL, 100, n_iter2, TOL, idx=idx[chosen],
                                     rows_per_workgroup=ROWS, purity=purity)
    for b, r in enumerate(runs):
        hold(each(out, b), r, 5, purity)
    assert np.all(out[1][:, 5, 6] == 0.0)  # (mass 0: the unknown row of that sample is exactly zero after one step)


# ---- 3. edge shapes ----------------------------------------------------------------------------------------------------

EDGE_ROWS = [edge + (ROWS,) for edge in cases.EDGES] + [(1000, 64, 12, 4, 20, 512)]


@pytest.mark.parametrize("N,S,n_c,n_u,n_iter2,rows", EDGE_ROWS)
def test_purity_edge_shapes_fixed_iterations(ctx, N, S, n_c, n_u, n_iter2, rows):
    """tol = 0 never satisfies the stop test: exactly three outer iterations on both sides.  (64, 1, 1, 1): one sample,
    one-row blocks; (257, 3): a one-row slab; (65, 64): every sample row of a 1 024-thread workgroup; (777, 33): one sample
    beyond a multiple of 16 and of 4; (2049, 17, 15, 1): nine slabs, K = 16 fills every lane, and the one Frank-Wolfe step per
    outer iteration puts every block on a vertex exactly -- bit-identical alpha."""
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, mid_solve_plan

    (V, D, Rt), purity, runs = cases.edge_runs(N, S, n_c, n_u, n_iter2)
    cases.check_preconditions(f"edge {(N, S, n_c, n_u, n_iter2)}", runs, 0.0)
    assert mid_solve_plan(N, S, rows)[1] == -(-N // rows)
    with Problem(ctx, V, D, Rt) as p:
        out = p.solve_many_mid(*stacks(runs), L.DMF_MODE_PARTIAL, cases.EDGE_ITERS, n_iter2, 0.0, rows_per_workgroup=rows,
                               purity=purity)
    for b, r in enumerate(runs):
        assert len(r.trace) == cases.EDGE_ITERS
        hold(each(out, b), r, n_c, purity)
        if n_iter2 == 1:
            assert np.array_equal(out[1][b], r.alpha)


# ---- 4. determinism, bit for bit ---------------------------------------------------------------------------------------

def test_a_purity_solve_does_not_depend_on_its_slot_or_its_neighbours(toy_problem):
    """The same solve alone and in slots 0, 7 and 39 of B = 40, the other slots holding other solves."""
    from demethify_amd import _lib as L

    runs = cases.toy_restarts()
    purity = 1 - P / 100
    alone = toy_problem.solve_many_mid(runs[0].u0[None], runs[0].a0[None], L.DMF_MODE_PARTIAL, 100, 500, TOL,
                                       rows_per_workgroup=ROWS, purity=purity)
    B = 40
    u0s = np.stack([runs[b % 15 + 1].u0 for b in range(B)])
    a0s = np.stack([runs[b % 15 + 1].a0 for b in range(B)])
    for slot in (0, 7, B - 1):
        u0s[slot], a0s[slot] = runs[0].u0, runs[0].a0
    many = toy_problem.solve_many_mid(u0s, a0s, L.DMF_MODE_PARTIAL, 100, 500, TOL, rows_per_workgroup=ROWS, purity=purity)
    assert int(alone[3][0]) == len(runs[0].trace)
    for slot in (0, 7, B - 1):
        same(each(alone, 0), each(many, slot))
    assert int(many[3][1]) == len(runs[2].trace)  # (slot 1 is seed 3's solve, stopping where the oracle's does)


def test_purity_results_do_not_depend_on_check_every_the_index_or_the_call(toy, toy_problem):
    """check_every of 1, 7 and the default agree; idx = arange(N) equals no index; a repeated call gives the same."""
    from demethify_amd import _lib as L

    N = toy[0].shape[0]
    runs = cases.toy_restarts()[:4]
    u0s, a0s = stacks(runs)
    purity = 1 - P / 100
    kw = dict(rows_per_workgroup=ROWS, purity=purity)
    want = toy_problem.solve_many_mid(u0s, a0s, L.DMF_MODE_PARTIAL, 100, 500, TOL, **kw)
    assert [int(i) for i in want[3]] == [len(r.trace) for r in runs]
    same(want, toy_problem.solve_many_mid(u0s, a0s, L.DMF_MODE_PARTIAL, 100, 500, TOL, **kw))
    same(want, toy_problem.solve_many_mid(u0s, a0s, L.DMF_MODE_PARTIAL, 100, 500, TOL, idx=np.tile(np.arange(N), (4, 1)), **kw))
    for every in (1, 7):
        same(want, toy_problem.solve_many_mid(u0s, a0s, L.DMF_MODE_PARTIAL, 100, 500, TOL, check_every=every, **kw))


# ---- 5. bad arguments and untouched inputs -----------------------------------------------------------------------------

def test_purity_bad_arguments_and_untouched_inputs(ctx, toy, toy_problem):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem

    V, D, ref, _ = toy
    N = V.shape[0]
    runs = cases.toy_restarts()[:2]
    u0s, a0s = (x.copy() for x in stacks(runs))
    idx = np.tile(np.arange(N)[::-1], (2, 1))
    purity = (1 - P / 100).copy()
    keep = [x.copy() for x in (u0s, a0s, idx, purity)]
    with pytest.raises(ValueError, match="purity"):
        toy_problem.solve_many_mid(u0s, a0s, L.DMF_MODE_PARTIAL, 3, 5, 0.0, purity=purity[:9])
    with pytest.raises(ValueError, match="purity"):
        toy_problem.solve_many_mid(u0s, a0s, L.DMF_MODE_UNSUPERVISED, 3, 5, 0.0, purity=purity)
    one = np.empty(1)

    def raw(problem, purity_ptr, mode):
        return problem._lib.dmf_solve_mid_purity(ctx._h, problem._h, 1, None, u0s.ctypes.data, a0s.ctypes.data, purity_ptr, 1, mode,
                                                 1, 1, 0.0, 0, 0, 0, one.ctypes.data, one.ctypes.data, one.ctypes.data,
                                                 one.ctypes.data)

    with Problem(ctx, V, D, None) as bare:
        with pytest.raises(ValueError, match="purity"):
            bare.solve_many_mid(u0s, a0s[:, 5:], L.DMF_MODE_PARTIAL, 3, 5, 0.0, purity=purity)
        # the C entry refuses the same on its own account, before any launch
        for mode in (L.DMF_MODE_PARTIAL, L.DMF_MODE_UNSUPERVISED):
            assert raw(bare, purity.ctypes.data, mode) == L.DMF_ERR_BAD_ARG
    assert raw(toy_problem, purity.ctypes.data, L.DMF_MODE_UNSUPERVISED) == L.DMF_ERR_UNSUPPORTED
    assert raw(toy_problem, None, L.DMF_MODE_PARTIAL) == L.DMF_ERR_BAD_ARG
    mask = np.ones(V.shape, dtype=bool)
    mask[::7, 3] = False
    with toy_problem.masked(mask) as held:
        with pytest.raises(L.DemethifyHipError) as e:
            held.solve_many_mid(u0s, a0s, L.DMF_MODE_PARTIAL, 3, 5, 0.0, purity=purity)
    assert e.value.status == L.DMF_ERR_BAD_ARG
    before = {name: toy_problem.copy_out(name) for name in ("V", "D", "Rt")}
    toy_problem.solve_many_mid(u0s, a0s, L.DMF_MODE_PARTIAL, 3, 5, 0.0, idx=idx, purity=purity)
    for got, want in zip((u0s, a0s, idx, purity), keep):
        assert np.array_equal(got, want)
    for name, want in before.items():
        assert np.array_equal(toy_problem.copy_out(name), want)
    # purity=None is the call without the keyword
    same(toy_problem.solve_many_mid(u0s, a0s, L.DMF_MODE_PARTIAL, 3, 5, 0.0, idx=idx, purity=None),
         toy_problem.solve_many_mid(u0s, a0s, L.DMF_MODE_PARTIAL, 3, 5, 0.0, idx=idx))


# ---- 6. drivers --------------------------------------------------------------------------------------------------------

def test_bt_ci_mid_purity_matches_the_oracle_bounds(tmp_path, toy, monkeypatch):
    from demethify_amd import bootstrap
    from demethify_amd.device import Problem

    V, D, ref, header = toy
    _, runs = cases.toy_replicates(20)
    cases.check_preconditions("toy replicate 100 x 20", runs, TOL)
    calls = []
    real = Problem.solve_many_mid
    monkeypatch.setattr(Problem, "solve_many_mid",
                        lambda self, *a, **k: calls.append((len(a[0]), k.get("purity") is not None)) or real(self, *a, **k))
    monkeypatch.setattr(Problem, "solve_many", lambda *a, **k: calls.append("solve_many"))
    samples = [f"s{k}" for k in range(V.shape[1])]
    props, (lower_u, upper_u) = bootstrap.bt_ci(95, 24, 1, V, D, ref, "uniform_", 100, 20, TOL, header, str(tmp_path), samples,
                                                list(P), 1, materialize=False, batched=True, batch_kernel="mid",
                                                batched_mid_purity=True)
    assert calls == [(24, True)]
    lo_a, hi_a = odrv.percentile_bounds(np.stack([r.alpha for r in runs]), 95)
    lo_u, hi_u = odrv.percentile_bounds(np.stack([r.u for r in runs]), 95)
    got = np.array([[cell for cell in props[col]] for col in props.columns])  # (S, K, 2)
    assert np.abs(got[:, :, 0].T - lo_a).max() <= TIGHT and np.abs(got[:, :, 1].T - hi_a).max() <= TIGHT
    assert np.abs(lower_u - lo_u).max() <= TIGHT and np.abs(upper_u - hi_u).max() <= TIGHT
    assert (tmp_path / "confidence_interval_celltypes_proportions.csv").exists()
    assert (tmp_path / "confidence_interval_methylation_estimate.csv").exists()


def test_command_line_mid_purity_restarts_pick_the_oracle_winner(tmp_path, toy, monkeypatch):
    """DEMETHIFY_BATCH_MID_PURITY=1 --purity P --restart 8 on the toy, the gate moved around the toy's size: the restarts go
    through solve_many_mid with the purity vector, and the winner is the one an oracle loop over the seeds
    restart_seed(1, k) = 1..8 picks (strict '<': the first minimum), its CSVs within 1e-8."""
    from demethify_amd import bootstrap, demethify, shard
    from demethify_amd.device import Problem

    V = toy[0]
    assert [shard.restart_seed(1, k) for k in range(8)] == list(range(1, 9))
    runs = cases.toy_restarts()[:8]
    cases.check_preconditions("toy restart", runs, TOL)
    costs = np.array([r.trace[-1] for r in runs])
    want_k = int(np.argmin(costs))
    ordered = np.sort(costs)
    # each cost is held to COST_RTOL; a gap of ten times that cannot be closed by two such errors
    print(f"oracle costs {costs}, two best {(ordered[1] - ordered[0]) / ordered[0]:.2e} apart")
    assert (ordered[1] - ordered[0]) / ordered[0] > 10 * COST_RTOL
    calls = []
    real = Problem.solve_many_mid
    monkeypatch.setattr(Problem, "solve_many_mid",
                        lambda self, *a, **k: calls.append((len(a[0]), k.get("purity") is not None)) or real(self, *a, **k))
    monkeypatch.setattr(Problem, "solve_many", lambda *a, **k: calls.append("solve_many"))
    monkeypatch.setattr(bootstrap, "MID_BATCH_PURITY_MIN_ELEMENTS", V.size)
    monkeypatch.setattr(bootstrap, "MID_BATCH_PURITY_MAX_ELEMENTS", V.size)
    monkeypatch.delenv("DEMETHIFY_BATCH", raising=False)
    monkeypatch.delenv("DEMETHIFY_BATCH_MID", raising=False)
    monkeypatch.setenv("DEMETHIFY_BATCH_MID_PURITY", "1")
    out = tmp_path / "out"
    samples = [str(UPSTREAM / "output_gen" / f"sample{i}.bed") for i in range(1, 11)]
    demethify.main(["--ref", str(UPSTREAM / "output_gen" / "ref_matrix.bed"), "--methfreq", *samples, "--bedmethyl", "--noprint",
                    "--nbunknown", "1", "--restart", "8", "--purity", *[str(int(p)) for p in P], "--outdir", str(out)])
    assert calls == [(8, True)]
    got_alpha = pd.read_csv(out / "celltypes_proportions.csv", index_col=0, float_precision="round_trip").values
    got_u = pd.read_csv(out / "methylation_profile_estimate.csv", float_precision="round_trip").values
    assert np.abs(got_alpha - runs[want_k].alpha).max() <= TIGHT and np.abs(got_u - runs[want_k].u).max() <= TIGHT
    others = [r.alpha for k, r in enumerate(runs) if k != want_k]
    assert min(np.abs(got_alpha - o).max() for o in others) > 1e-6  # (no other restart's proportions would pass)
