"""The reference-based regression's kernels held to exact sums and to every branch of the active-set loop (cases, models and
bounds: tests/wls_model.py; the CPU side: tests/test_wls_model_host.py).

  * k_wls_moments<u16 | f64> + k_wls_reduce through Problem.wls_moments: bit for bit on the dyadic family over the table
    wls_model.MOMENT_CASES (fewer rows than a workgroup, second and third trip of the grid-stride loop, 64-sample block edges,
    the 16-column slice boundaries, the known / unknown split, both targets, both templates, rows without coverage), and
    inside the derived bound on real inputs;
  * k_nnls_intercept through Context.nnls_normal on constructed normal equations: 32 correlated systems per K = 1 .. 64 (each
    batch drops variables), the named single systems (two variables dropped in one step, two consecutive step-backs, a tie of
    the largest duals, a dropped variable that re-enters), and batches that interleave the statuses 0, 1 and 2 -- against
    scipy.optimize.nnls at the regression's bar of 1e-10;
  * the public route, Problem.wls_intercept, on problems whose samples drop variables, on 8193 and 16385 rows and on a
    gathered problem of 9000 rows, against the oracle.

No case exists for a rejected candidate, an emptied passive set or the 3 K cap: wls_model's docstring says what was searched.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from oracle import solver as osol

import wls_model as wm
from test_gpu_wls import TOL, draw_u, oracle_wls

pytestmark = pytest.mark.gpu


def open_problem(ctx, c, V, D, Rt):
    """The problem of a moments case, with the plan the case means to cover asserted on the live problem."""
    from demethify_amd.device import Problem

    p = Problem(ctx, V, D, Rt)
    r = p.report()
    has_copies = bool(r["has_D16"] and r["has_X16"])
    assert has_copies == (c.form != "f64_plain"), (c, r)
    return p


# ------------------------------------------------------------------------------------------------ moments, bit for bit
@pytest.mark.parametrize("c", wm.MOMENT_CASES, ids=wm.moment_case_id)
def test_dyadic_moments_are_exact(ctx, c):
    V, D, Rt, u = wm.dyadic_moment_data(c)
    want = wm.exact_moments(V, D, wm.full_R(Rt, u), c.target)
    assert want.exact and want.table.max() * 256.0 < 2.0 ** 53
    K = c.n_c + c.n_u
    with open_problem(ctx, c, V, D, Rt) as p:
        got = p.wls_moments(u, c.target, f64_arrays=c.form == "f64_flag")
        other = p.wls_moments(u, c.target, f64_arrays=c.form != "f64_flag") if c.form != "f64_plain" else None
    wrong = int((got != want.table).sum())
    print(f"DEV moments {wm.moment_case_id(c)}: trips={wm.moments_trips(c.N)} grid={wm.moments_grid(c.N)} "
          f"slices={(K + wm.SLICE - 1) // wm.SLICE} entries differing {wrong} of {got.size}")
    assert np.array_equal(got[2 * K:], want.table[2 * K:]), "sw / st (written by column slice 0 alone)"
    assert np.array_equal(got[:K], want.table[:K]), "m"
    assert np.array_equal(got[K:2 * K], want.table[K:2 * K]), "r"
    if other is not None:
        assert np.array_equal(other, got), "the u16 and the f64 form differ on the same data"


# ------------------------------------------------------------------------------------------------ moments, real inputs
@pytest.mark.parametrize("c", wm.GENERAL_MOMENT_CASES, ids=wm.moment_case_id)
def test_general_moments_stay_inside_the_derived_bound(ctx, c):
    V, D, Rt, u = wm.general_moment_data(c)
    want = wm.exact_moments(V, D, wm.full_R(Rt, u), c.target)
    assert not want.exact
    with open_problem(ctx, c, V, D, Rt) as p:
        got = p.wls_moments(u, c.target, f64_arrays=c.form == "f64_flag")
    ratio = wm.moment_ratio(got, want, c.N)
    print(f"DEV moments {wm.moment_case_id(c)}: n_terms={wm.moment_terms(c.N)} |got - exact| / bound = {ratio:.3f}")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ the solver
def solve_batch(ctx, systems):
    G = np.stack([s.A for s in systems])
    B = np.stack([s.b for s in systems], axis=1)
    got, status = ctx.nnls_normal(G, wm.plain_moments(B))
    want = np.stack([wm.scipy_proportions(s.M, s.y) for s in systems], axis=1)
    return got, status, want


@pytest.mark.parametrize("K", range(1, 65))
def test_correlated_systems_against_scipy(ctx, K):
    """32 systems per K in one launch; tests/test_wls_model_host.py shows that each batch beyond K = 1 drops variables."""
    got, status, want = solve_batch(ctx, wm.correlated_batch(K))
    err = float(np.abs(got - want).max())
    print(f"DEV nnls K={K}: max abs diff to scipy {err:.3e}, status {sorted(set(status.tolist()))}")
    assert (status == 0).all()
    assert err <= TOL


@pytest.mark.parametrize("name", sorted(wm.NAMED_EVIDENCE))
def test_named_systems(ctx, name):
    s = wm.named_systems()[name]
    got, status, want = solve_batch(ctx, [s])
    err = float(np.abs(got - want).max())
    print(f"DEV nnls {name}: max abs diff to scipy {err:.3e}, proportions {got[:, 0].tolist()}")
    assert status.tolist() == [0]
    assert err <= TOL
    if name == "two_drops_at_once":  # (every operation of this solve is exact but the final division)
        x = np.array([0.0, 0.0, 2.5 / (9.0 / 64.0), 0.5])
        assert np.array_equal(got[:, 0], x / x.sum())


@pytest.mark.parametrize("S", [1, 2, 65, 300])
def test_statuses_interleaved(ctx, S):
    """Statuses 0, 1 and 2 in one launch: the columns that were not solved come back untouched (the wrapper's NaN), the
    solved ones are right."""
    G, mom, want_status, systems = wm.status_batch(S)
    got, status = ctx.nnls_normal(G, mom)
    print(f"DEV nnls statuses S={S}: {np.bincount(status, minlength=3).tolist()} samples with status 0 / 1 / 2")
    assert np.array_equal(status, want_status)
    solved = status == 0
    assert np.isnan(got[:, ~solved]).all()
    want = np.stack([wm.scipy_proportions(systems[s].M, systems[s].y) for s in np.flatnonzero(solved)], axis=1)
    assert np.abs(got[:, solved] - want).max() <= TOL


# ------------------------------------------------------------------------------------------------ the public route
def check_route(got, status, want, label):
    err = float(np.abs(got - want).max())
    print(f"DEV wls {label}: max abs diff to the oracle {err:.3e}")
    assert (status == 0).all()
    assert err <= TOL


@pytest.mark.parametrize("target", ["v", "dv"])
@pytest.mark.parametrize("K", wm.ROUTE_K)
def test_route_on_samples_that_drop_variables(ctx, K, target):
    from demethify_amd.device import Problem

    V, D, R = wm.route_problem(K)
    want = oracle_wls(V, D, R, target)
    with Problem(ctx, V, D, R) as p:
        r = p.report()
        assert bool(r["has_D16"] and r["has_X16"]) == (K <= 48)  # (more than 48 known types: the f64 form)
        got = p.wls_intercept(None, target)
        check_route(got, p.wls_status, want, f"K={K} N={K + 6} S=64 target={target}")


@functools.lru_cache(maxsize=None)
def long_case(N):
    V, D, Rt = osol.synthetic_problem(N, 5, 6, 2)
    u = draw_u(N, 2)
    want = {t: oracle_wls(V, D, np.c_[Rt, u], t) for t in ("v", "dv")}
    for a in (V, D, Rt, u) + tuple(want.values()):
        a.setflags(write=False)
    return V, D, Rt, u, want


@pytest.mark.parametrize("target", ["v", "dv"])
@pytest.mark.parametrize("N", [8193, 16385])
def test_route_beyond_one_trip(ctx, N, target):
    from demethify_amd.device import Problem

    V, D, Rt, u, want = long_case(N)
    assert wm.moments_trips(N) == (2 if N == 8193 else 3)
    with Problem(ctx, V, D, Rt) as p:
        assert p.report()["has_X16"]
        got = p.wls_intercept(u, target)
        check_route(got, p.wls_status, want[target], f"N={N} S=5 6+2 target={target}")


def test_route_on_a_gathered_problem_of_9000_rows(ctx):
    from demethify_amd.device import Problem
    from demethify_amd.staging import indices_to_device

    V, D, Rt = osol.synthetic_problem(3000, 6, 5, 0)
    idx = np.random.RandomState(5).randint(0, 3000, size=9000)
    want = oracle_wls(V[idx], D[idx], Rt[idx], "dv")
    with Problem(ctx, V, D, Rt) as full, full.gather(indices_to_device(idx, ctx)) as resampled:
        assert resampled.report()["N"] == 9000 and wm.moments_trips(9000) == 2
        got = resampled.wls_intercept(None, "dv")
        check_route(got, resampled.wls_status, want, "gathered 9000 x 6, 5 known")
        mom = resampled.wls_moments(None, "dv")
    ref = wm.exact_moments(V[idx], D[idx], Rt[idx], "dv")
    ratio = wm.moment_ratio(mom, ref, 9000)
    print(f"DEV moments gathered 9000 x 6: |got - exact| / bound = {ratio:.3f}")
    assert ratio <= 1.0
