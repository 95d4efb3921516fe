"""The row pass on the methylated read counts (X16: x = rint(v d) as u16, built by dmf_problem_create when every element
is an exact x / d): which inputs take it, and that it computes what the row pass on V computes.

Each problem is created twice in one process, once with the context's X16 switch off (every kernel reads V, as before)
and once with it on; the describe token " x16" tells which path a solver is on."""
import numpy as np
import pytest

from oracle import solver as osol

from conftest import rel_err

pytestmark = pytest.mark.gpu

TIGHT = 1e-8   # oracle parity, as in tests/test_gpu_bench_paths.py
PATHS = 1e-12  # the two paths against each other


def _describe(ctx, V, D, Rt, n_u=2, x16=True):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    S = V.shape[1]
    n_c = 0 if Rt is None else Rt.shape[1]
    rs = np.random.RandomState(3)
    u0 = rs.uniform(size=(V.shape[0], n_u))
    a0 = rs.dirichlet(np.ones(n_c + n_u), S).T
    ctx.set_x16(x16)
    try:
        with Problem(ctx, V, D, Rt) as p, Solver(p, u0, a0, L.DMF_MODE_PARTIAL if n_c else L.DMF_MODE_UNSUPERVISED) as s:
            return s.describe(20)
    finally:
        ctx.set_x16(True)


def _small(seed=0):
    return osol.synthetic_problem(2048 + 3, 96, 6, 2, seed=seed, depth=40)


def test_x_over_d_is_accepted(ctx):
    V, D, Rt = _small()
    got = _describe(ctx, V, D, Rt)
    assert "k_rowpass_v2<2,2>" in got and " x16 " in got
    off = _describe(ctx, V, D, Rt, x16=False)
    assert "k_rowpass_v2<2,2>" in off and "x16" not in off


def test_percent_over_100_is_accepted(ctx):
    """modkit-style inputs: percent_modified = 100 x / d, the frequency read back as percent / 100 (the upstream .bed
    fixtures)."""
    V, D, Rt = _small(1)
    X = np.rint(V * D)
    pct = 100.0 * X / D
    assert " x16 " in _describe(ctx, pct / 100.0, D, Rt)


@pytest.mark.parametrize("what", ["perturbed", "non_integral", "x_above_d"])
def test_inexact_products_fall_back_to_v(ctx, what):
    V, D, Rt = _small(2)
    V = V.copy()
    if what == "perturbed":
        V[100, 7] += 1e-9
    elif what == "non_integral":
        V[5, 3] = (np.rint(V[5, 3] * D[5, 3]) + 0.3) / D[5, 3]
    else:
        V[2047, 95] = 1.0 + 1.0 / D[2047, 95]
    got = _describe(ctx, V, D, Rt)
    assert "k_rowpass_v2<2,2>" in got and "x16" not in got


def test_zero_count_with_nonzero_frequency_is_accepted(ctx):
    V, D, Rt = _small(3)
    V, D = V.copy(), D.copy()
    D[10, 11] = 0
    V[10, 11] = 0.7
    assert " x16 " in _describe(ctx, V, D, Rt)


def _solve(ctx, V, D, Rt, n_u, T1, x16, u0, a0):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    mode = L.DMF_MODE_PARTIAL if Rt is not None else L.DMF_MODE_UNSUPERVISED
    ctx.set_x16(x16)
    try:
        with Problem(ctx, V, D, Rt) as p, Solver(p, u0, a0, mode) as s:
            desc = s.describe(20)
            s.step(T1, 20, 0.0)
            u, alpha, _, _ = s.get()
    finally:
        ctx.set_x16(True)
    assert "k_rowpass_v2" in desc and (" x16 " in desc) == x16, desc
    return u, alpha


CASES = [
    (40_000, 256, 12, 4, "the bench's shape in everything but the row count"),
    (8192 + 3, 255, 12, 4, "odd S, ragged last column group"),
    (4096 + 5, 512, 12, 4, "eight-wave form"),
    (3000, 128, 0, 4, "unsupervised gradient point, no known types"),
]


@pytest.mark.parametrize("N,S,n_c,n_u,why", CASES)
def test_both_paths_agree_and_match_the_oracle(ctx, N, S, n_c, n_u, why):
    T1 = 3
    V, D, Rt = osol.synthetic_problem(N, S, n_c, n_u, seed=0, depth=50)
    if n_c:
        u0, R, a0 = osol.init_partial("uniform_", V, D, Rt, n_u, seed=1)
        wu, wa = osol.solve_partial(u0.copy(), R, a0.copy(), V, D, Rt, n_u, T1, 20, 0.0,
                                    project=osol.simplex_project_columns_fast)
    else:
        Rt = None
        u0, a0 = osol.init_unsupervised("uniform_", V, n_u, seed=1)
        wu, wa = osol.solve_unsupervised(V, n_u, D, "uniform_", T1, 20, 0.0, init=(u0.copy(), a0.copy()),
                                         project=osol.simplex_project_columns_fast)
    u_v, a_v = _solve(ctx, V, D, Rt, n_u, T1, False, u0, a0)
    u_x, a_x = _solve(ctx, V, D, Rt, n_u, T1, True, u0, a0)
    assert rel_err(a_x, a_v) <= PATHS and rel_err(u_x, u_v) <= PATHS, (rel_err(a_x, a_v), rel_err(u_x, u_v))
    assert rel_err(a_x, wa) < TIGHT and np.abs(u_x - wu).max() < TIGHT


def test_bootstrap_replicate_keeps_the_path(ctx):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    N, S, n_c, n_u = 6000, 128, 6, 2
    V, D, Rt = osol.synthetic_problem(N, S, n_c, n_u, seed=4, depth=50)
    idx = np.random.RandomState(5).randint(0, N, size=N)
    u0, _, a0 = osol.init_partial("uniform_", V[idx], D[idx], Rt[idx], n_u, seed=1)
    out = {}
    for x16 in (False, True):
        ctx.set_x16(x16)
        try:
            with Problem(ctx, V, D, Rt) as p:
                with p.gather(idx) as r, Solver(r, u0, a0, L.DMF_MODE_PARTIAL) as s:
                    desc = s.describe(20)
                    s.step(2, 20, 0.0)
                    out[x16] = s.get()[:2]
        finally:
            ctx.set_x16(True)
        assert "k_rowpass_v2<2,2>" in desc and (" x16 " in desc) == x16, desc
    assert rel_err(out[True][1], out[False][1]) <= PATHS and rel_err(out[True][0], out[False][0]) <= PATHS
    # the replicate itself, created directly, solves to the same place
    with Problem(ctx, V[idx], D[idx], Rt[idx]) as p, Solver(p, u0, a0, L.DMF_MODE_PARTIAL) as s:
        s.step(2, 20, 0.0)
        u_d, a_d = s.get()[:2]
    assert rel_err(out[True][1], a_d) <= PATHS and rel_err(out[True][0], u_d) <= PATHS
