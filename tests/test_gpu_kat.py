"""Per-function known-answer tests of the HIP path against the CPU oracle.
All calls go through the C-ABI (demethify_amd.device / demethify_amd.deconvolution)."""
import numpy as np
import pytest

from oracle import solver as osol

from conftest import rel_err

pytestmark = pytest.mark.gpu

SHAPES = [  # (N, S, n_c, n_u)
    (257, 7, 6, 1), (1000, 64, 6, 2), (513, 100, 0, 4), (300, 10, 5, 3), (2048, 130, 12, 4), (129, 33, 3, 8),
]
# ... and for the cost alone, real-valued data on each two-samples-per-lane form and on the any-shape kernel
COST_SHAPES = SHAPES + [(200, 129, 3, 2), (150, 64, 2, 7), (60, 20, 17, 1)]
COST_KERNELS = ["k_cost_cols<2,1,u16>", "k_cost_cols<2,2,u16>", "k_cost_cols<0,4,u16>", "k_cost_cols<2,3,u16>",
                "k_cost_cols2<3,4,even>", "k_cost_cols2<1,8,odd>", "k_cost_cols2<1,2,odd>", "k_cost_cols2<1,7,even>",
                "k_cost alpha=lds"]


def _problem(N, S, n_c, n_u, seed):
    V, D, Rt = osol.synthetic_problem(N, S, n_c, n_u, seed=seed, depth=20)
    rs = np.random.RandomState(seed + 100)
    u = rs.uniform(size=(N, n_u))
    alpha = rs.dirichlet(np.ones(n_c + n_u), S).T
    return V, D, Rt, u, alpha, rs


@pytest.mark.parametrize("N,S,n_c,n_u", COST_SHAPES)
def test_cost_matches_oracle(ctx, N, S, n_c, n_u):
    """cost_f_w on real-valued data against sum d e e in extended precision (no sqrt(d), which oracle.solver.weighted_cost
    goes through), on the kernel the shape is listed for."""
    from demethify_amd.device import Problem

    kernel = COST_KERNELS[COST_SHAPES.index((N, S, n_c, n_u))]
    V, D, Rt, u, alpha, _ = _problem(N, S, n_c, n_u, 1)
    ld = np.longdouble
    e = V.astype(ld) - np.c_[Rt, u].astype(ld) @ alpha.astype(ld)
    want = float((D.astype(ld) * e * e).sum())
    with Problem(ctx, V, D, Rt if n_c else None) as p:
        assert p.cost_describe(n_u) == "cost=" + kernel
        got = p.cost(u, alpha)
    print(f"{kernel}: rel {abs(got - want) / abs(want):.2e}")
    assert abs(got - want) <= 1e-11 * abs(want)


def test_cost_f_w_reference_signature(ctx):
    from demethify_amd.deconvolution import cost_f_w

    V, D, Rt, u, alpha, _ = _problem(400, 12, 4, 2, 2)
    R = np.c_[Rt, u]
    assert abs(cost_f_w(V, R, alpha, D) - osol.weighted_cost(V, R, alpha, D)) <= 1e-11 * osol.weighted_cost(V, R, alpha, D)
    # float counts are accepted too (csv input without coverage column sets counts to 1)
    Df = D.astype(np.float64)
    assert abs(cost_f_w(V, R, alpha, Df) - osol.weighted_cost(V, R, alpha, Df)) <= 1e-11 * osol.weighted_cost(V, R, alpha, Df)


@pytest.mark.parametrize("K,S", [(1, 5), (2, 64), (5, 10), (8, 65), (16, 256), (17, 3), (30, 70), (64, 9)])
def test_projection_matches_oracle(ctx, K, S):
    rs = np.random.RandomState(K * 1000 + S)
    X = rs.randn(K, S) * rs.choice([0.05, 1.0, 20.0], size=(1, S))
    X[:, 0] = 0.0  # all-equal column
    if S > 2:
        X[:, 1] = np.linspace(0, 1, K)  # already sorted ascending
        X[:, 2] = X[0, 2]  # ties
    got = ctx.project_simplex(X)
    want = osol.simplex_project_columns(X)
    assert np.abs(got - want).max() <= 1e-14 * max(1.0, np.abs(X).max())
    assert np.allclose(got.sum(axis=0), 1.0, atol=1e-12)
    got2 = ctx.project_simplex(X, z=2.5)
    assert np.abs(got2 - osol.simplex_project_columns(X, z=2.5)).max() <= 1e-14 * max(1.0, np.abs(X).max())


# (a1, l_w_prev / l_w) of test_update_u_matches_oracle.  QUIET leaves (a1 - 1) / a_next below the cap 0.9999 sqrt(l_w_prev / l_w)
# throughout; under SQRT the cap decides the first inner step, under FLAT every one (tests/momentum_ref.py)
U_STATES = {"QUIET": (2.7, 0.8), "SQRT": (40.0, 0.5), "FLAT": (3e4, 1.0)}


def _update_u_cases():
    """(N, S, n_c, n_u, generic, state); the QUIET cases keep the ids they had before the other states came."""
    return [pytest.param(N, S, n_c, n_u, generic, state,
                         id=f"{N}-{S}-{n_c}-{n_u}-{generic}" + ("" if state == "QUIET" else "-" + state))
            for state in U_STATES for N, S, n_c, n_u in SHAPES for generic in (0, 1, 2, 3)]


@pytest.mark.parametrize("N,S,n_c,n_u,generic,state", _update_u_cases())
def test_update_u_matches_oracle(ctx, N, S, n_c, n_u, generic, state):
    """update_u with a NON-initial momentum state (a1 > 1, l_w_ != l_w or the cap at 0.9999, u_ != u)."""
    from demethify_amd.device import Problem

    V, D, Rt, u, alpha, rs = _problem(N, S, n_c, n_u, 3)
    u_prev = np.clip(u + 0.05 * rs.randn(N, n_u), 0, 1)
    d = float(D.max()) ** 2
    l_w = np.linalg.norm(alpha[-n_u:]) ** 2 * d
    a1, l_w_prev = U_STATES[state][0], U_STATES[state][1] * l_w
    want = osol.u_phase(u, alpha, 5, a1, l_w_prev, l_w, u_prev, V, Rt, n_u, D)
    ctx.set_generic(generic)
    try:
        with Problem(ctx, V, D, Rt if n_c else None) as p:
            got = p.update_u(u, u_prev, alpha, 5, a1, l_w_prev, l_w)
    finally:
        ctx.set_generic(0)
    assert np.abs(got[0] - want[0]).max() < 1e-11
    assert np.abs(got[1] - want[1]).max() < 1e-11
    assert got[2] == pytest.approx(want[2], rel=1e-15) and got[3] == want[3]


def test_update_u_unsupervised_gradient_point(ctx):
    """deconvolution.py:163: the unsupervised loop takes the gradient at the previous iterate."""
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem

    N, S, n_u = 700, 21, 3
    V, D, _, u, alpha, rs = _problem(N, S, 0, n_u, 4)
    u_prev = np.clip(u + 0.1 * rs.randn(N, n_u), 0, 1)
    d = float(D.max()) ** 2
    l_w = np.linalg.norm(alpha) ** 2 * d
    a1, l_prev = 1.9, 1.3 * l_w
    # oracle: two inner steps of the inline loop
    uo, uo_prev, a, lp = u, u_prev, a1, l_prev
    for _ in range(2):
        a0 = a
        a, beta = osol.momentum_step(a0, lp, l_w)
        ut = uo + beta * (uo - uo_prev)
        uo_prev = uo
        uo = np.clip(ut + (D * (V - uo @ alpha)) @ alpha.T / l_w, 0, 1)
        lp = l_w
    for generic in (0, 1, 2, 3):
        ctx.set_generic(generic)
        try:
            with Problem(ctx, V, D, None) as p:
                got = p.update_u(u, u_prev, alpha, 2, a1, l_prev, l_w, mode=L.DMF_MODE_UNSUPERVISED)
        finally:
            ctx.set_generic(0)
        assert np.abs(got[0] - uo).max() < 1e-11
        assert np.abs(got[1] - uo_prev).max() < 1e-11


def _alpha_cases():
    """(N, S, n_c, n_u, generic) of test_update_alpha_matches_oracle with the alpha kernel each must run.  The small shapes
    put K = n_c + n_u on both sides of every branch of the alpha kernels -- 2..16: the shortened sort, scan and product of
    k_alpha_phase_row16 and k_alpha_phase<4 / 8 / 16>; 17, 32: k_alpha_phase_lanes<32>; 33, 64: k_alpha_phase_lanes<64>;
    17..64: k_alpha_phase_dyn -- each with and without known types, at sample counts ragged against the columns of a wave
    (4 for row16, 2 for lanes<32>, 64 for the thread-per-sample kernels of level 1)."""
    cases = []
    for generic in (0, 1):
        tag = "" if generic == 0 else "-level1"
        for N, S, n_c, n_u in SHAPES + [(500, 20, 10, 10), (400, 6, 5, 25)]:
            cases.append(pytest.param(N, S, n_c, n_u, generic, id=f"{N}-{S}-{n_c}-{n_u}{tag}"))
        for K in (2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 32, 33, 64):
            sizes = (3, 66) if generic == 1 else (3, 5) if K <= 16 else (5,) if K <= 32 else (3,)
            for S in sizes:
                for n_c in (0, K // 2):
                    cases.append(pytest.param(300, S, n_c, K - n_c, generic, id=f"300-{S}-{n_c}-{K - n_c}{tag}"))
    return cases


def _alpha_kernel(K, generic):
    if generic == 1:
        return "k_alpha_phase" if K <= 16 else "k_alpha_phase_dyn"
    return "k_alpha_phase_row16" if K <= 16 else "k_alpha_phase_lanes"


@pytest.mark.parametrize("N,S,n_c,n_u,generic", _alpha_cases())
def test_update_alpha_matches_oracle(ctx, N, S, n_c, n_u, generic):
    from demethify_amd.device import Problem, Solver

    V, D, Rt, u, alpha, rs = _problem(N, S, n_c, n_u, 5)
    alpha_prev = rs.dirichlet(np.ones(n_c + n_u), S).T
    R = np.c_[Rt, u]
    d = float(D.max()) ** 2
    l_h = np.linalg.norm(R) ** 2 * d
    a2, l_h_prev = 3.1, 1.1 * l_h
    want = osol.alpha_phase(4, alpha, a2, l_h_prev, l_h, alpha_prev, R, D, V)
    ctx.set_generic(generic)
    try:
        with Problem(ctx, V, D, Rt if n_c else None) as p:
            got = p.update_alpha(u, alpha, alpha_prev, 4, a2, l_h_prev, l_h)
            with Solver(p, u, alpha) as s:
                path = s.describe(4)
    finally:
        ctx.set_generic(0)
    print(f"max |alpha - oracle| = {np.abs(got[0] - want[0]).max():.3e}, "
          f"max |alpha_prev - oracle| = {np.abs(got[1] - want[1]).max():.3e}  ({path})")
    assert path.endswith("alpha=" + _alpha_kernel(n_c + n_u, generic))
    assert np.abs(got[0] - want[0]).max() < 1e-10
    assert np.abs(got[1] - want[1]).max() < 1e-10
    assert got[2] == pytest.approx(want[2], rel=1e-15) and got[3] == want[3]


def test_reference_signatures_update_functions(ctx):
    from demethify_amd import deconvolution as dd

    V, D, Rt, u, alpha, rs = _problem(300, 9, 4, 2, 6)
    R = np.c_[Rt, u]
    d = float(D.max()) ** 2
    l_w = np.linalg.norm(alpha[-2:]) ** 2 * d
    l_h = np.linalg.norm(R) ** 2 * d
    got = dd.update_u(u, alpha, 3, 1.0, l_w, l_w, u.copy(), V, Rt, 2, D)
    want = osol.u_phase(u, alpha, 3, 1.0, l_w, l_w, u.copy(), V, Rt, 2, D)
    assert np.abs(got[0] - want[0]).max() < 1e-11 and got[2] == pytest.approx(want[2])
    got = dd.update_alpha(3, alpha, 1.0, l_h, l_h, alpha.copy(), R, D, V)
    want = osol.alpha_phase(3, alpha, 1.0, l_h, l_h, alpha.copy(), R, D, V)
    assert np.abs(got[0] - want[0]).max() < 1e-10
    assert np.abs(dd.projection_simplex_sort_2d(alpha * 3) - osol.simplex_project_columns(alpha * 3)).max() < 1e-14


def test_gather_rows_matches_fancy_indexing(ctx):
    from demethify_amd.device import Problem

    V, D, Rt, u, alpha, rs = _problem(600, 11, 5, 2, 7)
    idx = osol.bootstrap_indices(11, 600)
    with Problem(ctx, V, D, Rt) as p, p.gather(idx) as q:
        got = q.cost(u, alpha)
    want = osol.weighted_cost(V[idx], np.c_[Rt[idx], u], alpha, D[idx])
    assert abs(got - want) <= 1e-11 * want
    # the same resample from row indices that are already in HBM (what the bootstrap driver's worker thread uploads)
    from demethify_amd.staging import indices_to_device

    with Problem(ctx, V, D, Rt) as p, p.gather(indices_to_device(idx, ctx)) as q:
        assert q.N == idx.size
        assert q.cost(u, alpha) == got


def test_bad_arguments_raise(ctx):
    from demethify_amd._lib import DemethifyHipError
    from demethify_amd.device import Problem, Solver

    V, D, Rt, u, alpha, _ = _problem(100, 5, 3, 2, 8)
    with pytest.raises(ValueError):
        Problem(ctx, V, D[:, :4], Rt)
    with pytest.raises(ValueError):
        Problem(ctx, np.where(V > 2, V, np.nan), D, Rt)
    with Problem(ctx, V, D, Rt) as p:
        with pytest.raises(ValueError):
            Solver(p, u, alpha[:-1])
        with pytest.raises(DemethifyHipError):
            p.gather(np.array([0, 100]))
        from demethify_amd.staging import indices_to_device

        for bad in ([0, 100], [-1, 5], [3, 1 << 40]):  # (range-checked on the device before any row is read)
            with pytest.raises(DemethifyHipError):
                p.gather(indices_to_device(np.array(bad), ctx))
        with p.gather(indices_to_device(np.array([99, 0, 99]), ctx)) as q:
            assert q.N == 3


@pytest.mark.parametrize("n,m,q", [
    (500, 1000, [2.5, 97.5]),     # the usual 95 % interval: both order statistics in the register tails
    (200, 777, [5.0, 95.0]),
    (40, 513, [0.0, 100.0]),      # extremes: no interpolation
    (500, 300, [25.0, 75.0]),     # inside the column: ranking kernel
    (3000, 65, [50.0, 2.5]),      # mixed: one in a tail, one not -> ranking kernel, 4 positions per workgroup
    (1, 10, [2.5, 97.5]),
    (2, 10, [30.0]),
    (33, 129, [10.0, 50.0, 99.0]),  # an odd number of percentiles
])
def test_percentile_axis0_is_numpy_bit_for_bit(ctx, n, m, q):
    """bootstrap.py:51-54 / :75-78: np.percentile(stack, q, axis=0), default "linear" method.  numpy itself is
    the reference here; the kernel repeats its interpolation operation by operation, so equality is exact."""
    rs = np.random.RandomState(n + m)
    x = rs.uniform(size=(n, m))
    x[:, ::7] = np.round(x[:, ::7], 1)  # heavy ties in some columns
    x[:, 3 % m] = 0.25                  # a constant column
    want = np.percentile(x, q, axis=0)
    got = ctx.percentile_axis0(x, q)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_percentile_axis0_on_device_tensors_and_3d(ctx):
    torch = pytest.importorskip("torch")
    rs = np.random.RandomState(0)
    x = rs.beta(0.5, 0.5, size=(120, 16, 10))  # (replicates, K, S) like the proportions stack
    want = np.percentile(x, [2.5, 97.5], axis=0)
    assert np.array_equal(ctx.percentile_axis0(x, [2.5, 97.5]), want)
    xt = torch.from_numpy(x).to("cuda:0")
    got = ctx.percentile_axis0(xt, [2.5, 97.5])
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)


def test_percentile_axis0_rejects_bad_input(ctx):
    from demethify_amd._lib import DemethifyHipError

    x = np.zeros((4, 4))
    with pytest.raises(DemethifyHipError):
        ctx.percentile_axis0(x, [101.0])
    with pytest.raises(DemethifyHipError):
        ctx.percentile_axis0(np.zeros((20000, 2)), [50.0])  # more replicates than the ranking tile holds
