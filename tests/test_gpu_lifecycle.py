"""Handle lifecycle on one context, the way a bootstrap uses it: problems and solvers are created, solved and closed over
and over, so every large buffer of a round is a block that an earlier round gave back to the context's pool.  Which block
a buffer gets depends on the order of release; the results must not."""
import numpy as np
import pytest

from oracle import solver as osol

pytestmark = pytest.mark.gpu
TIGHT = 1e-8
N, S, N_C, N_U = 4100, 40, 3, 2  # a ragged 16-row tail; V is 1.3 MB: above the 1 MB threshold of the kept blocks
T1, T2 = 3, 20


def _solve(problem, u0, a0, full=None):
    from demethify_amd.device import Solver

    with Solver(problem, u0, a0) as s:
        s.step(T1, T2, 0.0)
        u, alpha, cost, _ = s.get()
        held_out = s.holdout_error(full) if full is not None else None
    return u, alpha, cost, held_out


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]


def test_reused_blocks_do_not_change_results(ctx):
    from demethify_amd._lib import DemethifyHipError
    from demethify_amd.device import Problem, Solver

    V, D, Rt = osol.synthetic_problem(N, S, N_C, N_U, seed=11, depth=12)
    u0, R, a0 = osol.init_partial("uniform_", V, D, Rt, N_U, seed=1)
    wu, wa = osol.solve_partial(u0.copy(), R, a0.copy(), V, D, Rt, N_U, T1, T2, 0.0,
                                project=osol.simplex_project_columns_fast)

    def plain_round():
        with Problem(ctx, V, D, Rt) as p:
            return _solve(p, u0, a0)

    rounds = [plain_round() for _ in range(3)]
    assert _same(rounds[0], rounds[1]) and _same(rounds[0], rounds[2])
    assert np.abs(rounds[0][1] - wa).max() < TIGHT and np.abs(rounds[0][0] - wu).max() < TIGHT
    assert np.isfinite(rounds[0][2])

    rs = np.random.RandomState(5)
    idx = rs.randint(0, N, size=N)
    mask = rs.rand(N, S) >= 0.25
    with Problem(ctx, V, D, Rt) as full:
        def gather_round():
            with full.gather(idx) as g:
                return _solve(g, u0, a0)

        def mask_round():
            with full.masked(mask) as m:
                return _solve(m, u0, a0, full=full)

        gathered = [gather_round() for _ in range(2)]
        masked = [mask_round() for _ in range(2)]
    assert _same(gathered[0], gathered[1])
    assert _same(masked[0], masked[1])
    assert masked[0][3][1] == int((~mask).sum())

    # a solver that is refused (K = 65 > 64) leaves the context as it was
    Vw, Dw, Rtw = osol.synthetic_problem(300, 6, 60, 4, seed=8, depth=12)
    with Problem(ctx, Vw, Dw, Rtw) as pw:
        with pytest.raises(DemethifyHipError) as err:
            Solver(pw, rs.uniform(size=(300, 5)), rs.dirichlet(np.ones(65), 6).T)
        assert err.value.status == 5  # DMF_ERR_UNSUPPORTED
        again = plain_round()
    assert _same(rounds[0], again)
