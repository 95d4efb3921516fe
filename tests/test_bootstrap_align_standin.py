"""bt_ci's own logic -- no-reference replicates, the anchor, the assignment and where it is applied, the tables -- on a
stand-in device built from the oracle's solver: Problem / Solver / staging are replaced by numpy objects with the same
methods, so the driver runs end to end without a GPU and is compared with the pipeline of tests/test_gpu_bootstrap_align.py
(which runs the same comparison on the real kernels).  No GPU."""
import numpy as np
import pytest

from oracle import solver as osol

import test_gpu_bootstrap_align as ref_side


class _Ctx:
    device = 0

    @staticmethod
    def percentile_axis0(x, q):
        return np.percentile(x, q, axis=0)


class _Problem:
    def __init__(self, ctx, V, D, Rt=None):
        self.ctx, self.V, self.D, self.Rt = ctx, np.asarray(V), np.asarray(D), Rt
        self.N, self.S = self.V.shape
        self.n_c = 0 if Rt is None else Rt.shape[1]

    def gather(self, idx):
        return _Problem(self.ctx, self.V[idx], self.D[idx], None if self.Rt is None else self.Rt[idx])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass


class _Solver:
    def __init__(self, problem, u0, a0, mode):
        self.p, self.u, self.alpha, self.mode = problem, np.array(u0), np.array(a0), mode
        self.n_u = self.u.shape[1]

    def step(self, n1, n2, tol):
        p = self.p
        if p.Rt is None:
            self.u, self.alpha = osol.solve_unsupervised(p.V, self.n_u, p.D, None, n1, n2, tol, init=(self.u, self.alpha))
        else:
            self.u, self.alpha = osol.solve_partial(self.u, np.c_[p.Rt, self.u], self.alpha, p.V, p.D, p.Rt, self.n_u, n1, n2, tol)

    def match_components(self, anchor, idx=None):
        return self.u.T @ (anchor if idx is None else anchor[idx])

    def get(self):
        return self.u.copy(), self.alpha.copy(), 0.0, 0

    def get_alpha(self):
        return self.alpha.copy()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass


@pytest.fixture
def standin(monkeypatch):
    from demethify_amd import _lib as L
    from demethify_amd import bootstrap, staging

    def solve_problem(problem, u0, a0, mode, n1, n2, tol, return_info=False, purity=None):
        s = _Solver(problem, u0, a0, mode)
        s.step(n1, n2, tol)
        return s.u, s.alpha

    monkeypatch.setattr(bootstrap, "get_context", lambda *a: _Ctx)
    monkeypatch.setattr(bootstrap, "Problem", _Problem)
    monkeypatch.setattr(bootstrap, "Solver", _Solver)
    monkeypatch.setattr(bootstrap, "solve_problem", solve_problem)
    monkeypatch.setattr(bootstrap, "_device_stack", lambda *a: None)  # the stack on the host, as without torch
    monkeypatch.setattr(staging, "to_device", lambda arrays, ctx: [np.array(a) for a in arrays])
    monkeypatch.setattr(staging, "indices_to_device", lambda idx, ctx: np.array(idx))
    monkeypatch.setattr(staging, "reserve", lambda *a, **k: None)
    return L


@pytest.mark.parametrize("N,S,n_c,n_u,B", [(600, 12, 0, 3, 6), (1024, 20, 3, 2, 5)])
def test_driver_on_a_standin_device_matches_the_aligned_pipeline(tmp_path, standin, N, S, n_c, n_u, B):
    V, D, Rt, pipe = ref_side.problem_and_pipeline(N, S, n_c, n_u, B)
    if n_c == 0:
        ref_side.check_oracle_side(pipe)
    header = [f"k{k}" for k in range(n_c)]
    res, seen, samples = ref_side._run_bt_ci(tmp_path, V, D, Rt, n_u, B, header, align_unknown=True)
    for i in range(B):
        assert seen[i][1].tolist() == pipe["perms"][i].tolist(), i
    rows = header + [f"unknown_cell_{k + 1}" for k in range(n_u)]
    ref_side.check_csvs(tmp_path, rows, samples, n_u, pipe["alphas"], pipe["us"])
    if n_c == 0:  # the default without a reference is the aligned one
        (tmp_path / "default").mkdir()
        ref_side._run_bt_ci(tmp_path / "default", V, D, None, n_u, B, [])
        for f in ("confidence_interval_celltypes_proportions.csv", "confidence_interval_methylation_estimate.csv"):
            assert (tmp_path / f).read_text() == (tmp_path / "default" / f).read_text()


def test_a_given_anchor_names_the_components(tmp_path, standin):
    """anchor=(u, alpha) with its columns swapped swaps the rows of both tables, and nothing else."""
    N, S, n_u, B = 600, 12, 3, 6
    V, D, _, _ = ref_side.problem_and_pipeline(N, S, 0, n_u, B)
    u, alpha = ref_side._oracle_solve(V, D, None, n_u, ref_side.SEED)
    swap = [2, 0, 1]
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    _, seen_a, samples = ref_side._run_bt_ci(tmp_path / "a", V, D, None, n_u, B, [], anchor=(u, alpha))
    _, seen_b, _ = ref_side._run_bt_ci(tmp_path / "b", V, D, None, n_u, B, [], anchor=(u[:, swap], alpha[swap]))
    inv = np.argsort(swap)
    for i in range(B):
        assert seen_b[i][1].tolist() == inv[seen_a[i][1]].tolist()
    pipe = ref_side.oracle_pipeline(V, D, None, n_u, B, anchor=(u[:, swap], alpha[swap]))
    ref_side.check_csvs(tmp_path / "b", [f"unknown_cell_{k + 1}" for k in range(n_u)], samples, n_u, pipe["alphas"], pipe["us"])
    with pytest.raises(ValueError, match="anchor"):
        ref_side._run_bt_ci(tmp_path / "b", V, D, None, n_u, B, [], anchor=(u[:, :2], alpha[:2]))
