"""Bootstrap intervals without a reference, unknown components aligned: k_match_gram and
k_copy_cols_permuted against numpy, bt_ci without a reference and with ``align_unknown`` against a pipeline built here from
the oracle's solver, and the command line.  The oracle pipelines are computed once per shape and shared."""
import ctypes as C
import functools
import itertools
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
from scipy.optimize import linear_sum_assignment

from oracle import drivers as odrv
from oracle import solver as osol

from conftest import ROOT

EPS = np.finfo(np.float64).eps
ITER1, ITER2, SEED = 25, 20, 1
# the bound tests/test_cli.py::test_confidence_intervals_match_oracle_bootstrap holds the partial path to
CI_ATOL = 1e-8
MIN_MARGIN = 1e-2

# (N, n_u): the issue's shapes -- one row, a ragged tile, several tiles of several workgroups, pairs in two row groups
# (n_u = 9), 256 pairs exactly (16), 16 accumulators per thread (33, 64) -- and two more for paths they leave out: 4
# accumulators per thread (17 <= n_u <= 32) and more tiles than workgroups (N > 256 * (2048 // n_u))
MATCH_SHAPES = [(1, 1), (63, 2), (1000, 3), (4097, 4), (2048, 9), (777, 16), (515, 33), (300, 64), (130, 24), (9000, 64)]


# ------------------------------------------------------------------------------------------------ the oracle side
def _oracle_solve(V, D, Rt, n_u, seed):
    if Rt is None:
        return osol.solve_unsupervised(V, n_u, D, "uniform_", n_iter1=ITER1, n_iter2=ITER2, tol=0.0, seed=seed)
    u, R, alpha = osol.init_partial("uniform_", V, D, Rt, n_u, seed=seed)
    return osol.solve_partial(u, R, alpha, V, D, Rt, n_u, ITER1, ITER2, 0.0)


def _assign(P):
    """(perm, margin): perm[a] = the anchor component of replicate component a, by scipy; the margin (best - second best)
    / best over ALL assignments by brute force (n_u <= 4 here)."""
    rows, cols = linear_sum_assignment(P, maximize=True)
    perm = np.empty(len(rows), dtype=np.int64)
    perm[rows] = cols
    n = P.shape[0]
    scores = sorted((sum(P[a, p[a]] for a in range(n)) for p in itertools.permutations(range(n))), reverse=True)
    assert abs(scores[0] - sum(P[a, perm[a]] for a in range(n))) <= 1e-12 * scores[0]
    return perm, (scores[0] - scores[1]) / scores[0]


def oracle_pipeline(V, D, Rt, n_u, B, anchor=None):
    """Replicates solved by the oracle, aligned to the anchor (the oracle's solve of the full data with SEED unless one is
    given) -> dict(us (B, N, n_u), alphas (B, K, S), perms, margins), us / alphas in the anchor's component order."""
    n_c = 0 if Rt is None else Rt.shape[1]
    if anchor is None:
        anchor = _oracle_solve(V, D, Rt, n_u, SEED)
    anchor_u = np.asarray(anchor[0]).reshape(V.shape[0], n_u)
    us, alphas, perms, margins = [], [], [], []
    for s in osol.bootstrap_seeds(SEED, B):
        idx = osol.bootstrap_indices(s, V.shape[0])
        u, alpha = _oracle_solve(V[idx], D[idx], None if Rt is None else Rt[idx], n_u, s)
        perm, margin = _assign(u.T @ anchor_u[idx])
        order = np.argsort(perm)
        alpha = alpha.copy()
        alpha[n_c:] = alpha[n_c:][order]
        us.append(u[:, order])
        alphas.append(alpha)
        perms.append(perm)
        margins.append(margin)
    return {"us": np.stack(us), "alphas": np.stack(alphas), "perms": perms, "margins": margins}


@functools.lru_cache(maxsize=None)
def problem_and_pipeline(N, S, n_c, n_u, B):
    V, D, Rt = osol.synthetic_problem(N, S, n_c, n_u)  # (data seed 0: the shapes DESIGN.md section 6 tabulates)
    Rt = Rt if n_c else None
    return V, D, Rt, oracle_pipeline(V, D, Rt, n_u, B)


def check_oracle_side(pipe):
    """What makes the comparison meaningful: no replicate's assignment is a near tie, and the replicates do come out in
    different orders (a missing or wrong alignment then cannot pass)."""
    assert min(pipe["margins"]) >= MIN_MARGIN, pipe["margins"]
    n_u = len(pipe["perms"][0])
    assert sum(p.tolist() != list(range(n_u)) for p in pipe["perms"]) >= 2, pipe["perms"]


def parse_cells(column):
    return np.array([eval(cell, {"np": np}) for cell in column])  # "(lo, hi)" tuples, as upstream writes them


def check_csvs(outdir, rows, samples, n_u, alphas, us):
    lo, hi = odrv.percentile_bounds(alphas, 90)
    table = pd.read_csv(outdir / "confidence_interval_celltypes_proportions.csv", index_col=0)
    assert table.index.name == "Cell Type" and list(table.index) == rows and list(table.columns) == samples
    for s_i, col in enumerate(table.columns):
        cells = parse_cells(table[col])
        print("proportions", col, np.abs(cells[:, 0] - lo[:, s_i]).max(), np.abs(cells[:, 1] - hi[:, s_i]).max())
        assert np.abs(cells[:, 0] - lo[:, s_i]).max() < CI_ATOL and np.abs(cells[:, 1] - hi[:, s_i]).max() < CI_ATOL
    lo_u, hi_u = odrv.percentile_bounds(us, 90)
    prof = pd.read_csv(outdir / "confidence_interval_methylation_estimate.csv")
    assert list(prof.columns) == [f"unknown_cell_{k + 1}" for k in range(n_u)] and len(prof) == us.shape[1]
    for k, col in enumerate(prof.columns):
        cells = parse_cells(prof[col])
        print("profiles", col, np.abs(cells[:, 0] - lo_u[:, k]).max(), np.abs(cells[:, 1] - hi_u[:, k]).max())
        assert np.abs(cells[:, 0] - lo_u[:, k]).max() < CI_ATOL and np.abs(cells[:, 1] - hi_u[:, k]).max() < CI_ATOL


# ------------------------------------------------------------------------------------------------ kernels
@functools.lru_cache(maxsize=None)
def match_inputs(N, n_u):
    rs = np.random.RandomState(1000 * n_u + N % 997)
    S, M = 3, N + 37
    V, D = rs.rand(N, S), rs.randint(1, 40, size=(N, S)).astype(np.int64)
    u0 = rs.rand(N, n_u)
    a0 = rs.dirichlet(np.ones(n_u), S).T
    anchor_same, anchor_other = rs.rand(N, n_u), rs.rand(M, n_u)
    idx = rs.randint(0, M, size=N)
    if N > 2:
        idx[1] = idx[0]  # (a repeat for sure)
    for a in (V, D, u0, a0, anchor_same, anchor_other, idx):
        a.setflags(write=False)
    return V, D, u0, a0, anchor_same, anchor_other, idx


def _solver(ctx, N, n_u):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    V, D, u0, a0 = match_inputs(N, n_u)[:4]
    p = Problem(ctx, V, D, None)
    return p, Solver(p, u0, a0, L.DMF_MODE_UNSUPERVISED)


@pytest.mark.gpu
@pytest.mark.parametrize("N,n_u", MATCH_SHAPES)
def test_match_gram_against_numpy(ctx, N, n_u):
    import torch

    from demethify_amd.staging import indices_to_device, to_device

    _, _, u0, _, anchor_same, anchor_other, idx = match_inputs(N, n_u)
    p, s = _solver(ctx, N, n_u)
    with p, s:
        cases = [("identity", to_device((anchor_same,), ctx)[0], None, u0.T @ anchor_same),
                 ("gathered", to_device((anchor_other,), ctx)[0], indices_to_device(idx, ctx), u0.T @ anchor_other[idx]),
                 ("tensors", torch.from_numpy(anchor_other.copy()).to(f"cuda:{ctx.device}"),
                  torch.from_numpy(idx.astype(np.int64)).to(f"cuda:{ctx.device}"), u0.T @ anchor_other[idx])]
        for name, anchor_dev, idx_dev, want in cases:
            P = s.match_components(anchor_dev, idx_dev)
            # all terms are non-negative: any summation order is within N eps relative, numpy's included
            excess = (np.abs(P - want) / (2 * N * EPS * want)).max()
            print(name, (N, n_u), "largest |P - ref| / (2 N eps P) =", excess)
            assert P.shape == (n_u, n_u) and excess <= 1.0, (name, excess)
            assert np.array_equal(P, s.match_components(anchor_dev, idx_dev)), name  # the same bits twice
        assert np.array_equal(s.match_components(cases[1][1], cases[1][2]), s.match_components(cases[2][1], cases[2][2]))
        with pytest.raises(ValueError):
            s.match_components(anchor_other)  # a host array
        if n_u > 1:
            with pytest.raises(ValueError):
                s.match_components(to_device((anchor_other.ravel()[:n_u * 5 + 1],), ctx)[0])  # not rows of n_u


@pytest.mark.gpu
@pytest.mark.parametrize("N,n_u,where,value", [(1000, 3, 0, -1), (1000, 3, 999, 1037), (4097, 4, 2500, 1 << 40),
                                                (515, 33, 514, 552), (63, 2, 7, -(1 << 62))])
def test_match_gram_refuses_an_index_outside_the_anchor(ctx, N, n_u, where, value):
    from demethify_amd import _lib as L
    from demethify_amd.device import _ptr
    from demethify_amd.staging import indices_to_device, to_device

    _, _, _, _, anchor_same, anchor_other, idx = match_inputs(N, n_u)
    bad = idx.copy()
    bad[where] = value
    p, s = _solver(ctx, N, n_u)
    with p, s:
        anchor_dev, = to_device((anchor_other,), ctx)
        bad_dev = indices_to_device(bad, ctx)
        with pytest.raises(L.DemethifyHipError) as e:
            s.match_components(anchor_dev, bad_dev)
        assert e.value.status == L.DMF_ERR_BAD_ARG
        sentinel = np.full((n_u, n_u), -7.25)
        out = sentinel.copy()
        rc = s._lib.dmf_solver_match_components(s._h, _ptr(anchor_dev), anchor_other.shape[0], _ptr(bad_dev), _ptr(out))
        assert rc == L.DMF_ERR_BAD_ARG and np.array_equal(out, sentinel)  # out_P untouched
        # the identity needs an anchor of the problem's N rows; null pointers
        rc = s._lib.dmf_solver_match_components(s._h, _ptr(anchor_dev), anchor_other.shape[0], None, _ptr(out))
        assert rc == L.DMF_ERR_BAD_SHAPE and np.array_equal(out, sentinel)
        assert s._lib.dmf_solver_match_components(s._h, None, N, None, _ptr(out)) == L.DMF_ERR_BAD_ARG
        assert s._lib.dmf_solver_match_components(s._h, _ptr(anchor_dev), N, None, None) == L.DMF_ERR_BAD_ARG
        # ... and the solver still answers
        good = s.match_components(anchor_dev, indices_to_device(idx, ctx))
        assert np.all(np.isfinite(good))


@pytest.mark.gpu
@pytest.mark.parametrize("N,n_u", MATCH_SHAPES)
def test_copy_u_to_with_columns(ctx, N, n_u):
    import torch

    from demethify_amd import _lib as L
    from demethify_amd.device import _ptr

    u0 = match_inputs(N, n_u)[2]
    rs = np.random.RandomState(N + n_u)
    p, s = _solver(ctx, N, n_u)
    with p, s:
        def filled(*shape):
            # (the fill runs on torch's stream, the library writes on its own: let the fill finish first)
            t = torch.full(shape, -1.0, dtype=torch.float64, device=f"cuda:{ctx.device}")
            torch.cuda.synchronize()
            return t

        plain = filled(N * n_u)
        s.copy_u_to(plain)
        assert np.array_equal(plain.cpu().numpy().reshape(N, n_u), u0)  # columns=None: today's copy
        for columns in (np.arange(n_u), np.arange(n_u)[::-1], rs.permutation(n_u), rs.permutation(n_u).tolist()):
            out = filled(N, n_u)
            s.copy_u_to(out, columns=columns)
            assert np.array_equal(out.cpu().numpy(), u0[:, np.asarray(columns)]), columns
        out = filled(N, n_u)
        wrong = [[0] * n_u, list(range(1, n_u + 1)), list(range(n_u)) + [0], [-1] + list(range(1, n_u))]
        for columns in wrong[(1 if n_u == 1 else 0):]:
            with pytest.raises(ValueError):
                s.copy_u_to(out, columns=columns)
            if len(columns) == n_u:  # the library's own refusal, below the wrapper's
                cols = np.ascontiguousarray(columns, dtype=np.int32)
                rc = s._lib.dmf_solver_get_u_permuted(s._h, cols.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(out))
                assert rc == L.DMF_ERR_BAD_ARG
        assert (out.cpu().numpy() == -1.0).all()  # nothing was written by a refused call
        ident = np.arange(n_u, dtype=np.int32)
        assert s._lib.dmf_solver_get_u_permuted(s._h, ident.ctypes.data_as(C.POINTER(C.c_int32)), None) == L.DMF_ERR_BAD_ARG
        assert s._lib.dmf_solver_get_u_permuted(s._h, None, _ptr(out)) == L.DMF_ERR_BAD_ARG


# ------------------------------------------------------------------------------------------------ end to end
def _run_bt_ci(tmp_path, V, D, Rt, n_u, B, header, **kw):
    from demethify_amd.bootstrap import bt_ci

    seen = {}

    def observe(i, seed_i, idx, s):
        seen[i] = (seed_i, None if s.component_perm is None else np.array(s.component_perm))

    samples = [f"s{k}" for k in range(V.shape[1])]
    res = bt_ci(90, B, n_u, V, D, Rt, "uniform_", ITER1, ITER2, 0.0, header, str(tmp_path), samples, None, SEED,
                _observe=observe, **kw)
    return res, seen, samples


@pytest.mark.gpu
@pytest.mark.parametrize("N,S,n_u,B", [(600, 12, 3, 6), (1024, 20, 4, 6)])
def test_no_reference_bootstrap_matches_the_aligned_oracle_pipeline(tmp_path, N, S, n_u, B):
    V, D, _, pipe = problem_and_pipeline(N, S, 0, n_u, B)
    print("margins", pipe["margins"], "assignments", [p.tolist() for p in pipe["perms"]])
    check_oracle_side(pipe)
    res, seen, samples = _run_bt_ci(tmp_path, V, D, None, n_u, B, [])
    assert sorted(seen) == list(range(B))
    for i, want_seed in enumerate(osol.bootstrap_seeds(SEED, B)):
        assert seen[i][0] == want_seed
        assert seen[i][1].tolist() == pipe["perms"][i].tolist(), (i, seen[i][1], pipe["perms"][i])
    rows = [f"unknown_cell_{k + 1}" for k in range(n_u)]
    check_csvs(tmp_path, rows, samples, n_u, pipe["alphas"], pipe["us"])
    assert list(res[0].index) == rows and len(res) == 2


@pytest.mark.gpu
def test_opt_in_alignment_with_a_reference(tmp_path):
    N, S, n_c, n_u, B = 1024, 20, 3, 2, 5
    V, D, Rt, pipe = problem_and_pipeline(N, S, n_c, n_u, B)
    print("margins", pipe["margins"], "assignments", [p.tolist() for p in pipe["perms"]])
    assert min(pipe["margins"]) >= MIN_MARGIN
    assert any(p.tolist() != [0, 1] for p in pipe["perms"])
    header = ["a", "b", "c"]
    rows = header + ["unknown_cell_1", "unknown_cell_2"]
    (tmp_path / "aligned").mkdir()
    _, seen, samples = _run_bt_ci(tmp_path / "aligned", V, D, Rt, n_u, B, header, align_unknown=True)
    for i in range(B):
        assert seen[i][1].tolist() == pipe["perms"][i].tolist(), i
    check_csvs(tmp_path / "aligned", rows, samples, n_u, pipe["alphas"], pipe["us"])
    # the default with a reference stays upstream's: replicates as they come
    (tmp_path / "default").mkdir()
    _, seen, samples = _run_bt_ci(tmp_path / "default", V, D, Rt, n_u, B, header)
    assert all(perm is None for _, perm in seen.values())
    us, alphas = odrv.bootstrap_replicates(B, n_u, V, D, Rt, "uniform_", ITER1, ITER2, 0.0, SEED)
    check_csvs(tmp_path / "default", rows, samples, n_u, alphas, us)


# ------------------------------------------------------------------------------------------------ command line
def run_cli(*argv, expect=0):
    proc = subprocess.run([sys.executable, "-m", "demethify_amd", *argv], cwd=ROOT, capture_output=True, text=True)
    assert proc.returncode == expect, proc.stderr[-2000:]
    return proc


@pytest.mark.gpu
def test_command_line_without_a_reference(tmp_path):
    N, S, n_u, B = 600, 12, 3, 6
    V, D, _, _ = problem_and_pipeline(N, S, 0, n_u, B)
    names = []
    for k in range(S):
        names.append(f"sample{k + 1}.csv")
        pd.DataFrame({"valid_coverage": D[:, k], "percent_modified": V[:, k]}).to_csv(tmp_path / names[-1], index=False)
    # (the values as the command reads them back from the text)
    V_read = np.column_stack([pd.read_csv(tmp_path / n)["percent_modified"].values for n in names])
    files = [str(tmp_path / n) for n in names]
    common = ["--methfreq", *files, "--iterations", str(ITER1), str(ITER2), "--termination", "0", "--noprint"]
    out = tmp_path / "out"
    run_cli(*common, "--nbunknown", str(n_u), "--confidence", "90", str(B), "--outdir", str(out))
    rows = [f"unknown_cell_{k + 1}" for k in range(n_u)]
    point = pd.read_csv(out / "celltypes_proportions.csv", index_col=0)
    assert list(point.index) == rows
    anchor_u = pd.read_csv(out / "methylation_profile_estimate.csv").values
    want_u, want_alpha = _oracle_solve(V_read, D, None, n_u, SEED)
    assert np.abs(anchor_u - want_u).max() < CI_ATOL and np.abs(point.values - want_alpha).max() < CI_ATOL
    # the oracle pipeline whose anchor is the command's own point estimate
    pipe = oracle_pipeline(V_read, D, None, n_u, B, anchor=(anchor_u, point.values))
    check_oracle_side(pipe)
    check_csvs(out, rows, names, n_u, pipe["alphas"], pipe["us"])

    p = run_cli(*common, "--nbunknown", "0", "--confidence", "90", str(B), "--outdir", str(tmp_path / "none"), expect=1)
    assert "Invalid number of unknown value" in p.stderr
    assert not (tmp_path / "none" / "confidence_interval_celltypes_proportions.csv").exists()

    # two ranks sharing the GPU (gloo): every rank matches against the same anchor, the files are the same bytes
    from test_cli import run_cli_ranks

    out2 = tmp_path / "out2"
    run_cli_ranks(2, *common, "--nbunknown", str(n_u), "--confidence", "90", str(B), "--outdir", str(out2))
    for f in ("celltypes_proportions.csv", "methylation_profile_estimate.csv",
              "confidence_interval_celltypes_proportions.csv", "confidence_interval_methylation_estimate.csv"):
        assert (out / f).read_text() == (out2 / f).read_text(), f
