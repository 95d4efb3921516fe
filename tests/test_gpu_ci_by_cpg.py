"""Profile intervals by CpG on the device: Solver.copy_u_by_cpg and Context.nanpercentile_axis0
against the numpy model of tests/ci_by_cpg_model.py, bt_ci(profile_rows="cpg") end to end on the committed 350 x 10 data,
and the command line.  Every comparison is exact: the copy moves bits, the percentile arithmetic repeats numpy's."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import ci_by_cpg_model as model

from conftest import ROOT, UPSTREAM, load_toy

SENTINEL = -7.25
ITER1, ITER2, TOL, SEED, LEVEL, B = 30, 20, 1e-2, 1, 90, 12  # (tol and seed: the command line's defaults)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def ci_percentiles(level):
    a = 1 - level / 100  # bootstrap.py:20-22, as written there
    return [100 * (a / 2), 100 * (1 - (a / 2))]


# ------------------------------------------------------------------------------------------------ 1. the copy
# (source rows = len(idx), destination rows): one row, around one workgroup of 256, several workgroups, mostly absent
# CpGs, every CpG drawn many times
COPY_SHAPES = [(1, 1), (255, 255), (256, 256), (257, 257), (4099, 4099), (100, 4099), (5000, 300)]


def index_cases(N, n_rows, rs):
    cases = {"randint": rs.randint(0, n_rows, size=N), "all_equal": np.full(N, n_rows // 2)}
    if N <= n_rows:
        cases["identity"] = np.arange(N)
        cases["reversed"] = np.arange(N)[::-1].copy()
    return {k: v.astype(np.int64) for k, v in cases.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("n_u", [1, 3, 4, 7])
@pytest.mark.parametrize("N,n_rows", COPY_SHAPES)
def test_copy_u_by_cpg_against_the_model(ctx, N, n_rows, n_u):
    import torch

    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver
    from demethify_amd.staging import indices_to_device

    rs = np.random.RandomState(100 * N + n_u)
    S = 3
    V, D = rs.rand(N, S), rs.randint(1, 40, size=(N, S)).astype(np.int64)
    u0, a0 = rs.rand(N, n_u), rs.dirichlet(np.ones(n_u), S).T

    def filled():
        # (the fill runs on torch's stream, the library writes on its own: let the fill finish first)
        t = torch.full((n_rows, n_u), SENTINEL, dtype=torch.float64, device=f"cuda:{ctx.device}")
        torch.cuda.synchronize()
        return t

    with Problem(ctx, V, D, None) as p, Solver(p, u0, a0, L.DMF_MODE_UNSUPERVISED) as s:  # not stepped: u == u0
        for name, idx in index_cases(N, n_rows, rs).items():
            as_tensor = torch.from_numpy(idx).to(f"cuda:{ctx.device}")
            for columns in (None, rs.permutation(n_u)):
                want = model.rows_by_cpg(u0, idx, n_rows, order=columns)
                out = filled()
                s.copy_u_by_cpg(out, indices_to_device(idx, ctx), n_rows, columns=columns)
                got = out.cpu().numpy()
                # the copied values and the NaN of the rows not drawn, bit for bit; no sentinel is left
                assert np.array_equal(bits(got), bits(want)), (name, columns)
                again = filled()
                s.copy_u_by_cpg(again, as_tensor, n_rows, columns=columns)  # a second call, idx as a CUDA tensor
                assert np.array_equal(bits(again.cpu().numpy()), bits(got)), (name, columns)
        # an index outside the destination's rows: refused, nothing written
        for where, value in ((0, -1), (N - 1, n_rows), (N // 2, 1 << 40)):
            bad = rs.randint(0, n_rows, size=N).astype(np.int64)
            bad[where] = value
            out = filled()
            with pytest.raises(L.DemethifyHipError) as e:
                s.copy_u_by_cpg(out, indices_to_device(bad, ctx), n_rows)
            assert e.value.status == L.DMF_ERR_BAD_ARG
            assert (out.cpu().numpy() == SENTINEL).all(), (where, value)
        # the wrapper's own refusals
        good = indices_to_device(np.zeros(N, dtype=np.int64), ctx)
        with pytest.raises(ValueError):
            s.copy_u_by_cpg(filled().reshape(-1)[:-1], good, n_rows)  # one element short
        with pytest.raises(ValueError):
            s.copy_u_by_cpg(filled(), np.zeros(N, dtype=np.int64), n_rows)  # a host index array
        with pytest.raises(ValueError):
            s.copy_u_by_cpg(filled(), indices_to_device(np.zeros(N + 1, dtype=np.int64), ctx), n_rows)
        with pytest.raises(ValueError):
            s.copy_u_by_cpg(filled(), good, n_rows, columns=[0] * n_u if n_u > 1 else [1])
        # ... and the solver still answers
        out = filled()
        s.copy_u_by_cpg(out, good, n_rows)
        assert np.array_equal(bits(out.cpu().numpy()), bits(model.rows_by_cpg(u0, np.zeros(N, dtype=np.int64), n_rows)))


# ------------------------------------------------------------------------------------------------ 2. the percentiles
Q_SETS = [[2.5, 97.5], [0.0, 100.0], [50.0, 50.0], [10.0, 90.0], [97.5], [2.5, 50.0, 97.5]]


def nan_patterns(n, m, rs):
    """name -> (n, m) stack.  `special`: a column without a number, a column with one number, a column of ties, among
    columns with 37 % NaN (with one column only, each of the three on its own)."""
    base = rs.rand(n, m)
    out = {"none": base.copy()}
    p37 = base.copy()
    p37[rs.rand(n, m) < 0.37] = np.nan
    out["p37"] = p37
    if n == 1300:
        p95 = base.copy()
        p95[rs.rand(n, m) < 0.95] = np.nan  # few numbers under a large n
        out["p95"] = p95

    def all_nan(x, c):
        x[:, c] = np.nan

    def one_value(x, c):
        x[:, c] = np.nan
        x[(3 * n) // 4, c] = 0.625

    def ties(x, c):
        x[:, c] = np.round(x[:, c], 1)

    if m >= 3:
        x = p37.copy()
        all_nan(x, 0), one_value(x, m // 2), ties(x, m - 1)
        out["special"] = x
    else:
        for name, fn in (("all_nan", all_nan), ("one_value", one_value), ("ties", ties)):
            x = p37.copy()
            fn(x, 0)
            out[name] = x
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 255, 257, 1000])
@pytest.mark.parametrize("n", [1, 2, 7, 40, 200, 1300])
def test_nanpercentile_axis0_against_numpy(ctx, n, m):
    import torch

    rs = np.random.RandomState(7 * n + m)
    for name, x in nan_patterns(n, m, rs).items():
        on_device = torch.from_numpy(x).to(f"cuda:{ctx.device}")
        for q in Q_SETS:
            want = model.bounds(x, q)
            got = ctx.nanpercentile_axis0(x, q)
            assert got.shape == (len(q), m)
            assert np.array_equal(got, want, equal_nan=True), (name, q, np.flatnonzero((bits(got) != bits(want)).any(axis=0))[:8])
            got_t = ctx.nanpercentile_axis0(on_device, q)
            assert got_t.is_cuda and np.array_equal(bits(got_t.cpu().numpy()), bits(got)), (name, q)
            if name == "none":  # without NaNs: the bits of percentile_axis0
                assert np.array_equal(bits(got), bits(ctx.percentile_axis0(x, q))), q
    # a stack of more dimensions keeps its trailing shape
    if m == 1000:
        x = nan_patterns(n, m, rs)["p37"]
        got = ctx.nanpercentile_axis0(x.reshape(n, 250, 4), [2.5, 97.5])
        assert np.array_equal(got, model.bounds(x, [2.5, 97.5]).reshape(2, 250, 4), equal_nan=True)


# ------------------------------------------------------------------------------------------------ 3. end to end
def run_bt_ci(outdir, n_u, with_ref, n_bootstrap, **kw):
    """bt_ci on the committed 350 x 10 data -> (results, what _observe saw per replicate, sample names)."""
    from demethify_amd.bootstrap import bt_ci

    V, D, ref, header = load_toy()
    seen = {}

    def observe(i, seed_i, idx, s):
        perm = None if s.component_perm is None else np.array(s.component_perm)
        seen[i] = (np.array(idx), s.get()[0], perm)

    samples = [f"sample{k + 1}.bed" for k in range(V.shape[1])]
    outdir.mkdir()
    res = bt_ci(LEVEL, n_bootstrap, n_u, V, D, ref if with_ref else None, "uniform_", ITER1, ITER2, TOL,
                header if with_ref else [], str(outdir), samples, None, SEED, materialize=False, _observe=observe, **kw)
    return res, seen


def model_bounds(seen, n_rows):
    stack = np.stack([model.rows_by_cpg(u, idx, n_rows, order=None if perm is None else np.argsort(perm))
                      for _, (idx, u, perm) in sorted(seen.items())])
    lo, hi = model.bounds(stack, ci_percentiles(LEVEL))
    return stack, lo, hi


def parse_interval_csv(path, n_u):
    prof = pd.read_csv(path)
    assert list(prof.columns) == [f"unknown_cell_{k + 1}" for k in range(n_u)]
    cells = np.array([[eval(cell, {"np": np, "nan": np.nan}) for cell in prof[col]] for col in prof.columns])  # (n_u, N, 2)
    return cells[:, :, 0].T, cells[:, :, 1].T


@pytest.fixture(scope="module")
def partial_run(tmp_path_factory):
    """The run the command line is compared with: partial reference, one unknown type, 12 replicates."""
    out = tmp_path_factory.mktemp("by_cpg") / "partial"
    res, seen = run_bt_ci(out, 1, True, B, profile_rows="cpg")
    return out, res, seen


def check_by_cpg(out, res, seen, n_u, n_bootstrap):
    assert sorted(seen) == list(range(n_bootstrap))
    stack, lo, hi = model_bounds(seen, 350)
    lower, upper = res[1]
    assert lower.shape == upper.shape == (350, n_u)
    assert np.array_equal(lower, lo, equal_nan=True) and np.array_equal(upper, hi, equal_nan=True)
    csv_lo, csv_hi = parse_interval_csv(out / "confidence_interval_methylation_estimate.csv", n_u)
    assert np.array_equal(csv_lo, lo, equal_nan=True) and np.array_equal(csv_hi, hi, equal_nan=True)
    return stack, lo, hi


@pytest.mark.gpu
def test_bt_ci_by_cpg_with_a_reference(partial_run):
    out, res, seen = partial_run
    assert all(perm is None for _, _, perm in seen.values())
    stack, lo, hi = check_by_cpg(out, res, seen, 1, B)
    present = (~np.isnan(stack[:, :, 0])).sum(axis=0)
    print("CpGs by the number of replicates that drew them: min", present.min(), "mean", present.mean())
    assert 0.5 < present.mean() / B < 0.75  # about 63 % of the replicates draw a CpG
    assert not np.array_equal(lo, hi, equal_nan=True)


@pytest.mark.gpu
def test_bt_ci_by_cpg_without_a_reference_aligned(tmp_path):
    res, seen = run_bt_ci(tmp_path / "out", 2, False, B, profile_rows="cpg")
    assert all(perm is not None and sorted(perm.tolist()) == [0, 1] for _, _, perm in seen.values())
    check_by_cpg(tmp_path / "out", res, seen, 2, B)


@pytest.mark.gpu
def test_two_replicates_leave_cpgs_without_an_interval(tmp_path):
    from demethify_amd.bootstrap import bootstrap_row_indices, bootstrap_seed_sequence

    drawn = np.zeros(350, dtype=bool)
    for seed in bootstrap_seed_sequence(SEED, 2):
        drawn[bootstrap_row_indices(seed, 350)] = True
    assert 20 <= (~drawn).sum() <= 80, (~drawn).sum()  # about 47 of 350 are expected in neither replicate
    res, seen = run_bt_ci(tmp_path / "out", 1, True, 2, profile_rows="cpg")
    _, lo, hi = check_by_cpg(tmp_path / "out", res, seen, 1, 2)
    assert np.array_equal(np.isnan(lo[:, 0]), ~drawn) and np.array_equal(np.isnan(hi[:, 0]), ~drawn)
    got = (tmp_path / "out" / "confidence_interval_methylation_estimate.csv").read_bytes()
    assert got == model.interval_csv_bytes(["unknown_cell_1"], lo, hi)


@pytest.mark.gpu
def test_position_is_the_default(tmp_path):
    res_a, _ = run_bt_ci(tmp_path / "a", 1, True, 4)
    res_b, _ = run_bt_ci(tmp_path / "b", 1, True, 4, profile_rows="position")
    for x, y in zip(res_a[1], res_b[1]):
        assert np.array_equal(x, y) and not np.isnan(x).any()
    for f in ("confidence_interval_methylation_estimate.csv", "confidence_interval_celltypes_proportions.csv"):
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes()


# ------------------------------------------------------------------------------------------------ 4. command line
@pytest.mark.gpu
def test_command_line_by_cpg(tmp_path, partial_run):
    out, _, _ = partial_run
    samples = [str(UPSTREAM / "output_gen" / f"sample{i}.bed") for i in range(1, 11)]
    argv = ["--ref", str(UPSTREAM / "output_gen" / "ref_matrix.bed"), "--methfreq", *samples, "--bedmethyl", "--nbunknown", "1",
            "--confidence", str(LEVEL), str(B), "--iterations", str(ITER1), str(ITER2), "--noprint", "--outdir",
            str(tmp_path / "cli")]
    proc = subprocess.run([sys.executable, "-m", "demethify_amd", *argv], cwd=ROOT, capture_output=True, text=True,
                          env=dict(os.environ, DEMETHIFY_CI_ROWS="cpg"))
    assert proc.returncode == 0, proc.stderr[-2000:]
    for f in ("confidence_interval_methylation_estimate.csv", "confidence_interval_celltypes_proportions.csv"):
        assert (tmp_path / "cli" / f).read_bytes() == (out / f).read_bytes(), f
