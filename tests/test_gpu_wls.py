"""Reference-based regression on the device: Problem.wls_intercept (k_wls_moments + k_nnls_intercept) against the oracle's
``nnls_intercept_proportions`` sample by sample, and the three callers behind ``init_func.DEVICE_WLS_MIN_ELEMENTS``.

The bound is the project's 1e-10 of the alpha-phase known-answer tests: the Gram form of the regression differs from the
oracle's QR route by 1.5e-14 at most on the CPU, the rest covers the kernels' summation order."""
from __future__ import annotations

import functools

import numpy as np
import pandas as pd
import pytest

from oracle import solver as osol

from conftest import UPSTREAM, read_props

pytestmark = pytest.mark.gpu

TOL = 1e-10
SAMPLES = [str(UPSTREAM / "output_gen" / f"sample{i}.bed") for i in range(1, 11)]
REF = str(UPSTREAM / "output_gen" / "ref_matrix.bed")


def draw_u(N, n_u):
    return np.random.RandomState(9).uniform(size=(N, n_u)) if n_u else None


def oracle_wls(V, D, R_full, target):
    cols = []
    for k in range(V.shape[1]):
        x = D[:, k:k + 1] * V[:, k:k + 1] if target == "dv" else V[:, k:k + 1]
        cols.append(osol.nnls_intercept_proportions(x, D[:, k:k + 1], R_full))
    return np.concatenate(cols, axis=1)


@functools.lru_cache(maxsize=None)
def case(N, S, n_c, n_u, depth=50):
    """(V, D, Rt, u, {target: oracle}) of one synthetic shape, computed once per session and never written to."""
    V, D, Rt = osol.synthetic_problem(N, S, n_c, n_u, depth=depth)
    u = draw_u(N, n_u)
    R_full = np.c_[Rt, u] if n_u else Rt
    want = {t: oracle_wls(V, D, R_full, t) for t in ("v", "dv")}
    for a in (V, D, Rt, R_full) + tuple(want.values()) + ((u,) if n_u else ()):
        a.setflags(write=False)
    return V, D, Rt, u, want


def device_wls(ctx, V, D, Rt, u, target, **kw):
    from demethify_amd.device import Problem

    with Problem(ctx, V, D, Rt) as p:
        got = p.wls_intercept(u, target, **kw)
        return got, p.wls_status


def check(ctx, V, D, Rt, u, target, want):
    got, status = device_wls(ctx, V, D, Rt, u, target)
    err = float(np.abs(got - want).max())
    print(f"wls {V.shape} K={want.shape[0]} target={target}: max abs diff {err:.3e}, status {status.tolist()[:8]}")
    assert (status == 0).all()
    assert err <= TOL
    return got


@pytest.mark.parametrize("target", ["v", "dv"])
@pytest.mark.parametrize("shape", [(4096, 7, 6, 2), (1000, 5, 12, 4), (3000, 9, 25, 0), (777, 4, 3, 1, 5)],
                         ids=lambda s: "x".join(map(str, s)))
def test_basic_shapes(ctx, shape, target):
    V, D, Rt, u, want = case(*shape)
    if shape != (3000, 9, 25, 0):
        # the active-set path is really taken: some column has a coefficient at zero and at least two positive ones
        w = want[target]
        assert (((w == 0).sum(axis=0) >= 1) & ((w > 0).sum(axis=0) >= 2)).any()
    check(ctx, V, D, Rt, u, target, want[target])


def test_single_sample_config1(ctx):
    """S = 1 (no integer count copies: the f64 arrays): the upstream config-1 fixture, first six reference columns."""
    ref = pd.read_csv(UPSTREAM / "config1" / "bed1_select_ref_intersect.bed", sep="\t").iloc[:, 3:9].values.astype(np.float64)
    t = pd.read_csv(UPSTREAM / "config1" / "bed2_intersect.bed", sep="\t")
    V = (t["percent_modified"].values / 100).reshape(-1, 1)
    D = t["valid_coverage"].values.reshape(-1, 1)
    assert V.shape == (393, 1)
    want = oracle_wls(V, D, ref, "dv")
    got = check(ctx, V, D, ref, None, "dv", want)
    assert np.abs(got.ravel() - np.array([0, 0, 0.03548921, 0, 0, 0.96451079])).max() < 5e-9


@pytest.mark.parametrize("shape", [(33, 3, 2, 1), (2048, 65, 6, 2), (2048, 130, 6, 2), (4096, 4, 48, 0), (4096, 4, 60, 4)],
                         ids=lambda s: "x".join(map(str, s)))
def test_edge_shapes(ctx, shape):
    """Fewer rows than one row block, sample counts just past one and two 64-lane blocks, K = 48 and K = 64."""
    V, D, Rt, u, want = case(*shape)
    check(ctx, V, D, Rt, u, "dv", want["dv"])
    if shape[0] == 33:
        check(ctx, V, D, Rt, u, "v", want["v"])


def test_more_than_64_types_is_unsupported(ctx):
    from demethify_amd import _lib as L

    V, D, Rt = osol.synthetic_problem(256, 2, 61, 4)
    with pytest.raises(L.DemethifyHipError) as e:
        device_wls(ctx, V, D, Rt, draw_u(256, 4), "v")
    assert e.value.status == 5  # DMF_ERR_UNSUPPORTED


COUNT_SHAPE = (2048, 8, 6, 2)


def test_counts_with_two_digit_planes(ctx):
    V, D, Rt, u, want = case(*COUNT_SHAPE, 300)
    assert D.max() > 127
    check(ctx, V, D, Rt, u, "dv", want["dv"])


def test_count_beyond_u16_form_takes_f64(ctx):
    V, D, Rt, u, _ = case(*COUNT_SHAPE)
    V, D = V.copy(), D.copy()
    D[5, 2], V[5, 2] = 40000, 12345 / 40000
    check(ctx, V, D, Rt, u, "dv", oracle_wls(V, D, np.c_[Rt, u], "dv"))


def test_x16_on_and_off_agree(ctx):
    V, D, Rt, u, want = case(*COUNT_SHAPE)
    try:
        ctx.set_x16(False)
        off = check(ctx, V, D, Rt, u, "dv", want["dv"])
    finally:
        ctx.set_x16(True)
    on = check(ctx, V, D, Rt, u, "dv", want["dv"])
    assert np.abs(on - off).max() <= 1e-12


def test_generic_level_one(ctx):
    V, D, Rt, u, want = case(*COUNT_SHAPE)
    try:
        ctx.set_generic(1)
        check(ctx, V, D, Rt, u, "dv", want["dv"])
    finally:
        ctx.set_generic(0)


def test_rows_without_coverage(ctx):
    V, D, Rt, u, _ = case(*COUNT_SHAPE)
    V, D = V.copy(), D.copy()
    hole = np.random.RandomState(4).uniform(size=D.shape) < 0.1
    hole[:, 0] = False
    D[hole], V[hole] = 0, 0.0
    check(ctx, V, D, Rt, u, "dv", oracle_wls(V, D, np.c_[Rt, u], "dv"))


def test_gathered_problem(ctx):
    from demethify_amd.device import Problem
    from demethify_amd.staging import indices_to_device

    V, D, Rt, _, _ = case(3000, 6, 5, 0)
    idx = np.random.RandomState(3).randint(0, 3000, size=3000)
    want = oracle_wls(V[idx], D[idx], Rt[idx], "dv")
    with Problem(ctx, V, D, Rt) as full, full.gather(indices_to_device(idx, ctx)) as resampled:
        got = resampled.wls_intercept(None, "dv")
        assert (resampled.wls_status == 0).all()
    assert np.abs(got - want).max() <= TOL


def test_rank_deficient_profiles_go_to_the_host(ctx):
    from demethify_amd.init_func import wls_intercept

    V, D, Rt, _, _ = case(1000, 5, 12, 4)
    Rd = np.ascontiguousarray(np.c_[Rt[:, :4], Rt[:, 1]])
    got, status = device_wls(ctx, V, D, Rd, None, "dv", host_arrays=(V, D, Rd))
    assert (status == 1).all()
    host = np.concatenate([wls_intercept(D[:, k:k + 1] * V[:, k:k + 1], D[:, k:k + 1], Rd) for k in range(V.shape[1])], axis=1)
    assert np.array_equal(got, host)
    with pytest.raises(RuntimeError):
        device_wls(ctx, V, D, Rd, None, "dv")


def test_sample_without_counts_raises(ctx):
    V, D, Rt, _, _ = case(1000, 5, 12, 4)
    V, D = V.copy(), D.copy()
    D[:, 2], V[:, 2] = 0, 0.0
    with pytest.raises(ZeroDivisionError):
        device_wls(ctx, V, D, Rt[:, :4].copy(), None, "dv")


def test_upstream_reference_based_pin(ctx, toy):
    V, D, ref, _ = toy
    got, status = device_wls(ctx, V, D, ref, None, "dv")
    assert (status == 0).all()
    assert np.abs(got - read_props("output_ref_based")).max() <= TOL


# ---- the three callers -----------------------------------------------------------------------------------------------

BASE = ["--ref", REF, "--methfreq", *SAMPLES, "--bedmethyl", "--noprint"]
RUNS = {
    "ref_based": ["--nbunknown", "0"],
    "bootstrap": ["--nbunknown", "0", "--confidence", "95", "6"],
    "uniform_init": ["--init", "uniform", "--nbunknown", "1", "--iterations", "5", "20", "--termination", "0"],
}


def run_main(tmp_path, name, extra):
    from demethify_amd import demethify

    out = tmp_path / name
    demethify.main([*BASE, *extra, "--outdir", str(out)])
    return out


def read_exact(path, **kw):
    """A table as written: pandas' default float parser is off by an ulp now and then."""
    return pd.read_csv(path, float_precision="round_trip", **kw).values


def intervals(path):
    table = pd.read_csv(path, index_col=0)
    return np.array([[eval(cell, {"np": np}) for cell in table[col]] for col in table.columns])


@pytest.fixture
def device_path(monkeypatch):
    """The gate at zero, and a count of the device regressions the run makes."""
    from demethify_amd import init_func
    from demethify_amd.device import Problem

    calls = []
    inner = Problem.wls_intercept

    def counted(self, *a, **kw):
        out = inner(self, *a, **kw)
        assert (self.wls_status == 0).all()
        calls.append(self.wls_status)
        return out

    monkeypatch.setattr(init_func, "DEVICE_WLS_MIN_ELEMENTS", 0)
    monkeypatch.setattr(Problem, "wls_intercept", counted)
    return calls


@pytest.fixture
def host_path(monkeypatch):
    """The gate left alone: a device regression is an error."""
    from demethify_amd.device import Problem

    def refuse(self, *a, **kw):
        raise AssertionError("the host path was expected")

    monkeypatch.setattr(Problem, "wls_intercept", refuse)


def test_cli_reference_based_on_the_device(tmp_path, device_path):
    out = run_main(tmp_path, "ref_based", RUNS["ref_based"])
    got = pd.read_csv(out / "celltypes_proportions.csv", index_col=0).values
    assert len(device_path) == 1
    assert np.abs(got - read_props("output_ref_based")).max() <= TOL


def host_bootstrap_props(toy, n):
    from demethify_amd.bootstrap import bootstrap_row_indices, bootstrap_seed_sequence
    from demethify_amd.init_func import wls_intercept

    V, D, ref, _ = toy
    stack = []
    for seed in bootstrap_seed_sequence(1, n):
        idx = bootstrap_row_indices(seed, V.shape[0])
        mf, ct, rf = V[idx], D[idx], ref[idx]
        stack.append(np.concatenate([wls_intercept(ct[:, k:k + 1] * mf[:, k:k + 1], ct[:, k:k + 1], rf)
                                     for k in range(V.shape[1])], axis=1))
    a = 1 - 95 / 100  # (bootstrap.py:22-24, as coded)
    return np.percentile(np.stack(stack), [100 * (a / 2), 100 * (1 - (a / 2))], axis=0)  # (2, K, S)


def test_cli_supervised_bootstrap_on_the_device(tmp_path, toy, device_path):
    out = run_main(tmp_path, "bootstrap", RUNS["bootstrap"])
    assert len(device_path) == 6 + 1  # six replicates and the point estimate
    got = intervals(out / "confidence_interval_celltypes_proportions.csv")  # (S, K, 2)
    want = host_bootstrap_props(toy, 6).transpose(2, 1, 0)
    assert np.abs(got - want).max() <= TOL


def test_cli_uniform_init_on_the_device(tmp_path, toy, device_path):
    V, D, ref, _ = toy
    out = run_main(tmp_path, "uniform_init", RUNS["uniform_init"])
    assert len(device_path) == 1
    u0, R0, a0 = osol.init_partial("uniform", V, D, ref, 1, seed=1)
    u, alpha = osol.solve_partial(u0, R0, a0, V, D, ref, 1, n_iter1=5, n_iter2=20, tol=0.0)
    got_a = pd.read_csv(out / "celltypes_proportions.csv", index_col=0).values
    got_u = pd.read_csv(out / "methylation_profile_estimate.csv").values
    assert np.abs(got_a - alpha).max() <= 1e-8 and np.abs(got_u - u.reshape(got_u.shape)).max() <= 1e-8


def test_cli_below_the_gate_runs_the_host_code(tmp_path, toy, host_path):
    """With DEVICE_WLS_MIN_ELEMENTS as shipped the three runs make no device regression and write what the host code
    computes, bit for bit."""
    from demethify_amd import _lib as L
    from demethify_amd.deconvolution import init_BSSMF_md, solve_problem
    from demethify_amd.device import Problem, get_context
    from demethify_amd.init_func import wls_intercept

    V, D, ref, _ = toy
    out = run_main(tmp_path, "ref_based", RUNS["ref_based"])
    host = np.concatenate([wls_intercept(D[:, k:k + 1] * V[:, k:k + 1], D[:, k:k + 1], ref) for k in range(V.shape[1])], axis=1)
    assert np.array_equal(read_exact(out / "celltypes_proportions.csv", index_col=0), host)

    out = run_main(tmp_path, "bootstrap", RUNS["bootstrap"])
    want = host_bootstrap_props(toy, 6).transpose(2, 1, 0)
    assert np.array_equal(intervals(out / "confidence_interval_celltypes_proportions.csv"), want)

    out = run_main(tmp_path, "uniform_init", RUNS["uniform_init"])
    u0, _, a0 = init_BSSMF_md("uniform", V, D, ref, 1, rb_alg=wls_intercept, seed=1, _stack=False)
    with Problem(get_context(), V, D, ref) as p:
        u, alpha = solve_problem(p, u0, a0, L.DMF_MODE_PARTIAL, 5, 20, 0.0)
    assert np.array_equal(read_exact(out / "celltypes_proportions.csv", index_col=0), alpha)
    assert np.array_equal(read_exact(out / "methylation_profile_estimate.csv"), u)
