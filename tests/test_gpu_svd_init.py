"""The SVD initialiser on the device: dmf_svd_gram against ``Yres.T @ Yres`` in numpy, Problem.nndsvd (k_svd_gram, the
host's eigh, k_svd_project, k_svd_finish) against the host route of init_func, and the callers behind
``init_func.DEVICE_SVD_MIN_ELEMENTS``.

Bounds.  The Gram: 1e-12 max|C|, twice the worst case N 2^-53 of a sum of N <= 4096 positive products.  The factors:
the project's 1e-10 of the known-answer tests -- on the CPU the Gram route and the LAPACK route differ by 5.6e-14 (u0) and
1.8e-13 (alpha0) at most on these shapes, provided no positive / negative decision is a near tie and
the used eigenvalues are separated, which every case asserts on the host route's result first."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from oracle import drivers as odrv
from oracle import solver as osol

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TOL = 1e-10


def host_h1(V, D, Rt):
    from demethify_amd.init_func import wls_intercept

    return np.concatenate([wls_intercept(V[:, k:k + 1], D[:, k:k + 1], Rt) for k in range(V.shape[1])], axis=1)


def project(H, n_u, guard=True):
    """projection_simplex_sort_2d and the zero guard of deconvolution.py:74-76, by the oracle."""
    alpha = osol.simplex_project_columns(H)
    if guard and alpha[-n_u:][0].all() == 0.0:
        alpha[-n_u:][0] = 1e-10
        alpha[:-n_u] = (1 - 1e-10) * alpha[:-n_u]
    return alpha


def decision_margins(Y, rank):
    """(smallest relative margin |termp - termn| / max of init_func.py:63 over components 1 .. rank - 1, smallest gap
    between consecutive used eigenvalues of Y^T Y relative to the largest)."""
    from scipy.linalg import svd

    U, s, Et = svd(Y, full_matrices=False)
    margin = np.inf
    for i in range(1, rank):
        tp = np.linalg.norm(np.maximum(U[:, i], 0)) * np.linalg.norm(np.maximum(Et[i], 0))
        tn = np.linalg.norm(np.maximum(-U[:, i], 0)) * np.linalg.norm(np.maximum(-Et[i], 0))
        margin = min(margin, abs(tp - tn) / max(tp, tn))
    lam = s[:rank] ** 2
    gap = np.min(-np.diff(lam)) / lam[0] if rank > 1 else np.inf
    return margin, gap


@functools.lru_cache(maxsize=None)
def case(N, S, n_c, n_u, depth=50):
    """One synthetic shape and its host route, computed once per session and never written to:
    (V, D, Rt, H1, Yres, u0, H, alpha0)."""
    from demethify_amd.init_func import nndsvd_initialize

    V, D, Rt = osol.synthetic_problem(N, S, n_c, n_u, depth=depth)
    if n_c:
        H1 = host_h1(V, D, Rt)
        Y = np.maximum(V - Rt @ H1, 1e-8)
    else:
        Rt, H1, Y = None, None, V
    W2, H2 = nndsvd_initialize(Y, n_u)
    u0 = np.clip(W2, 0, 1)
    H = np.vstack([H1, H2]) if n_c else H2
    out = (V, D, Rt, H1, Y, u0, H, project(H, n_u))
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def ids(s):
    return "x".join(map(str, s))


GRAM_SHAPES = [(33, 3, 2, 1), (777, 4, 3, 1, 5), (4096, 7, 6, 2), (2048, 65, 6, 3), (2048, 130, 6, 8), (2048, 256, 12, 4),
               (3000, 9, 0, 4), (1024, 16, 48, 2)]


@pytest.mark.parametrize("shape", GRAM_SHAPES, ids=ids)
def test_gram(ctx, shape):
    """Fewer rows than one row block; a ragged last block; S no multiple of 4; one sample past one and past two 64-column
    groups; four column groups (two workgroups per row slab); no residual; the widest H1."""
    from demethify_amd.device import Problem

    V, D, Rt, H1, Y, *_ = case(*shape)
    want = Y.T @ Y
    with Problem(ctx, V, D, Rt) as p:
        got, negatives, nonfinite = p.svd_gram(H1)
        again, _, _ = p.svd_gram(H1)
    err = float(np.abs(got - want).max())
    print(f"gram {shape}: max abs diff {err:.3e} of max |C| {np.abs(want).max():.3e}")
    assert err <= 1e-12 * np.abs(want).max()
    assert np.array_equal(got, got.T)
    assert np.array_equal(got, again)
    assert negatives == 0 and nonfinite == 0


def test_gram_counts_negative_entries(ctx):
    from demethify_amd.device import Problem

    V, D, *_ = case(3000, 9, 0, 4)
    V = V.copy()
    V[1234, 5] = -0.25
    with Problem(ctx, V, D, None) as p:
        got, negatives, nonfinite = p.svd_gram(None)
        assert (negatives, nonfinite) == (1, 0)
        assert np.abs(got - V.T @ V).max() <= 1e-12 * np.abs(got).max()
        with pytest.raises(ValueError, match="The input matrix contains negative elements."):
            p.nndsvd(2)


@pytest.mark.parametrize("shape", [(300, 256, 0, 64), (300, 512, 3, 30), (100, 320, 0, 54), (1000, 5, 12, 4)], ids=ids)
def test_projection_against_numpy(ctx, shape):
    """k_svd_project and k_svd_finish on their own, at the three corners of the LDS limit (149, 157 and 160 KB) and at a
    rank that is no power of two: T = Yres @ B for a positive B with column sums 1 / 2, so that every t lies in
    (1e-11, 1) and sign 0, scale 1 returns T itself.  Bound: S 2^-53 <= 5.7e-14 for a sum of S positive products below 1."""
    from demethify_amd.device import Problem

    N, S, n_c, rank = shape
    V, D, Rt = osol.synthetic_problem(N, S, n_c, 2)
    H1 = host_h1(V, D, Rt) if n_c else None
    Y = np.maximum(V - Rt @ H1, 1e-8) if n_c else V
    B = np.random.RandomState(5).uniform(0.1, 1.0, size=(S, rank))
    B /= 2 * B.sum(axis=0)
    want = Y @ B
    assert want.min() > 1e-11 and want.max() < 1
    with Problem(ctx, V, D, Rt if n_c else None) as p:
        t_dev, norms = p.svd_factor(H1, B)
        got = p.svd_finish(t_dev, np.zeros(rank), np.ones(rank))
        t_dev, _ = p.svd_factor(H1, B)
        sign = np.where(np.arange(rank) % 2, -1.0, 1.0)
        half = p.svd_finish(t_dev, sign, np.full(rank, 3.0))
    print(f"project {shape}: max abs diff {np.abs(got - want).max():.3e}")
    assert np.abs(got - want).max() <= 1e-13
    assert np.allclose(norms[0], (want ** 2).sum(axis=0), rtol=1e-12, atol=0) and np.array_equal(norms[1], np.zeros(rank))
    assert np.array_equal(half[:, 1::2], np.zeros_like(half[:, 1::2]))
    assert np.abs(half[:, ::2] - np.minimum(3.0 * want[:, ::2], 1.0)).max() <= 3e-13


def check_against_host(u0, H, n_u, want_u0, want_alpha, label, guard=True):
    alpha = project(H, n_u, guard)
    du, da = float(np.abs(u0 - want_u0).max()), float(np.abs(alpha - want_alpha).max())
    print(f"nndsvd {label}: max |du0| {du:.3e}, max |dalpha0| {da:.3e}, zeros {(want_u0 == 0).sum()}")
    assert du <= TOL and da <= TOL
    assert np.array_equal(u0 == 0, want_u0 == 0)


@pytest.mark.parametrize("shape", GRAM_SHAPES + [(4096, 64, 12, 16)], ids=ids)
def test_nndsvd_matches_the_host_route(ctx, shape):
    from demethify_amd.device import Problem

    V, D, Rt, H1, Y, want_u0, _, want_alpha = case(*shape)
    n_u = shape[3]
    margin, gap = decision_margins(Y, n_u)
    print(f"{shape}: decision margin {margin:.3e}, eigenvalue gap {gap:.3e}")
    assert margin >= 1e-3 and gap >= 1e-4
    with Problem(ctx, V, D, Rt) as p:
        u0, H = p.nndsvd(n_u, host_arrays=(V, D, Rt))
        if Rt is not None:
            assert (p.wls_status == 0).all()
    check_against_host(u0, H, n_u, want_u0, want_alpha, shape)


def test_declined_sample_takes_h1_from_the_host(ctx):
    """A duplicated reference column: the device regression declines every sample (status 1), H1 comes from the host
    regression, the rest still runs on the device."""
    from demethify_amd.device import Problem
    from demethify_amd.init_func import constrained_nndsvd

    V, D, Rt, *_ = case(1000, 5, 12, 4)
    Rd = np.ascontiguousarray(np.c_[Rt[:, :4], Rt[:, 1]])
    W, H = constrained_nndsvd(V, Rd, D, 2)
    margin, gap = decision_margins(np.maximum(V - Rd @ H[:5], 1e-8), 2)
    assert margin >= 1e-3 and gap >= 1e-4
    with Problem(ctx, V, D, Rd) as p:
        u0, Hd = p.nndsvd(2, host_arrays=(V, D, Rd))
        assert (p.wls_status == 1).all()
        with pytest.raises(RuntimeError):
            p.nndsvd(2)
    assert np.array_equal(Hd[:5], H[:5])
    check_against_host(u0, Hd, 2, W[:, 5:], project(H, 2), "declined")


def test_unsupported_shape_takes_the_host_route(ctx):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem
    from demethify_amd.init_func import constrained_nndsvd

    V, D, Rt = osol.synthetic_problem(64, 513, 2, 1)
    W, H = constrained_nndsvd(V, Rt, D, 1)
    with Problem(ctx, V, D, Rt) as p:
        with pytest.raises(L.DemethifyHipError) as e:
            p.svd_gram(H[:2])
        assert e.value.status == L.DMF_ERR_UNSUPPORTED
        u0, Hd = p.nndsvd(1, host_arrays=(V, D, Rt))
    assert np.array_equal(u0, W[:, 2:]) and np.array_equal(Hd, H)


def test_masked_problem_is_refused(ctx):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem

    V, D, Rt, H1, *_ = case(777, 4, 3, 1, 5)
    mask = np.random.RandomState(2).uniform(size=V.shape) < 0.7
    with Problem(ctx, V, D, Rt) as full, full.masked(mask) as fold:
        with pytest.raises(L.DemethifyHipError) as e:
            fold.svd_gram(H1)
        assert e.value.status == L.DMF_ERR_BAD_ARG


COUNT_SHAPE = (4096, 7, 6, 2)


def test_x16_on_and_off_agree_bit_for_bit(ctx):
    from demethify_amd.device import Problem

    V, D, Rt, H1, *_ = case(*COUNT_SHAPE)
    out = []
    for on in (False, True):
        try:
            ctx.set_x16(on)
            with Problem(ctx, V, D, Rt) as p:
                out.append((p.svd_gram(H1)[0],) + p.nndsvd(2))
        finally:
            ctx.set_x16(True)
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_regression_from_the_f64_arrays_ignores_x16(ctx):
    """H1 as nndsvd asks for it (f64_arrays): bit-identical with X16 on and off, and within the regression's 1e-10 of the
    default form, which reads (X16, D16) where the problem carries them."""
    from demethify_amd.device import Problem

    V, D, Rt, H1, *_ = case(*COUNT_SHAPE)
    got = []
    for on in (False, True):
        try:
            ctx.set_x16(on)
            with Problem(ctx, V, D, Rt) as p:
                got.append(p.wls_intercept(None, "v", f64_arrays=True))
                default = p.wls_intercept(None, "v")
        finally:
            ctx.set_x16(True)
    assert np.array_equal(got[0], got[1])
    assert np.abs(got[1] - default).max() <= TOL and np.abs(got[1] - H1).max() <= TOL


def test_generic_level_one(ctx):
    from demethify_amd.device import Problem

    V, D, Rt, _, _, want_u0, _, want_alpha = case(*COUNT_SHAPE)
    try:
        ctx.set_generic(1)
        with Problem(ctx, V, D, Rt) as p:
            u0, H = p.nndsvd(2)
    finally:
        ctx.set_generic(0)
    check_against_host(u0, H, 2, want_u0, want_alpha, "generic level 1")


def test_gathered_problem(ctx):
    from demethify_amd.device import Problem
    from demethify_amd.init_func import constrained_nndsvd
    from demethify_amd.staging import indices_to_device

    V, D, Rt = osol.synthetic_problem(3000, 6, 5, 2)
    idx = np.random.RandomState(3).randint(0, 3000, size=3000)
    W, H = constrained_nndsvd(V[idx], Rt[idx], D[idx], 2)
    margin, gap = decision_margins(np.maximum(V[idx] - Rt[idx] @ H[:5], 1e-8), 2)
    assert margin >= 1e-3 and gap >= 1e-4
    with Problem(ctx, V, D, Rt) as full, full.gather(indices_to_device(idx, ctx)) as resampled:
        u_dev, Hd = resampled.nndsvd(2, keep_on_device=True)
        assert u_dev.is_cuda and u_dev.shape == (3000, 2)
        u0, Hd2 = resampled.nndsvd(2)
    assert np.array_equal(Hd, Hd2)
    check_against_host(u0, Hd, 2, W[:, 5:], project(H, 2), "gathered")


# ---- the callers ------------------------------------------------------------------------------------------------------

@pytest.fixture
def device_route(monkeypatch):
    """The gate at zero, and a count of the device initialisations a run makes."""
    from demethify_amd import init_func
    from demethify_amd.device import Problem

    calls = []
    inner = Problem.nndsvd

    def counted(self, *a, **kw):
        calls.append(self.N)
        return inner(self, *a, **kw)

    monkeypatch.setattr(init_func, "DEVICE_SVD_MIN_ELEMENTS", 0)
    monkeypatch.setattr(Problem, "nndsvd", counted)
    return calls


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN / "svd_init" / "reference_nndsvd.npz") as z:
        return {k: z[k] for k in z.files}


def test_purity_block_scaling_on_the_device(ctx, device_route):
    """deconvolution.py:262 as coded: the known block scaled by the purity, the unknown block left at mass 1, no guard."""
    from demethify_amd.deconvolution import init_BSSMF_md_p

    V, D, Rt, _, _, want_u0, H, _ = case(1000, 5, 12, 4)
    purity = np.linspace(0.3, 0.8, 5)
    u, R, alpha = init_BSSMF_md_p("SVD", V, D, Rt, 4, purity, _stack=False)
    assert len(device_route) == 1 and R is None
    want = np.vstack((purity * osol.simplex_project_columns(H[:-4]), osol.simplex_project_columns(H[-4:])))
    assert np.abs(alpha - want).max() <= TOL and np.abs(u - want_u0).max() <= TOL
    assert np.abs(alpha[-4:].sum(axis=0) - 1).max() <= 1e-12 and np.abs(alpha[:-4].sum(axis=0) - purity).max() <= 1e-12


def test_partial_solve_from_the_svd_init(ctx, toy, golden, device_route):
    from demethify_amd import _lib as L
    from demethify_amd.deconvolution import init_BSSMF_md, solve_problem
    from demethify_amd.device import Problem

    V, D, ref, _ = toy
    u0, _, a0 = init_BSSMF_md("SVD", V, D, ref, 1, _stack=False)
    assert len(device_route) == 1
    with Problem(ctx, V, D, ref) as p:
        u, alpha = solve_problem(p, u0, a0, L.DMF_MODE_PARTIAL, 5, 20, 0.0)
    gu = np.ascontiguousarray(golden["partial_r1_W"][:, 5:])
    wu, wa = osol.solve_partial(gu, np.c_[ref, gu], project(golden["partial_r1_H"], 1), V, D, ref, 1, n_iter1=5, n_iter2=20,
                                tol=0.0)
    assert np.abs(u - wu.reshape(u.shape)).max() <= 1e-8 and np.abs(alpha - wa).max() <= 1e-8


def test_unsupervised_solve_from_the_svd_init(ctx, toy, golden, device_route):
    from demethify_amd.deconvolution import unsupervised_deconv

    V, D, _, _ = toy
    u, alpha = unsupervised_deconv(V, 4, D, "SVD", n_iter1=5, n_iter2=20, tol=0.0)
    assert len(device_route) == 1
    init = (golden["unsup_r4_W"].clip(0, 1), project(golden["unsup_r4_H"], 4, guard=False))
    wu, wa = osol.solve_unsupervised(V, 4, D, "SVD", n_iter1=5, n_iter2=20, tol=0.0, init=init)
    assert np.abs(u - wu).max() <= 1e-8 and np.abs(alpha - wa).max() <= 1e-8


def host_init_partial(V, D, Rt, n_u):
    from demethify_amd.init_func import constrained_nndsvd

    W, H = constrained_nndsvd(V, Rt, D, n_u)
    u = np.ascontiguousarray(W[:, Rt.shape[1]:])
    return u, np.c_[Rt, u], project(H, n_u)


def intervals(path):
    import pandas as pd

    table = pd.read_csv(path, index_col=0)
    return np.array([[eval(cell, {"np": np}) for cell in table[col]] for col in table.columns])


def test_bootstrap_with_the_svd_init(ctx, toy, tmp_path, device_route):
    from demethify_amd.bootstrap import bt_ci

    V, D, ref, header = toy
    samples = [f"s{k}" for k in range(V.shape[1])]
    bt_ci(95, 4, 1, V, D, ref, "SVD", 5, 20, 0.0, header, str(tmp_path), samples, None, 1)
    assert device_route == [350] * 4
    alphas = []
    for s in osol.bootstrap_seeds(1, 4):
        idx = osol.bootstrap_indices(s, V.shape[0])
        u, R, a = host_init_partial(V[idx], D[idx], ref[idx], 1)
        alphas.append(osol.solve_partial(u, R, a, V[idx], D[idx], ref[idx], 1, 5, 20, 0.0)[1])
    lo, hi = odrv.percentile_bounds(np.stack(alphas), 95)
    got = intervals(tmp_path / "confidence_interval_celltypes_proportions.csv")  # (S, K, 2)
    assert np.abs(got - np.stack([lo, hi]).transpose(2, 1, 0)).max() <= 1e-8


def test_aic_sweep_with_the_svd_init(ctx, toy, device_route):
    from demethify_amd.ic import evaluate_best_ic

    V, D, ref, _ = toy
    u, alpha, n_best, scores = evaluate_best_ic(V, ref, D, "SVD", "AIC", 1, 5, 20, 0.0, n_u_values=range(1, 4))
    assert device_route == [350] * 3
    want = []
    for n_u in range(1, 4):
        u0, R, a0 = host_init_partial(V, D, ref, n_u)
        wu, wa = osol.solve_partial(u0, R, a0, V, D, ref, n_u, 5, 20, 0.0)
        want.append(osol.aic_as_coded(osol.weighted_cost(V, np.c_[ref, wu.reshape(-1, n_u)], wa, D), n_u, 350, 5, 10))
    assert n_best == 1 + int(np.argmin(want))
    assert np.allclose(scores, want, rtol=1e-9, atol=0)
