"""The SVD initialiser's host route (init_func.nndsvd_initialize / constrained_nndsvd) against arrays recorded from the
reference's own functions, the seam functions' handling of "SVD" and "ICA", and the host half of the device route
(init_func.nndsvd_from_eig) against the host route through a numpy restatement of the three kernels.

tests/golden/svd_init/reference_nndsvd.npz holds what the reference returns on the committed 350 x 10 data set
(tests/golden/upstream/output_gen, read as conftest.load_toy reads it: V, D, R), recorded with the reference's
demethify/ directory on sys.path:

    import init_func as ref
    for r in (1, 2): partial_r{r}_W, partial_r{r}_H = ref.constrained_nndsvd(V, R, D, rank=r, flag=0)
    unsup_r4_W, unsup_r4_H = ref.nndsvd_initialize(V, rank=4)
    unsup_r4_flag1_W, unsup_r4_flag1_H = ref.nndsvd_initialize(V, rank=4, flag=1)
    np.random.seed(7); unsup_r4_flag2_W, unsup_r4_flag2_H = ref.nndsvd_initialize(V, rank=4, flag=2)

The bound against the goldens is 1e-12: the same LAPACK route, and the construction does not depend on the joint sign of a
singular pair, which is all that another LAPACK build may change."""
from __future__ import annotations

import ctypes
import re

import numpy as np
import pytest

from oracle import solver as osol

from conftest import GOLDEN, ROOT

TOL = 1e-12


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN / "svd_init" / "reference_nndsvd.npz") as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("rank", [1, 2])
def test_constrained_nndsvd_matches_the_reference(toy, golden, rank):
    from demethify_amd.init_func import constrained_nndsvd

    V, D, R, _ = toy
    W, H = constrained_nndsvd(V, R, D, rank=rank, flag=0)
    assert W.shape == (350, 5 + rank) and H.shape == (5 + rank, 10)
    assert np.abs(W - golden[f"partial_r{rank}_W"]).max() <= TOL
    assert np.abs(H - golden[f"partial_r{rank}_H"]).max() <= TOL
    assert np.array_equal(W == 0, golden[f"partial_r{rank}_W"] == 0)
    assert np.array_equal(W[:, :5], R) and W[:, 5:].min() >= 0 and W[:, 5:].max() <= 1


def test_nndsvd_initialize_matches_the_reference(toy, golden):
    from demethify_amd.init_func import nndsvd_initialize

    V = toy[0]
    W, H = nndsvd_initialize(V, 4)
    assert np.abs(W - golden["unsup_r4_W"]).max() <= TOL and np.abs(H - golden["unsup_r4_H"]).max() <= TOL
    assert np.array_equal(W == 0, golden["unsup_r4_W"] == 0) and (W == 0).sum() > 0


def test_flags_one_and_two(toy, golden):
    from demethify_amd.init_func import nndsvd_initialize

    V = toy[0]
    W, H = nndsvd_initialize(V, 4, flag=1)
    assert np.abs(W - golden["unsup_r4_flag1_W"]).max() <= TOL and np.abs(H - golden["unsup_r4_flag1_H"]).max() <= TOL
    assert (W == np.mean(V)).sum() == (golden["unsup_r4_W"] == 0).sum()
    np.random.seed(7)
    W, H = nndsvd_initialize(V, 4, flag=2)
    assert np.abs(W - golden["unsup_r4_flag2_W"]).max() <= TOL and np.abs(H - golden["unsup_r4_flag2_H"]).max() <= TOL


def test_negative_input_raises(toy):
    from demethify_amd.deconvolution import _init_unsupervised
    from demethify_amd.init_func import nndsvd_initialize

    V = toy[0].copy()
    V[3, 2] = -0.25
    with pytest.raises(ValueError, match="The input matrix contains negative elements."):
        nndsvd_initialize(V, 2)
    with pytest.raises(ValueError, match="The input matrix contains negative elements."):
        _init_unsupervised("SVD", V, 2, seed=1)


def test_seam_functions_on_the_host_route(toy, golden):
    """Below the gate (350 x 10 is) the three seam functions run the host route and touch no device: u = the clipped W2,
    alpha = the projected H, with the zero guard in init_BSSMF_md only and the purity scaling as coded upstream (:262)."""
    from demethify_amd import init_func
    from demethify_amd.deconvolution import _init_unsupervised, init_BSSMF_md, init_BSSMF_md_p

    V, D, R, _ = toy
    assert not init_func.device_svd(350, 10, 5, 2)
    u, Rfull, alpha = init_BSSMF_md("SVD", V, D, R, 2, seed=3)
    assert np.abs(u - golden["partial_r2_W"][:, 5:]).max() <= TOL and np.array_equal(Rfull, np.c_[R, u])
    want = osol.simplex_project_columns(golden["partial_r2_H"])
    if want[-2:][0].all() == 0.0:
        want[-2:][0] = 1e-10
        want[:-2] = (1 - 1e-10) * want[:-2]
    assert np.abs(alpha - want).max() <= TOL
    purity = np.linspace(0.2, 0.9, 10)
    u, _, alpha = init_BSSMF_md_p("SVD", V, D, R, 2, purity)
    H = golden["partial_r2_H"]
    want = np.vstack((purity * osol.simplex_project_columns(H[:-2]), osol.simplex_project_columns(H[-2:])))
    assert np.abs(alpha - want).max() <= TOL
    assert np.abs(alpha[-2:].sum(axis=0) - 1).max() <= 1e-12  # the unknown block is NOT scaled by 1 - purity
    u, alpha = _init_unsupervised("SVD", V, 4, seed=None, d_x=D)
    assert np.abs(u - golden["unsup_r4_W"].clip(0, 1)).max() <= TOL
    assert np.abs(alpha - osol.simplex_project_columns(golden["unsup_r4_H"])).max() <= TOL


def test_host_projection_is_the_reference_projection():
    from demethify_amd.init_func import project_simplex_columns

    X = np.random.RandomState(0).normal(size=(9, 40)) * np.array([0.01, 1, 5, 30])[np.arange(40) % 4]
    X[:, 3] = 0.0
    X[2:, 5] = X[1, 5]
    assert np.array_equal(project_simplex_columns(X), osol.simplex_project_columns(X))
    assert np.array_equal(project_simplex_columns(X, 0.4), osol.simplex_project_columns(X, 0.4))


def test_bcv_fold_initialises_from_the_masked_arrays_on_the_host(toy, monkeypatch):
    """A bi-cross-validation fold draws its mask first, then runs the SVD initialiser on the masked HOST arrays: the host
    route whatever the size (the gate is at zero here), no device touched."""
    from demethify_amd import init_func
    from demethify_amd.ic import _bcv_draw_fold

    monkeypatch.setattr(init_func, "DEVICE_SVD_MIN_ELEMENTS", 0)
    V, D, R, _ = toy
    np.random.seed(11)
    mask, u0, a0, staged = _bcv_draw_fold(V, D, R, 2, "SVD", 11, 0.3)
    np.random.seed(11)
    want_mask = np.random.rand(*V.shape) < 0.3
    assert staged is None and np.array_equal(mask, want_mask)
    W, H = init_func.constrained_nndsvd(V * mask, R, D * mask, rank=2)
    assert np.array_equal(u0, W[:, 5:])
    want = osol.simplex_project_columns(H)
    if want[-2:][0].all() == 0.0:
        want[-2:][0] = 1e-10
        want[:-2] = (1 - 1e-10) * want[:-2]
    assert np.abs(a0 - want).max() <= TOL
    mask, u0, a0, _ = _bcv_draw_fold(V, D, None, 3, "SVD", 11, 0.3)
    W, H = init_func.nndsvd_initialize(V * mask, 3)
    assert np.array_equal(u0, W.clip(0, 1)) and np.abs(a0 - osol.simplex_project_columns(H)).max() <= TOL


def test_more_unknowns_than_samples_falls_back_to_uniform_(toy):
    from demethify_amd.deconvolution import _init_unsupervised, init_BSSMF_md

    V, D, R, _ = toy
    V3, D3 = V[:, :3], D[:, :3]
    u, _, alpha = init_BSSMF_md("SVD", V3, D3, R, 4, seed=5)
    wu, _, wa = init_BSSMF_md("uniform_", V3, D3, R, 4, seed=5)
    assert np.array_equal(u, wu) and np.array_equal(alpha, wa)
    u, alpha = _init_unsupervised("SVD", V3, 4, seed=5)
    wu, wa = _init_unsupervised("uniform_", V3, 4, seed=5)
    assert np.array_equal(u, wu) and np.array_equal(alpha, wa)


def test_ica_still_raises(toy):
    from demethify_amd.deconvolution import _init_unsupervised, init_BSSMF_md, init_BSSMF_md_p

    V, D, R, _ = toy
    for call in (lambda: init_BSSMF_md("ICA", V, D, R, 1), lambda: init_BSSMF_md_p("ICA", V, D, R, 1, np.ones(10)),
                 lambda: _init_unsupervised("ICA", V, 1, None)):
        with pytest.raises(NotImplementedError, match="N x N covariance"):
            call()


def test_entry_points_are_declared_bound_and_exported():
    from demethify_amd import _build, _lib

    _build.build()
    header = (ROOT / "include" / "demethify_hip.h").read_text()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("dmf_svd_gram", "dmf_svd_factor", "dmf_svd_finish"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert _lib.load().dmf_abi_version() == 1  # additive


def test_gate_follows_the_kernels_limits():
    from demethify_amd import init_func

    n = init_func.DEVICE_SVD_MIN_ELEMENTS
    assert init_func.device_svd(n, 1, 0, 1) and not init_func.device_svd(n - 1, 1, 0, 1)
    assert init_func.device_svd(1 << 20, 512, 64, 30) and init_func.device_svd(1 << 20, 256, 48, 64)
    assert not init_func.device_svd(1 << 20, 513, 4, 4) and not init_func.device_svd(1 << 20, 512, 4, 31)
    assert not init_func.device_svd(1 << 20, 64, 65, 4) and not init_func.device_svd(1 << 20, 64, 4, 65)


# ---- the Gram route, restated in numpy, against the LAPACK route ------------------------------------------------------

def gram_route(Y, rank):
    """What dmf_svd_gram, numpy.linalg.eigh, dmf_svd_factor and dmf_svd_finish compute, in numpy -> (u0, H2)."""
    from demethify_amd.init_func import nndsvd_from_eig

    lam, vec = np.linalg.eigh(Y.T @ Y)
    lam, vec = lam[::-1][:rank], vec[:, ::-1][:, :rank]
    sigma = np.sqrt(lam)
    T = Y @ (vec / sigma)
    norms = np.stack([(np.maximum(T, 0) ** 2).sum(axis=0), (np.maximum(-T, 0) ** 2).sum(axis=0)])
    sign, scale, H2 = nndsvd_from_eig(sigma, vec, norms)
    W = scale * np.where(sign == 0, np.abs(T), np.maximum(sign * T, 0))
    W[W < 1e-11] = 0
    return np.clip(W, 0, 1), H2


ROUTE_SHAPES = [(4096, 7, 6, 2), (1000, 5, 12, 4), (3000, 9, 0, 4), (2048, 65, 6, 3), (33, 3, 2, 1), (777, 4, 3, 1, 5)]


@pytest.mark.parametrize("shape", ROUTE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gram_route_equals_the_svd_route(shape):
    """DESIGN section 7b's table on the shapes that run in a second: the two routes agree three orders of magnitude inside
    the 1e-10 bar of the GPU tests, zeros included."""
    from demethify_amd.init_func import nndsvd_initialize, wls_intercept

    N, S, n_c, n_u = shape[:4]
    V, D, Rt = osol.synthetic_problem(N, S, n_c, n_u, **({"depth": shape[4]} if len(shape) > 4 else {}))
    if n_c:
        H1 = np.concatenate([wls_intercept(V[:, k:k + 1], D[:, k:k + 1], Rt) for k in range(S)], axis=1)
        Y = np.maximum(V - Rt @ H1, 1e-8)
    else:
        Y = V
    W, H = nndsvd_initialize(Y, n_u)
    u0, H2 = gram_route(Y, n_u)
    du, dh = np.abs(u0 - np.clip(W, 0, 1)).max(), np.abs(H2 - H).max()
    print(f"{shape}: max |du0| {du:.2e}, max |dH2| {dh:.2e}")
    assert du <= 1e-12 and dh <= 1e-12
    assert np.array_equal(u0 == 0, W == 0) and np.array_equal(H2 == 0, H == 0)
