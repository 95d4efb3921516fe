"""Component matching for the bootstrap, host side: the assignment rule, what it leaves unchanged, the refusals of the
no-reference bootstrap that come before any device work, and the two entry points' declarations.  No GPU."""
import ctypes
import itertools
import re

import numpy as np
import pytest

from conftest import ROOT


def _brute_force(P):
    n = P.shape[0]
    return max(sum(P[a, perm[a]] for a in range(n)) for perm in itertools.permutations(range(n)))


@pytest.mark.parametrize("n_u", [1, 2, 3, 4, 5, 6])
def test_assignment_matches_brute_force(n_u):
    from demethify_amd.bootstrap import match_components

    rs = np.random.RandomState(100 + n_u)
    for _ in range(20):
        P = rs.rand(n_u, n_u) * rs.choice([1.0, 50.0, 1e4])
        perm = match_components(P)
        assert sorted(perm.tolist()) == list(range(n_u))
        got = sum(P[a, perm[a]] for a in range(n_u))
        want = _brute_force(P)
        # both are sums of the same n_u entries of P when the maximiser is unique; eps covers the order of the additions
        assert abs(got - want) <= 4 * n_u * np.finfo(np.float64).eps * want


@pytest.mark.parametrize("n_u", [2, 3, 4, 6, 9])
def test_planted_permutation_is_recovered(n_u):
    from demethify_amd.bootstrap import match_components

    rs = np.random.RandomState(n_u)
    Q = np.eye(n_u) * 10.0 + rs.rand(n_u, n_u)  # replicate component a is anchor component a, before the shuffle
    for _ in range(10):
        perm = rs.permutation(n_u)
        P = np.empty_like(Q)
        P[:, perm] = Q  # replicate component a now matches anchor component perm[a]
        P += 0.1 * rs.rand(n_u, n_u)
        assert match_components(P).tolist() == perm.tolist()
        # the issue's form: P = Q[:, perm] + noise puts the heavy entry of row a in column argsort(perm)[a]
        P2 = Q[:, perm] + 0.1 * rs.rand(n_u, n_u)
        assert match_components(P2).tolist() == np.argsort(perm).tolist()


def test_diagonal_dominant_gives_the_identity():
    from demethify_amd.bootstrap import match_components

    rs = np.random.RandomState(7)
    for n_u in (1, 2, 5, 12):
        P = rs.rand(n_u, n_u) + np.eye(n_u) * n_u
        assert match_components(P).tolist() == list(range(n_u))
    with pytest.raises(ValueError):
        match_components(np.ones((2, 3)))


@pytest.mark.parametrize("n_c,n_u", [(0, 3), (2, 4), (5, 2)])
def test_alignment_leaves_the_fit_unchanged_bit_for_bit(n_c, n_u):
    """u[:, order] with alpha[-n_u:][order] is the same model: every row-times-column product has the same terms, and
    with them laid out in the same order the product is the same bits."""
    rs = np.random.RandomState(n_c * 10 + n_u)
    u = rs.rand(200, n_u)
    alpha = rs.dirichlet(np.ones(n_c + n_u), 7).T
    perm = rs.permutation(n_u)
    order = np.argsort(perm)
    u2 = u[:, order]
    alpha2 = alpha.copy()
    alpha2[n_c:] = alpha[n_c:][order]
    assert np.array_equal(alpha2[:n_c], alpha[:n_c])
    # term by term: component order[b] of the replicate sits at position b after the alignment
    want = np.zeros((200, 7))
    got = np.zeros((200, 7))
    for b in range(n_u):
        want += u[:, order[b]][:, None] * alpha[n_c + order[b]][None, :]
        got += u2[:, b][:, None] * alpha2[n_c + b][None, :]
    assert np.array_equal(got, want)
    # the matrix product itself, on dyadic inputs (multiples of 2**-10: every product and partial sum is exact, so the
    # order in which a BLAS adds the n_u terms cannot show) -- bit for bit
    ud = np.round(u * 1024) / 1024
    ad = np.round(alpha * 1024) / 1024
    ad2 = ad.copy()
    ad2[n_c:] = ad[n_c:][order]
    assert np.array_equal(ud[:, order] @ ad2[n_c:], ud @ ad[n_c:])
    # ... and on the random ones to the rounding of n_u additions
    assert np.allclose(u2 @ alpha2[n_c:], u @ alpha[n_c:], rtol=0, atol=4 * n_u * np.finfo(np.float64).eps)
    # aligned column perm[a] is the replicate's column a
    for a in range(n_u):
        assert np.array_equal(u2[:, perm[a]], u[:, a])


def test_no_reference_refusals_come_before_any_device_work(tmp_path, monkeypatch):
    from demethify_amd import bootstrap

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(bootstrap, "get_context", no_device)
    monkeypatch.setattr(bootstrap, "Problem", no_device)
    rs = np.random.RandomState(0)
    V, D = rs.rand(30, 4), rs.randint(1, 20, size=(30, 4))
    names = [f"s{i}" for i in range(4)]

    def call(init_option, purity=None, n_u=2):
        return bootstrap.bt_ci(90, 3, n_u, V, D, None, init_option, 5, 5, 0.0, [], str(tmp_path), names, purity, 1)

    with pytest.raises(NameError, match="R_trunc"):
        call("uniform")
    with pytest.raises(NotImplementedError, match="ICA"):
        call("ICA")
    with pytest.raises(ValueError, match="purity"):
        call("uniform_", purity=[50.0] * 4)
    with pytest.raises(ValueError, match="unknown"):
        call("uniform_", n_u=0)
    assert not list(tmp_path.iterdir())


def test_entry_points_are_declared_bound_and_exported():
    from demethify_amd import _build, _lib

    _build.build()
    header = (ROOT / "include" / "demethify_hip.h").read_text()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("dmf_solver_match_components", "dmf_solver_get_u_permuted"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert len(_lib.SIGNATURES["dmf_solver_match_components"][1]) == 5
    assert len(_lib.SIGNATURES["dmf_solver_get_u_permuted"][1]) == 3
    assert _lib.load().dmf_abi_version() == 1  # additive: no signature changed
    # null handles are refused without a device
    assert _lib.load().dmf_solver_match_components(None, None, 0, None, None) == _lib.DMF_ERR_BAD_ARG
    assert _lib.load().dmf_solver_get_u_permuted(None, None, None) == _lib.DMF_ERR_BAD_ARG
