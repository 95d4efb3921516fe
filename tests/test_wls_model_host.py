"""tests/wls_model.py without a GPU: every tabled case reaches the branch of k_nnls_intercept / k_wls_moments that its name
claims (the model's counters are the evidence), the model agrees with scipy.optimize.nnls on every tabled system, the shapes
that tests/test_gpu_wls.py already had reach NONE of the step-back code, the dyadic family is exact, and the two read-back
entry points are declared, bound, exported and check their arguments.

The searches behind wls_model.SEARCHED and behind the two cases that do NOT exist:

    hits, tried = wls_model.search_events(range(100000, 109100), recipe)   # recipe = "correlated", then "collinear"

200 200 systems in all (K = 2 .. 12 per seed).  Outcome: 0 rejected candidates, 0 emptied passive sets (in either recipe, at
any status), so neither has a test; second trips of the step-back loop in about a hundred systems (the first: K = 3, seed
100063, which ends with a single positive coefficient; the tabled one, K = 9, seed 100673, ends with three); one re-entry of a
dropped variable (K = 8, seed 102784).  No input is known that reaches the cap of 3 K factorisations.
"""
from __future__ import annotations

import ctypes
import re

import numpy as np
import pytest

from oracle import solver as osol

import wls_model as wm
from conftest import ROOT

TOL = 1e-10  # tests/test_gpu_wls.py's bar


def events(s):
    return wm.active_set_events(s.A, s.b)


# ------------------------------------------------------------------------------------------------ the solver's cases
def _check_batch(K):
    drops, worst = 0, 0.0
    for s in wm.correlated_batch(K):
        e = events(s)
        assert e.status == 0 and e.rejections == 0 and e.emptied == 0 and e.iterations <= 3 * K
        drops += e.drops
        worst = max(worst, float(np.abs(wm.proportions(e.x) - wm.scipy_proportions(s.M, s.y)).max()))
    assert worst <= TOL
    assert drops >= 1 or K == 1
    return drops, worst


def test_every_K_has_a_drop():
    """All 64 batches of tests/test_gpu_wls_exact.py: at least one drop per K >= 2, status 0 throughout, the model at
    scipy to 1e-10 (measured: 7 to 22 drops per K, 3.6e-14)."""
    stats = [_check_batch(K) for K in range(1, 65)]
    print("drops per K", [d for d, _ in stats], "worst vs scipy", max(w for _, w in stats))
    assert stats[0][0] == 0 and min(d for d, _ in stats[1:]) >= 1


@pytest.mark.parametrize("name", sorted(wm.NAMED_EVIDENCE))
def test_named_systems_reach_their_branch(name):
    s = wm.named_systems()[name]
    e = events(s)
    print(name, e._replace(x=None))
    assert e.status == 0 and wm.NAMED_EVIDENCE[name](e)
    assert np.abs(wm.proportions(e.x) - wm.scipy_proportions(s.M, s.y)).max() <= TOL


def test_two_drop_system_is_exact():
    """Both coefficients reach zero in the same step, in exact arithmetic: x = (0, 0, 160 / 9, 1 / 2)."""
    s = wm.two_drop_system()
    e = events(s)
    assert e.order == (0, 1, 2, 3) and e.dual_ties == 2 and e.multi_drops == 1 and e.drops == 2 and e.second_trips == 0
    assert np.array_equal(e.x, [0.0, 0.0, 2.5 / (9.0 / 64.0), 0.5])


def test_searched_names_are_all_tabled():
    assert set(wm.named_systems()) == set(wm.NAMED_EVIDENCE)
    assert "rejection" not in wm.SEARCHED and "emptied" not in wm.SEARCHED  # (none found: module docstring)


def test_a_slice_of_the_search_is_repeatable():
    """The seeds the searched cases came from, and a few hundred systems around them: the counters the table quotes."""
    hits, tried = wm.search_events(range(100060, 100066), "correlated")
    assert tried == 66 and (3, 100063, 0) in hits["second_trips"]
    assert not hits["rejections"] and not hits["emptied"]
    hits, _ = wm.search_events([100673], "correlated", ks=[9])
    assert hits["second_trips"] == [(9, 100673, 0)]
    hits, _ = wm.search_events([102784], "correlated", ks=[8])
    assert hits["reentries"] == [(8, 102784, 0)]
    hits, _ = wm.search_events(range(100000, 100010), "collinear")
    assert not hits["rejections"] and not hits["emptied"]


@pytest.mark.parametrize("S", [1, 2, 65, 300])
def test_status_batches(S):
    """Status 1 of the model on exactly and nearly duplicated columns (the pivot is about 1e-20 A_jj against a threshold of
    32 x 2^-52), status 0 on the solvable samples, which also agree with scipy."""
    G, mom, want, systems = wm.status_batch(S)
    K = G.shape[1]
    assert set(want.tolist()) == ({0} if S == 1 else {0, 1} if S == 2 else {0, 1, 2})
    for s in range(S):
        if want[s] == 2:
            assert not (mom[2 * K, s] > 0.0)
            continue
        A, b = wm.centred_system(G[s], mom[:, s])
        assert np.array_equal(A, G[s])  # (m = 0, sw = 1: the system as built)
        e = wm.active_set_events(A, b)
        assert e.status == want[s]
        if want[s] == 0:
            assert np.abs(wm.proportions(e.x) - wm.scipy_proportions(systems[s].M, systems[s].y)).max() <= TOL


def test_near_duplicate_pivot_is_far_below_the_threshold():
    """No status case sits near K 2^-52 A_jj: the computed pivot of the duplicate, exact or perturbed, is rounding noise
    below a quarter of the threshold (at most an eighth by the error analysis of wls_model.status_batch), and the smallest
    relative pivot of a solvable sample is a thousand thresholds up."""
    G, mom, want, _ = wm.status_batch(300)
    K = G.shape[1]
    tol = K * 2.0 ** -52
    for s in np.flatnonzero(want == 1):
        l10 = G[s][0, 1] / np.sqrt(G[s][0, 0])
        assert abs(G[s][1, 1] - l10 * l10) <= 0.25 * tol * G[s][1, 1]
    for s in np.flatnonzero(want == 0):
        L = wm._factor(G[s], list(range(K)), 0.0)
        assert (np.diag(L) ** 2 / np.diag(G[s])).min() > 1e3 * tol


# ------------------------------------------------------------------------------------------------ the public route
@pytest.mark.parametrize("K", wm.ROUTE_K)
def test_route_problems_drop_variables(K):
    """Issue figures: 4, 8, 10, 5 and 2 of 128 samples with a drop; at least one is what the GPU test needs."""
    V, D, R = wm.route_problem(K)
    assert V.shape == (K + 6, 64) and np.array_equal(R * 256, np.rint(R * 256)) and D.min() >= 1 and D.max() <= 8
    with_drop = 0
    for target in ("v", "dv"):
        for A, b in wm.route_systems(V, D, R, target):
            e = wm.active_set_events(A, b)
            assert e.status == 0
            with_drop += e.drops > 0
    print(f"route K={K}: {with_drop} of 128 samples drop a variable")
    assert with_drop >= 1


# the shapes tests/test_gpu_wls.py had before tests/test_gpu_wls_exact.py: (N, S, n_c, n_u[, depth])
OLD_SHAPES = [(4096, 7, 6, 2), (1000, 5, 12, 4), (3000, 9, 25, 0), (777, 4, 3, 1, 5), (33, 3, 2, 1), (2048, 65, 6, 2),
              (2048, 130, 6, 2), (4096, 4, 48, 0), (4096, 4, 60, 4), (2048, 8, 6, 2)]


def _count(V, D, R):
    tot = dict(entries=0, rejections=0, drops=0)
    for target in ("v", "dv"):
        for A, b in wm.route_systems(V, D, R, target):
            e = wm.active_set_events(A, b)
            assert e.status == 0
            for k in tot:
                tot[k] += getattr(e, k)
    return tot


@pytest.mark.parametrize("shape", OLD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_older_shapes_never_step_back(shape):
    """The finding this suite answers: on every shape of tests/test_gpu_wls.py each sample is solved by entering variables
    one after another -- no candidate is rejected and no variable ever leaves."""
    from test_gpu_wls import draw_u

    N, S, n_c, n_u = shape[:4]
    V, D, Rt = osol.synthetic_problem(N, S, n_c, n_u, **({"depth": shape[4]} if len(shape) > 4 else {}))
    R = np.c_[Rt, draw_u(N, n_u)] if n_u else Rt
    tot = _count(V, D, R)
    print(shape, tot)
    assert tot["entries"] > 0 and tot["drops"] == 0 and tot["rejections"] == 0


def test_the_toy_fixture_never_steps_back(toy):
    V, D, ref, _ = toy
    tot = _count(V, D, ref)
    assert tot["entries"] > 0 and tot["drops"] == 0 and tot["rejections"] == 0


# ------------------------------------------------------------------------------------------------ the moments' cases
def test_moment_table_covers_every_value_in_every_form_and_target():
    cases = wm.MOMENT_CASES
    assert 30 <= len(cases) <= 80
    assert all(wm.moment_case_allowed(c) or c == cases[0] for c in cases)
    assert cases[0][:4] == (16385, 129, 48, 16)  # the largest input
    for form in wm.MOMENT_FORMS:
        mine = [c for c in cases if c.form == form]
        assert {c.target for c in mine} == {"v", "dv"}
        assert {c.N for c in mine} == set(wm.MOMENT_N)
        assert {c.hole for c in mine} == {False, True}
        splits = {(c.n_c, c.n_u) for c in mine}
        want_s = set(wm.MOMENT_S) - ({1} if form != "f64_plain" else set())
        assert {c.S for c in mine} == want_s
        assert splits == {sp for sp in wm.MOMENT_SPLITS if form == "f64_plain" or sp[0] <= 48}
    for target in ("v", "dv"):
        mine = [c for c in cases if c.target == target]
        assert {c.N for c in mine} == set(wm.MOMENT_N) and {c.S for c in mine} == set(wm.MOMENT_S)
        assert {(c.n_c, c.n_u) for c in mine} == set(wm.MOMENT_SPLITS)
    # the slice boundaries, the second and third trip
    assert {c.n_c + c.n_u for c in cases} >= {1, 15, 16, 17, 32, 33, 48, 49, 64}
    assert wm.moments_trips(8192) == 1 and wm.moments_trips(8193) == 2 and wm.moments_trips(16385) == 3
    assert wm.moments_grid(15) == 1 and wm.moments_grid(17) == 2 and wm.moments_grid(8191) == 512


@pytest.mark.parametrize("c", wm.MOMENT_CASES, ids=wm.moment_case_id)
def test_dyadic_family_is_exact(c):
    """The precondition of the `==` comparisons: the largest entry of the table, in units of 2^-8, is below 2^53 (all
    terms are non-negative, so no partial sum in any order exceeds it), and the data are what the docstring says."""
    V, D, Rt, u = wm.dyadic_moment_data(c)
    R = wm.full_R(Rt, u)
    assert R.shape == (c.N, c.n_c + c.n_u) and np.array_equal(R * 256, np.rint(R * 256))
    assert R.max() == 1.0 and (R.min() == 0.0 or c.N == 1) and (D.sum(axis=0) > 0).all()
    assert np.array_equal(V * D, np.rint(V * D)) and (V >= 0).all() and (V <= 1).all()
    if c.hole:
        assert (D.sum(axis=1) == 0).sum() >= 1
    if c.form == "f64_plain" and c.S >= 2 and c.n_c <= 48:
        assert D.max() > 65535
    else:
        assert D.max() <= 256
    for target in ("v", "dv"):
        room = wm.dyadic_headroom(V, D, R, target)
        assert room > 0, room
    m = wm.exact_moments(V, D, R, c.target)
    assert m.exact
    # the integer table against an extended-precision sum of the same terms
    K = R.shape[1]
    ld = np.longdouble
    wt = (D * (D * V) if c.target == "dv" else D * V).astype(ld)
    assert np.array_equal(m.table[2 * K + 1].astype(ld), wt.sum(axis=0))
    assert np.array_equal(m.table[K].astype(ld), (R[:, :1].astype(ld) * wt).sum(axis=0))


def test_general_moments_reference_and_bound():
    c = wm.GENERAL_MOMENT_CASES[0]
    V, D, Rt, u = wm.general_moment_data(c)
    R = wm.full_R(Rt, u)
    m = wm.exact_moments(V, D, R, c.target)
    assert not m.exact and m.table.dtype == np.longdouble
    plain = np.vstack([R.T @ D, R.T @ (D * D * V), D.sum(axis=0, keepdims=True), (D * D * V).sum(axis=0, keepdims=True)])
    assert wm.moment_ratio(plain, m, c.N) <= 1.0      # a float64 matrix product sits inside the bound ...
    assert wm.moment_ratio(plain * (1 + 2.0 ** -45), m, c.N) > 1.0   # ... and a relative 3e-14 does not
    assert wm.moment_terms(16385) == 12 + 3 + 128 + 3 and wm.moment_terms(3) == 4 + 3 + 1 + 3


# ------------------------------------------------------------------------------------------------ the interface
def test_entry_points_are_declared_bound_and_exported():
    from demethify_amd import _build, _lib

    _build.build()
    header = (ROOT / "include" / "demethify_hip.h").read_text()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("dmf_wls_moments", "dmf_nnls_normal"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert len(_lib.SIGNATURES["dmf_wls_moments"][1]) == 7 and len(_lib.SIGNATURES["dmf_nnls_normal"][1]) == 7
    assert _lib.SIGNATURES["dmf_wls_moments"][1][:6] == _lib.SIGNATURES["dmf_wls_intercept"][1][:6]
    assert _lib.load().dmf_abi_version() == 1  # additive: no signature changed


def test_argument_checks_need_no_device():
    from demethify_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 16)()
    st = (ctypes.c_int * 4)()
    bad, unsupported = _lib.DMF_ERR_BAD_ARG, _lib.DMF_ERR_UNSUPPORTED
    assert lib.dmf_wls_moments(None, None, None, 0, 0, 0, buf) == bad
    assert lib.dmf_wls_moments(None, None, None, 0, 0, 0, None) == bad
    assert lib.dmf_nnls_normal(None, buf, buf, 1, 1, buf, st) == bad            # no context
    assert lib.dmf_nnls_normal(None, None, buf, 1, 1, buf, st) == bad
    assert lib.dmf_nnls_normal(None, buf, None, 1, 1, buf, st) == bad
    assert lib.dmf_nnls_normal(None, buf, buf, 1, 1, None, st) == bad
    assert lib.dmf_nnls_normal(None, buf, buf, 1, 1, buf, None) == bad
    assert lib.dmf_nnls_normal(None, buf, buf, 0, 1, buf, st) == bad            # K = 0
    assert lib.dmf_nnls_normal(None, buf, buf, 1, 0, buf, st) == bad            # S = 0
    assert lib.dmf_nnls_normal(None, buf, buf, 65, 1, buf, st) == unsupported   # K = 65: before the context is looked at
    assert lib.dmf_nnls_normal(None, buf, buf, 64, 1, buf, st) == bad           # K = 64 passes that check


def test_wrapper_packs_a_symmetric_gram():
    from demethify_amd.device import Context

    calls = []

    class Lib:
        def dmf_nnls_normal(self, h, gb, mom, K, S, out, status):
            n = K * (K + 1) // 2 * S
            calls.append((np.ctypeslib.as_array(ctypes.cast(gb, ctypes.POINTER(ctypes.c_double)), (n,)).copy(), K, S))
            return 0

    fake = Context.__new__(Context)
    fake._lib, fake._h = Lib(), None
    rs = np.random.RandomState(0)
    G = rs.uniform(size=(3, 4, 4))
    G = G + G.transpose(0, 2, 1)
    mom = np.zeros((10, 3))
    out, status = Context.nnls_normal(fake, G, mom)
    gb, K, S = calls[0]
    assert (K, S) == (4, 3) and np.isnan(out).all() and (status == -1).all()
    gb = gb.reshape(10, 3)
    for j in range(4):
        for i in range(j + 1):
            assert np.array_equal(gb[j * (j + 1) // 2 + i], G[:, i, j])
    Context.nnls_normal(fake, gb, mom)
    assert np.array_equal(calls[1][0].reshape(10, 3), gb)
    with pytest.raises(ValueError):
        Context.nnls_normal(fake, G + np.triu(np.ones((4, 4)), 1), mom)
    with pytest.raises(ValueError):
        Context.nnls_normal(fake, G[:, :3, :3], mom)
    fake._h = None
