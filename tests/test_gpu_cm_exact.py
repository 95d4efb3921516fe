"""k_cm_i8's per-row moments read back (Solver.row_moments) and held to exact values: M_i bit for bit against the model of
tests/cm_exact.py on both data families, c_i equal to the one right answer on the dyadic family and inside the derived
bound on the full-mantissa one, for every template instance and every launch-time split (tests/test_cm_exact_host.py proves
the table's coverage without a GPU).  Every case first asserts the launch plan on the LIVE solver -- what the accessor says it
ran, and dmf_solver_u_phase_describe -- then the numbers.  The same accessor on the FP64 producer: every split-mode
k_u_phase_mfma instance of tests/fp64_rowpass.py on dyadic data, c and M equal to the exact values.

Each full-family case prints "DEV c <ratio>": the largest |c - reference| over the derived limit (cm_exact.c_ratio)."""
import numpy as np
import pytest

import cm_exact as cm
import fp64_rowpass as fr

pytestmark = pytest.mark.gpu


def _bits_equal(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return got.shape == want.shape and got.tobytes() == want.tobytes()


def _first_difference(got, want):
    bad = np.argwhere(got != want)
    i, p = (int(x) for x in bad[0])
    return f"{len(bad)} entries differ; first at row {i}, column {p}: got {got[i, p]!r}, want {want[i, p]!r}"


def _moments(ctx, c, d):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    u0 = np.random.RandomState(3).rand(c.N, c.n_u)
    mode = L.DMF_MODE_PARTIAL if c.n_c else L.DMF_MODE_UNSUPERVISED
    with Problem(ctx, d.V, d.D, d.Rt) as p, Solver(p, u0, d.alpha, mode) as s:
        assert s.u_phase_describe(20, "update_u") == cm.u_phase_text(c.N, c.S, c.n_c, c.n_u, c.nd)
        got, text = s.row_moments()
    assert text == cm.plan_text(c.N, c.S, c.n_c, c.n_u, c.nd)
    return got[:, :c.n_u], got[:, c.n_u:]


@pytest.mark.parametrize("family", ["dyadic", "full"])
@pytest.mark.parametrize("case", cm.all_cases(), ids=cm.cid)
def test_row_moments_of_k_cm_i8(ctx, case, family):
    c = case
    d = cm.make(c, family)
    got_c, got_M = _moments(ctx, c, d)
    want_M = cm.model_M(d.alpha[c.n_c:], d.Di)
    assert np.isfinite(got_M).all() and np.isfinite(got_c).all()
    assert _bits_equal(got_M, want_M), _first_difference(got_M, want_M)
    if family == "dyadic":
        exact_M, exact_c = cm.dyadic_M(c, d), cm.dyadic_c(c, d)
        assert _bits_equal(got_M, exact_M), _first_difference(got_M, exact_M)   # the digit model IS the mathematics here
        assert _bits_equal(got_c, exact_c), _first_difference(got_c, exact_c)
    else:
        ratio = cm.c_ratio(c, d, got_c)
        print(f"DEV c {ratio:.3e} n={cm.c_operations(c)} {cm.cid(c)}")
        assert ratio <= 1.0, (cm.cid(c), ratio)
    if c.N >= 3:   # zero coverage: nothing at all, not a rounding residue
        assert not got_M[c.N // 2].any() and not got_c[c.N // 2].any()


# ------------------------------------------------------------------------------------------------ the accessor itself
def _small(family="full"):
    c = cm.Case(70, 130, 5, 6, 1, "", "")
    return c, cm.make(c, family)


def test_row_moments_leave_the_iterate_and_later_steps_alone(ctx):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    c, d = _small()
    rs = np.random.RandomState(5)
    u0 = rs.rand(c.N, c.n_u)
    a0 = rs.dirichlet(np.ones(c.n_c + c.n_u), c.S).T.copy()
    outs = []
    with Problem(ctx, d.V, d.D, d.Rt) as p:
        for peek in (False, True):
            with Solver(p, u0, a0, L.DMF_MODE_PARTIAL) as s:
                s.step(2, 20, 0.0)
                if peek:
                    before = s.get()
                    first = s.row_moments()
                    again = s.row_moments()
                    after = s.get()
                    assert _bits_equal(first[0], again[0]) and first[1] == again[1]
                    assert _bits_equal(before[0], after[0]) and _bits_equal(before[1], after[1])
                    # ... and they are the moments of the alpha the solver holds NOW
                    want = cm.model_M(after[1][c.n_c:], d.Di)
                    assert _bits_equal(first[0][:, c.n_u:], want)
                s.step(2, 20, 0.0)
                outs.append(s.get())
    assert _bits_equal(outs[0][0], outs[1][0]) and _bits_equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]


def test_a_stopped_solver_is_refused(ctx):
    """Once the stop test has fired the producers return at once: the accessor answers an error, not the scratch of an
    earlier iteration."""
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    c, d = _small()
    u0 = np.random.RandomState(5).rand(c.N, c.n_u)
    with Problem(ctx, d.V, d.D, d.Rt) as p, Solver(p, u0, d.alpha, L.DMF_MODE_PARTIAL) as s:
        s.row_moments()                       # (fills the scratch)
        _, converged = s.step(3, 20, 1e300)   # every difference is below this threshold: stops after the first iteration
        assert converged
        with pytest.raises(L.DemethifyHipError) as e:
            s.row_moments()
        assert e.value.status == L.DMF_ERR_BAD_ARG


def test_routes_without_row_moments_are_unsupported(ctx):
    """Level 3 with 12 unknowns runs k_u_phase_big, which keeps c_i / M_i in its registers; level 1 k_u_phase_gram."""
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    c = cm.Case(70, 8, 2, 12, 1, "", "")
    d = cm.make(c, "full")
    u0 = np.random.RandomState(5).rand(c.N, c.n_u)
    before = ctx.generic_level
    try:
        for level, kernel in ((3, "k_u_phase_big<"), (1, "k_u_phase_gram<")):
            ctx.set_generic(level)
            with Problem(ctx, d.V, d.D, d.Rt) as p, Solver(p, u0, d.alpha, L.DMF_MODE_PARTIAL) as s:
                assert s.u_phase_describe(51, "update_u").startswith(kernel)
                with pytest.raises(L.DemethifyHipError) as e:
                    s.row_moments()
                assert e.value.status == L.DMF_ERR_UNSUPPORTED
    finally:
        ctx.set_generic(before)
    lib, out = L.load(), np.zeros(4)
    assert lib.dmf_solver_row_moments(None, out.ctypes.data, None, 0) == L.DMF_ERR_BAD_ARG


# ------------------------------------------------------------------------------------------------ the FP64 split producer
SPLIT_CASES = [c for nkc in range(5) for n_u in range(1, 9) for form in fr.FORMS for c in [fr.mfma_case(nkc, n_u, form, "split")]]


def _split_data(c):
    """Dyadic data of a split-mode k_u_phase_mfma case: multiples of 2^-6, counts integers or -- where the case asks for
    fractional counts -- integers + 1/2, one alpha entry at 1.25 where the case wants alpha outside [0, 1].  -> (V, D, Rt,
    alpha, c exactly, M exactly): units of 2^-19 and 2^-13 with twice the counts as integers."""
    rs = np.random.RandomState(11 + 31 * c.n_c + c.n_u + c.S)
    K = c.n_c + c.n_u
    Vi = rs.randint(0, 65, size=(c.N, c.S)).astype(np.int64)
    Ri = rs.randint(0, 65, size=(c.N, c.n_c)).astype(np.int64)
    Ai = rs.randint(0, 65, size=(K, c.S)).astype(np.int64)
    D2 = 2 * rs.randint(0, 128, size=(c.N, c.S)).astype(np.int64)
    D2[rs.rand(c.N, c.S) < 0.1] = 0
    D2[c.N // 2] = 0
    D2[0, 0], D2[c.N - 1, c.S - 1] = 2 * 127, 2 * 127
    if not c.ints:
        D2 += 1
    if c.alpha_out:
        Ai[0, 0] = 80
    E = 64 * Vi - (Ri @ Ai[:c.n_c] if c.n_c else 0)
    ci = (D2 * E) @ Ai[c.n_c:].T
    J, Lq = cm.pair_index(c.n_u)
    mi = D2 @ (Ai[c.n_c:][J] * Ai[c.n_c:][Lq]).T
    assert int(np.abs(ci).max()) < (1 << 53) and int(mi.max()) < (1 << 53)
    return (Vi / 64.0, D2 / 2.0, (Ri / 64.0) if c.n_c else None, Ai / 64.0, np.ldexp(ci.astype(np.float64), -19),
            np.ldexp(mi.astype(np.float64), -13))


@pytest.mark.parametrize("case", SPLIT_CASES, ids=fr.uid)
def test_row_moments_of_the_fp64_split_producer(ctx, case):
    """All 120 k_u_phase_mfma instances in split mode: c and M equal the exact values on dyadic data."""
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    c = case
    V, D, Rt, alpha, want_c, want_M = _split_data(c)
    u0 = np.random.RandomState(3).rand(c.N, c.n_u)
    before = ctx.generic_level
    ctx.set_generic(c.level)
    try:
        with Problem(ctx, V, D, Rt) as p, Solver(p, u0, alpha, L.DMF_MODE_PARTIAL if c.n_c else L.DMF_MODE_UNSUPERVISED) as s:
            got, text = s.row_moments()
            assert text == s.u_phase_describe(fr.SPLIT_STEPS, "update_u")
    finally:
        ctx.set_generic(before)
    assert text == fr.mfma_text(c.N, c.S, c.n_c, c.n_u, fr.SPLIT_STEPS, fr.nd_of(c) > 0, True)
    assert _bits_equal(got[:, :c.n_u], want_c), _first_difference(got[:, :c.n_u], want_c)
    assert _bits_equal(got[:, c.n_u:], want_M), _first_difference(got[:, c.n_u:], want_M)
