"""Every instance of the streaming-cost kernels (k_cost_cols, k_cost_cols2, k_cost: csrc/dmf_kernels_stream.hip) against
exact integer sums.  The data of tests/cost_exact.py are dyadic, so every intermediate of every kernel is exactly
representable and cost * 2^20 is an integer that depends on the data alone (the helper's docstring has the argument): each
case first asserts the kernel it runs (Problem.cost_describe) and then EQUALITY with that integer, through the C-ABI.  No
tolerance appears in this file."""
import functools

import numpy as np
import pytest

import cost_exact as ce

pytestmark = pytest.mark.gpu

UNITS = ce.UNITS


def _id(c):
    return f"{c.expect[5:]}-{c.N}x{c.S}-{c.n_c}+{c.n_u}-d{c.dmax}" + ("-quarter" if c.count_scale != 1 else "") + \
        (f"-level{c.level}" if c.level else "")


@functools.lru_cache(maxsize=None)
def _data(N, S, n_c, n_u, dmax, seed, scale=1):
    c = ce.exact_case(N, S, n_c, n_u, dmax, seed, scale)
    for a in c:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def _check(ctx, case):
    """The case's problem, created at its level: the kernel the table names, the integer; and for a problem with u16 counts
    the same integer from the f64 copy through the any-shape kernel of level 1."""
    from demethify_amd.device import Problem

    c = ce.exact_case(case.N, case.S, case.n_c, case.n_u, case.dmax, case.seed, case.count_scale)
    unit = UNITS * case.count_scale
    ctx.set_generic(case.level)
    try:
        with Problem(ctx, c.V, c.D, c.Rt) as p:
            assert p.cost_describe(case.n_u) == case.expect
            got = p.cost(c.u, c.alpha)
            print(f"{case.expect}: got {got * unit!r} want {c.want}")
            assert got * unit == c.want
            if ce.has_u16(case):
                ctx.set_generic(1)
                assert p.cost_describe(case.n_u).startswith("cost=k_cost alpha=")
                assert p.cost(c.u, c.alpha) * unit == c.want
    finally:
        ctx.set_generic(0)


@pytest.mark.parametrize("case", ce.instance_cases(), ids=_id)
def test_every_column_instance(ctx, case):
    _check(ctx, case)


@pytest.mark.parametrize("case", ce.generic_cases(), ids=_id)
def test_any_shape_kernel(ctx, case):
    _check(ctx, case)


@pytest.mark.parametrize("case", ce.grid_cap_cases(), ids=_id)
def test_row_loop_takes_a_second_trip(ctx, case):
    _check(ctx, case)


def test_more_partial_columns_than_the_scratch_holds(ctx):
    """S = 65600: ceil(S / 64) = 1025 partial columns do not fit the 1024 partials, the plan names k_cost (the column
    kernel's launcher used to cap its grid at 1024 / 1025 = 0 row blocks and dmf_cost returned DMF_ERR_HIP)."""
    _check(ctx, ce.WIDE_S_CASE)


@pytest.mark.parametrize("S,nkc", [(S, nkc) for S in (127, 129) for nkc in (1, 2, 3, 4)])
def test_reference_mode_without_unknown_types(ctx, S, nkc):
    """n_u = 0, as deconvolution.py:43 calls it: Problem.cost(None, alpha)."""
    from demethify_amd.device import Problem

    n_c = 4 * nkc - (nkc & 1)
    c = _data(33, S, n_c, 0, 127, 5000 + S + nkc)
    with Problem(ctx, c.V, c.D, c.Rt) as p:
        assert p.cost_describe(0) == (f"cost=k_cost_cols<{nkc},0,u16>" if S < 128 else f"cost=k_cost_cols2<{nkc},0,odd>")
        assert c.u is None and p.cost(None, c.alpha) * UNITS == c.want


# ---------------------------------------------------------------------------------------------- derived problems
DERIVED = [(N, S, n_u) for N, S in ((77, 13), (96, 129), (257, 130)) for n_u in (2, 5)]


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("N,S,n_u", DERIVED)
def test_gathered_and_masked_problems(ctx, N, S, n_u, level):
    """A host-index and a device-index gather (repeated rows) against the integer of the fancy-indexed arrays, a masked problem
    against the integer of Di * mask: at level 0 the u16 copy derived on the device is read, at level 1 the f64 copy."""
    from demethify_amd.device import Problem
    from demethify_amd.staging import indices_to_device

    n_c = 2
    c = _data(N, S, n_c, n_u, 32639, 6000 + N + n_u)
    rs = np.random.RandomState(N + S)
    idx = rs.randint(0, N, size=N + 3)
    idx[:4] = (N - 1, 0, N - 1, N - 1)  # repeated rows, the last one among them
    mask = rs.rand(N, S) < 0.6
    mask[N - 1, S - 1] = True
    mask[:, S - 2] = False
    want_gather = ce.exact_sum(c.Di[idx], c.Vi[idx], c.Ri[idx], c.Ai)
    want_mask = ce.exact_sum(c.Di, c.Vi, c.Ri, c.Ai, weights=mask)
    assert len({want_gather, want_mask, c.want}) == 3
    expect = ce.expected_describe(S, n_c, n_u, level == 0, level)
    ctx.set_generic(level)
    try:
        with Problem(ctx, c.V, c.D, c.Rt) as p:
            assert p.cost_describe(n_u) == expect and p.cost(c.u, c.alpha) * UNITS == c.want
            with p.gather(idx) as q:
                assert q.cost_describe(n_u) == expect
                assert q.cost(c.u[idx], c.alpha) * UNITS == want_gather
            with p.gather(indices_to_device(idx, ctx)) as q:
                assert q.cost_describe(n_u) == expect
                assert q.cost(c.u[idx], c.alpha) * UNITS == want_gather
            with p.masked(mask) as q:
                assert q.cost_describe(n_u) == expect
                assert q.cost(c.u, c.alpha) * UNITS == want_mask
    finally:
        ctx.set_generic(0)


# ---------------------------------------------------------------------------------------------- solvers: hold-out error, resident iterate
def _masks(N, S, seed):
    rs = np.random.RandomState(seed)
    some = rs.rand(N, S) < 0.3
    some[1, :] = False
    some[N - 1, S - 1] = False
    last_sample = np.ones((N, S), dtype=bool)
    last_sample[:, S - 1] = False
    return {"some": some, "all_kept": np.ones((N, S), dtype=bool), "last_sample": last_sample}


@pytest.mark.parametrize("N,S,n_c,n_u,expect", [
    (96, 129, 2, 2, "cost=k_cost_cols2<1,2,odd>"),  # u16 weights: the lone lane reads the weights' padding
    (67, 131, 3, 6, "cost=k_cost_cols2<1,6,odd>"),  # ... in the wide form
    (40, 20, 1, 5, ce.LDS),                         # integer copies, but the any-shape k_cost: f64 weights on demand
])
def test_holdout_error_is_the_integer_sum_of_squares(ctx, N, S, n_c, n_u, expect):
    from demethify_amd.device import Problem, Solver

    c = _data(N, S, n_c, n_u, 127, 7000 + N)
    ones = np.ones_like(c.Di)
    with Problem(ctx, c.V, c.D, c.Rt) as full:
        assert full.cost_describe(n_u) == expect
        for name, mask in _masks(N, S, N + S).items():
            want = ce.exact_sum(ones, c.Vi, c.Ri, c.Ai, weights=~mask)
            with full.masked(mask) as held, Solver(held, c.u, c.alpha) as s:  # the dyadic iterate, zero steps
                assert held.cost_describe(n_u) == expect
                sum_sq, n_test = s.holdout_error(full)
                print(f"{name}: {sum_sq * UNITS!r} want {want} n_test {n_test}")
                assert n_test == int((~mask).sum())
                assert sum_sq * UNITS == want
                assert (want == 0) == (name == "all_kept")
                # the masked problem's own cost, from the resident iterate
                assert s.direct_cost() * UNITS == ce.exact_sum(c.Di, c.Vi, c.Ri, c.Ai, weights=mask)


@pytest.mark.parametrize("N,S,n_c,n_u,expect", [
    (96, 129, 4, 2, "cost=k_cost_cols2<1,2,odd>"), (64, 64, 8, 5, "cost=k_cost_cols2<2,5,even>"), (40, 20, 1, 5, ce.LDS),
])
def test_resident_iterate(ctx, N, S, n_c, n_u, expect):
    """Solver.direct_cost() and cost_begin() / cost_end() on a zero-step solver: the same integer as Problem.cost."""
    from demethify_amd.device import Problem, Solver

    c = _data(N, S, n_c, n_u, 32639, 8000 + N)
    with Problem(ctx, c.V, c.D, c.Rt) as p, Solver(p, c.u, c.alpha) as s:
        assert p.cost_describe(n_u) == expect
        assert p.cost(c.u, c.alpha) * UNITS == c.want
        assert s.direct_cost() * UNITS == c.want
        s.cost_begin()
        assert s.cost_end() * UNITS == c.want
        assert s.get_cost()[0] * UNITS == c.want  # (no iteration has run: the streaming cost of the starting point)


# ---------------------------------------------------------------------------------------------- device arrays 8 bytes off
@pytest.mark.parametrize("N,S,n_c,n_u", [(96, 128, 4, 2), (96, 129, 4, 2), (64, 64, 8, 5)])
def test_device_arrays_8_bytes_off_a_16_byte_boundary(ctx, N, S, n_c, n_u):
    """V, f64 counts and R_trunc as contiguous device views that start 8 bytes off a 16-byte boundary: the same kernel as for
    aligned arrays (the two-sample kernels take 16-byte loads from 8-byte-aligned rows) and the same integer."""
    import torch

    from demethify_amd.device import Problem

    c = _data(N, S, n_c, n_u, 127, 9000 + S)

    def on_device(a, off):
        flat = torch.zeros(a.size + 2, dtype=torch.float64, device=f"cuda:{ctx.device}")
        assert flat.data_ptr() % 16 == 0
        view = flat[off:off + a.size].view(*a.shape)
        view.copy_(torch.from_numpy(np.array(a, dtype=np.float64)))
        assert view.is_contiguous() and view.data_ptr() % 16 == 8 * off
        return view

    got = {}
    for off in (0, 1):
        V, D, Rt = (on_device(a, off) for a in (c.V, c.D, c.Rt))
        with Problem(ctx, V, D, Rt) as p:
            got[off] = (p.cost_describe(n_u), p.cost(c.u, c.alpha) * UNITS)
    assert got[0] == (ce.expected_describe(S, n_c, n_u, True, 0), c.want)
    assert got[1] == got[0]
