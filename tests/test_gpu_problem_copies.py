"""Every copy and constant that a problem builder leaves on the device, read back (Problem.report, Problem.copy_out) and held
to tests/problem_model.py: dmf_problem_create, dmf_problem_gather with host and with device indices, dmf_problem_mask, and
the derived problems of derived problems.  Compared: V, D, R_trunc, its padded copy, the u16 counts D16, the methylated read
counts X16, the hold-out weights W16, the digit planes Dt8 (every plane, every padding row), the mask bits, the six
constants on the host and on the device, ND / SD / N16 / plane_stride, x16_dev, x16_sum, n_test, d_f32_exact -- and that an
array the model says is absent IS absent.

Everything is equality.  Two tolerances appear, both named in the places they are used: ||R_trunc||_F^2 off the 2^-10 grid
is held to (N n_c + 4) 2^-53 relative to the exact rational sum (problem_model.rt_sumsq_ok; the worst case of one rounded
square and N n_c additions of non-negative terms in any order), and a solve whose derived problem keeps two digit planes
where the re-created one has one is held to 1e-10 against it (see test_resample_that_loses_the_maximum).

tests/test_problem_model_host.py proves, from the shapes, what each case of the table reaches.  Every test prints what it
compared -- per array the number of differing elements and the first of them -- before it asserts."""
import contextlib
import functools
import time

import numpy as np
import pytest

import gram_exact as ge
import problem_model as pm

from conftest import rel_err

pytestmark = pytest.mark.gpu

DIGIT_CHANGE_RTOL = 1e-10   # the bar of test_gpu_holdout.py::test_mask_that_removes_the_second_count_digit, for its reason


# ---------------------------------------------------------------------------------------------- reading a problem back
def _read(p):
    """-> (report, {array name: array or None}); asking for an array the report says is absent must be DMF_ERR_BAD_ARG."""
    from demethify_amd import _lib as L

    rep = p.report()
    has = {"V": True, "D": True, "Rt": rep["n_c"] > 0, "Rtp": rep["rtp_width"] > 0, "D16": rep["has_D16"], "X16": rep["has_X16"],
           "W16": rep["has_W16"], "Dt8": rep["has_Dt8"], "mask_bits": rep["has_mask_bits"], "consts": True}
    assert set(has) == set(L.PROBLEM_ARRAYS)
    arrays = {}
    for name, present in has.items():
        if present:
            arrays[name] = p.copy_out(name, rep)
        else:
            with pytest.raises(L.DemethifyHipError) as e:
                p.copy_out(name, rep)
            assert e.value.status == L.DMF_ERR_BAD_ARG, (name, e.value.status)
            arrays[name] = None
    return rep, arrays


def _check(name, p, model):
    rep, arrays = _read(p)
    pm.compare(name, rep, arrays, model)
    return rep, arrays


class _settings:
    """The context's X16 switch and kernel-selection level for the problems created inside; both put back on the way out."""

    def __init__(self, ctx, x16=True, level=0):
        self.ctx, self.x16, self.level = ctx, x16, level

    def __enter__(self):
        self.before = self.ctx.generic_level
        self.ctx.set_generic(self.level)
        self.ctx.set_x16(self.x16)

    def __exit__(self, *exc):
        self.ctx.set_generic(self.before)
        self.ctx.set_x16(True)


def _routes(ctx, name, V, D, Rt, idx, mask, x16=True, level=0, nested=False, expect=None):
    """Created, gathered by host indices, gathered by device indices, masked -- and, nested, gathered from gathered and masked
    from gathered -- each read back and compared.  expect: a function of the models {route: model} for what the case claims.
    -> {route: (report, arrays)} of created / gathered / masked."""
    from demethify_amd.device import Problem
    from demethify_amd.staging import indices_to_device

    t0 = time.time()
    models = {"created": pm.created(V, D, Rt, x16=x16, level=level)}
    models["gathered"] = pm.gathered(models["created"], idx, x16=x16, level=level)
    models["masked"] = pm.masked(models["created"], mask, x16=x16, level=level)
    if expect is not None:
        expect(models)
    t1 = time.time()
    got = {}
    with _settings(ctx, x16, level):
        with Problem(ctx, V, D, Rt) as src:
            got["created"] = _check(f"{name} created", src, models["created"])
            with src.gather(idx) as g:
                got["gathered"] = _check(f"{name} gathered (host indices)", g, models["gathered"])
                if nested:
                    rs = np.random.RandomState(len(idx))
                    idx2 = rs.randint(0, len(idx), size=len(idx) + 5)
                    mask2 = rs.rand(len(idx), V.shape[1]) < 0.5
                    with g.gather(idx2) as gg:
                        _check(f"{name} gathered from gathered", gg, pm.gathered(models["gathered"], idx2, x16=x16, level=level))
                    with g.masked(mask2) as gk:
                        _check(f"{name} masked from gathered", gk, pm.masked(models["gathered"], mask2, x16=x16, level=level))
            dev = indices_to_device(idx, ctx)
            with src.gather(dev) as g:
                _check(f"{name} gathered (device indices)", g, models["gathered"])
            dev.close()
            with src.masked(mask) as k:
                got["masked"] = _check(f"{name} masked", k, models["masked"])
    print(f"{name}: models {t1 - t0:.2f} s, device and comparison {time.time() - t1:.2f} s")
    return got


def _resample(N, n_idx, seed):
    return np.random.RandomState(seed).randint(0, N, size=n_idx).astype(np.int64)


def _mask(N, S, seed, kept=0.6):
    rs = np.random.RandomState(seed)
    mask = rs.rand(N, S) < kept
    mask[N // 2, :] = False      # one fully held-out row
    mask[:, S - 1] = False       # one fully held-out sample
    mask[0, :max(S - 1, 1)] = True
    return mask


# ---------------------------------------------------------------------------------------------- tails
@pytest.mark.parametrize("max_count", [100, 3000], ids=["one_digit", "two_digits"])
@pytest.mark.parametrize("c", pm.TAILS, ids=lambda c: f"{c.N}x{c.S}-{c.n_c}")
def test_tails_on_every_route(ctx, c, max_count):
    """Row tails of 16 and 32, one to ten sample blocks, every n_c % 4, no known types, no integer copies (S = 1), nothing to
    pad -- R_trunc on the grid with one digit (its norm is held to equality), full-mantissa with two (the bound)."""
    V, D, Rt = pm.true_data(c.N, c.S, c.n_c, 7 + c.N, max_count, rt_grid=max_count == 100, max_at=(c.N - 1, c.S - 1))

    def expect(m):
        ints = c.S >= 2
        for r in m.values():
            assert (r.D16 is not None) == ints and (r.X16 is not None) == ints and r.ND == ((1 if max_count == 100 else 2) if ints else 0)
        assert m["created"].rtp_borrows_rt == (c.n_c == 4) and (m["created"].Rtp is None) == (c.n_c == 0)

    _routes(ctx, f"tails {c.N}x{c.S}-{c.n_c}", V, D, Rt, _resample(c.N, c.N, 1), _mask(c.N, c.S, 2), nested=True, expect=expect)


# ---------------------------------------------------------------------------------------------- digits and thresholds
@pytest.mark.parametrize("max_count,nd", pm.THRESHOLDS)
def test_digit_thresholds(ctx, max_count, nd):
    """Maximum count 127, 128, 32639, 32640: ND and the presence of every copy as the model says.  From the 128 and the
    32639 sources, a gather that avoids the row holding every count above 127 and a mask that holds those elements out:
    ND = 2 is kept, kDmax <= 127, and the second digit plane is all zeros."""
    V, D, Rt, row = pm.planted_source(70, 40, 2, 6, 5, max_count)
    idx, mask = pm.avoiding(70, row, 70, 1), D <= 127

    def expect(m):
        assert m["created"].ND == nd and (m["created"].D16 is not None) == (nd > 0)

    got = _routes(ctx, f"max count {max_count}", V, D, Rt, idx, mask, expect=expect)
    assert got["created"][0]["ND"] == nd
    if nd == 2:
        for route in ("gathered", "masked"):
            rep, arrays = got[route]
            print(f"max count {max_count} {route}: ND {rep['ND']} kDmax {rep['kDmax']} plane 1 non-zero bytes "
                  f"{int(np.count_nonzero(arrays['Dt8'][1]))}")
            assert rep["ND"] == 2 and rep["kDmax"] <= 127 and not arrays["Dt8"][1].any() and arrays["Dt8"][0].any()


@pytest.mark.parametrize("what", ["fractional", "negative", "rt_above_one"])
def test_inputs_that_forbid_integer_copies(ctx, what):
    """One count 2.5, one count -1, one R_trunc entry 1 + 2^-52: no integer copies on any route, kIntCountMax = inf or
    kRtOutsideUnit = 1 -- carried by the mask, recomputed by the gather (whose rows may leave the offender out)."""
    V, D, Rt, row = pm.planted_source(70, 40, 2, 6, 5, 100)
    D = D.astype(np.float64)
    if what == "fractional":
        D[3, 3] = 2.5
    elif what == "negative":
        D[3, 3] = -1.0
    else:
        Rt = Rt.copy()
        Rt[3, 1] = 1.0 + 2.0 ** -52
    idx_with, idx_without = np.array([3, 3, 10, 69, 0]), pm.avoiding(70, 3, 90, 2)

    def expect(m):
        assert m["created"].ND == 0 and m["masked"].ND == 0 and m["created"].Rtp is not None
        assert (m["created"].consts["kIntCountMax"] == float("inf")) == (what != "rt_above_one")
        assert m["created"].consts["kRtOutsideUnit"] == float(what == "rt_above_one")

    got = _routes(ctx, f"{what}, offender gathered", V, D, Rt, idx_with, _mask(70, 40, 3), expect=expect)
    assert got["gathered"][0]["ND"] == 0 and got["created"][0]["has_D16"] == 0
    got = _routes(ctx, f"{what}, offender left out", V, D, Rt, idx_without, _mask(70, 40, 3))
    assert got["gathered"][0]["ND"] == 1 and got["gathered"][0]["has_D16"] == 1 and got["masked"][0]["ND"] == 0


# ---------------------------------------------------------------------------------------------- a resample that loses the maximum
def _solve(problem, u0, a0):
    """Three outer iterations as part A of tests/test_gpu_holdout.py runs them -> (describe, u, alpha, loop cost, streaming cost)."""
    from demethify_amd import _lib as L
    from demethify_amd.device import Solver

    with Solver(problem, u0, a0, L.DMF_MODE_PARTIAL) as s:
        desc = s.describe(20)
        s.step(3, 20, 0.0)
        u, alpha, cost, _ = s.get()
        return desc, u, alpha, cost, s.direct_cost()


@pytest.mark.parametrize("name,top,x16,nd_src,nd_again", pm.LOSE_MAX, ids=[c[0] for c in pm.LOSE_MAX])
def test_resample_that_loses_the_maximum(ctx, name, top, x16, nd_src, nd_again):
    """The largest count sits in one row that the resample never draws (tests/test_problem_model_host.py asserts it): kDmax
    and kIntCountMax are the rows', ND and the exactness flags the source's.  Then the solve of the gathered problem against
    the solve of Problem(V[idx], D[idx], Rt[idx]): the same kernels (describe), iterates and both costs bit for bit while
    the digit count is the same on both sides.  Where the gathered problem keeps two digit planes and the re-created one has
    one, both are exact integer arithmetic on the same counts, so they agree to 1e-10 instead of bit for bit -- which also
    pins max(D): the step lengths are 1 / (||.||^2 max(D)^2), and the source's maximum (300 against at most 60) would move
    the iterates by far more."""
    from demethify_amd.device import Problem

    N, S, n_c, n_u = 200, 64, 2, 2
    V, D, Rt, row = pm.planted_source(N, S, n_c, 21, 7, top)
    if not x16:
        V = np.round(V, 2)   # (two decimals: x / d no longer, X16 is rejected)
    idx = pm.avoiding(N, row, N, 4)

    def expect(m):
        assert (m["created"].ND, m["gathered"].ND) == (nd_src, nd_src) and (m["gathered"].X16 is not None) == x16
        assert m["gathered"].consts["kDmax"] == float(D[idx].max()) < m["created"].consts["kDmax"] == float(top)

    got = _routes(ctx, name, V, D, Rt, idx, D <= 60, expect=expect)
    assert got["gathered"][0]["kDmax"] == got["gathered"][0]["kIntCountMax"] == float(D[idx].max())
    rs = np.random.RandomState(3)
    u0, a0 = rs.uniform(size=(N, n_u)), rs.dirichlet(np.ones(n_c + n_u), S).T
    with Problem(ctx, V, D, Rt) as src, src.gather(idx) as g, Problem(ctx, V[idx], D[idx], Rt[idx]) as again:
        assert (g.report()["ND"], again.report()["ND"]) == (nd_src, nd_again)
        g_desc, g_u, g_alpha, g_cost, g_direct = _solve(g, u0, a0)
        a_desc, a_u, a_alpha, a_cost, a_direct = _solve(again, u0, a0)
    print(f"{name}: gathered [{g_desc}] re-created [{a_desc}]")
    print(f"{name}: u {rel_err(g_u, a_u):.3e} alpha {rel_err(g_alpha, a_alpha):.3e} cost {abs(g_cost - a_cost) / a_cost:.3e} "
          f"streaming cost {abs(g_direct - a_direct) / a_direct:.3e}")
    if nd_src == nd_again:
        assert g_desc == a_desc
        assert np.array_equal(g_u, a_u) and np.array_equal(g_alpha, a_alpha) and g_cost == a_cost and g_direct == a_direct
    else:
        assert rel_err(g_u, a_u) <= DIGIT_CHANGE_RTOL and rel_err(g_alpha, a_alpha) <= DIGIT_CHANGE_RTOL
        assert abs(g_cost - a_cost) <= DIGIT_CHANGE_RTOL * a_cost and abs(g_direct - a_direct) <= DIGIT_CHANGE_RTOL * a_direct


# ---------------------------------------------------------------------------------------------- n_idx != N
@functools.lru_cache(maxsize=1)
def _gather_source():
    N = pm.GATHER_SOURCE_N
    V, D, Rt = pm.true_data(N, 13, 3, 31, 300, rt_grid=False, max_at=(N - 1, 12))
    D[100:140] = 0       # forty rows without a single read
    V[100:140] = 0.5
    for a in (V, D, Rt):
        a.setflags(write=False)
    return V, D, Rt, pm.created(V, D, Rt)


def _index_sets():
    N = pm.GATHER_SOURCE_N
    sets = [(f"n_idx={n}", _resample(N, n, 40 + n)) for n in pm.GATHER_LENGTHS]
    sets.append(("every index equal", np.full(50, N - 1, dtype=np.int64)))
    sets.append(("the last row alone", np.array([N - 1], dtype=np.int64)))
    sets.append(("rows without reads", np.arange(100, 140, dtype=np.int64)[::-1].copy()))
    return sets


@pytest.mark.parametrize("which", range(len(_index_sets())), ids=[s[0].replace(" ", "_") for s in _index_sets()])
def test_gather_of_any_length(ctx, which):
    """From N = 1000: one row, 15, 16, 17, 31, 33 rows, N rows, 2500 rows, every index equal, and rows whose counts are all 0
    (kDmax = 0, every copy zero) -- N16, plane_stride, the zero rows and the tile count all follow n_idx.  Host and device
    indices.  Read back only."""
    from demethify_amd.device import Problem
    from demethify_amd.staging import indices_to_device

    name, idx = _index_sets()[which]
    V, D, Rt, src_m = _gather_source()
    want = pm.gathered(src_m, idx)
    with Problem(ctx, V, D, Rt) as src:
        with src.gather(idx) as g:
            rep, arrays = _check(f"{name} (host indices)", g, want)
        dev = indices_to_device(idx, ctx)
        with src.gather(dev) as g:
            _check(f"{name} (device indices)", g, want)
        dev.close()
    assert rep["N"] == len(idx) and rep["N16"] == (len(idx) + 15) // 16 * 16 and rep["ND"] == 2
    if name == "rows without reads":
        assert rep["kDmax"] == 0.0 and rep["kDsq"] == 0.0 and rep["x16_sum"] == 0.0
        assert not arrays["D16"].any() and not arrays["X16"].any() and not arrays["Dt8"].any()


def test_everything_held_out(ctx):
    """A mask that keeps nothing: every count copy zero, W16 one on the N x S elements and zero on the padding, kDmax = 0,
    n_test = N S, x16_dev still the source's.  Read back only."""
    from demethify_amd.device import Problem

    V, D, Rt, src_m = _gather_source()
    mask = np.zeros(V.shape, dtype=bool)
    with Problem(ctx, V, D, Rt) as src, src.masked(mask) as k:
        rep, arrays = _check("everything held out", k, pm.masked(src_m, mask))
    assert rep["kDmax"] == 0.0 and rep["n_test"] == V.size and int(arrays["W16"].sum()) == V.size
    assert not arrays["D16"].any() and not arrays["Dt8"].any() and rep["x16_dev"] == src_m.x16_dev


# ---------------------------------------------------------------------------------------------- X16
def _x16_base():
    V, D, Rt = pm.true_data(300, 37, 2, 12, 200, zero_fraction=0.0)
    D = np.maximum(D, 1)
    return np.rint(V * D) / D, D, Rt


X16_CASES = ["accepted", "perturbed", "non_integral", "x_above_d", "switched_off", "zero_count", "deviation_held_out"]


@pytest.mark.parametrize("what", X16_CASES)
def test_x16_on_every_route(ctx, what):
    """X16 accepted; rejected by each of the three planted elements of tests/test_gpu_x16.py (+1e-9, x + 0.3, x = d + 1);
    switched off by the context; d = 0 with v = 0.7 (x = 0, accepted); and a masked problem whose held-out elements carry all
    the deviation (x16_dev stays the source's: a bound over the source holds for any subset).  x16_sum and x16_dev exact on
    the created, the gathered and the masked problem."""
    V, D, Rt = _x16_base()
    N, S = V.shape
    mask, x16, accepted = _mask(N, S, 5), True, True
    if what == "perturbed":
        V[100, 7] += 1e-9
    elif what == "non_integral":
        V[5, 3] = (np.rint(V[5, 3] * D[5, 3]) + 0.3) / D[5, 3]
    elif what == "x_above_d":
        V[299, 36] = 1.0 + 1.0 / D[299, 36]
    elif what == "switched_off":
        x16 = False
    elif what == "zero_count":
        D[10, 11], V[10, 11] = 0, 0.7
    elif what == "deviation_held_out":
        D = 1 << np.random.RandomState(8).randint(0, 7, size=(N, S)).astype(np.int64)   # v = x / 2^k: no deviation at all ...
        V = np.floor(np.random.RandomState(9).rand(N, S) * (D + 1)) / D
        D[4, 5], V[4, 5] = 3, 1.0 / 3.0                                                # ... but here: |v d - 1| = 2^-54
        mask[4, 5] = False
    accepted = what in ("accepted", "zero_count", "deviation_held_out")

    def expect(m):
        for r in m.values():
            assert (r.X16 is not None) == accepted and r.D16 is not None
        if what == "deviation_held_out":
            again = pm.created(V * mask, D * mask, Rt)
            assert m["created"].x16_dev == m["masked"].x16_dev == 2.0 ** -54 and again.x16_dev == 0.0
        if what == "accepted":
            assert 0.0 < m["created"].x16_dev <= 2.0 ** -53

    got = _routes(ctx, f"x16 {what}", V, D, Rt, _resample(N, N + 30, 6), mask, x16=x16, expect=expect)
    for route, (rep, _) in got.items():
        print(f"x16 {what} {route}: has_X16 {rep['has_X16']} x16_dev {rep['x16_dev']!r} x16_sum {rep['x16_sum']!r}")
        assert rep["has_X16"] == int(accepted)


# ---------------------------------------------------------------------------------------------- recycled memory
def _poison(ctx, N, S, n_c, count):
    """A problem whose every device array is non-zero where it can be: counts `count`, V = 1, R_trunc = 1."""
    from demethify_amd.device import Problem

    return Problem(ctx, np.ones((N, S)), np.full((N, S), count, dtype=np.int64), np.ones((N, n_c)) if n_c else None)


@pytest.mark.parametrize("nd,count", [(1, 127), (2, 32639)], ids=["one_digit", "two_digits"])
def test_builders_write_their_padding_on_recycled_memory(ctx, nd, count):
    """DevBuf::alloc returns uninitialised memory, and the context keeps freed blocks of 1 MB and more by exact size (three per
    size) for the next allocation of that size.  At 8197 x 127 x 13 the u16 copies (8208 x 128 x 2 B), a digit plane
    (257 x 4 x 1024 B) and the padded R_trunc copy (8197 x 16 x 8 B) all reach that threshold
    (test_problem_model_host.py::test_recycled_case_reaches_the_keep_threshold), and each has padding: 11 rows and one
    sample, 27 digit rows, 3 columns.

    A  a poison problem of that shape (counts 127 or 32639, V = 1, R_trunc = 1) and its everything-held-out mask (W16 all
       ones) are created and closed; then the real case is created, gathered and masked and compared.
    B  a block freed by a problem of the SAME shape is zero exactly where the next problem's padding lies, so A alone would
       not notice a padding write that went missing.  With the real problems of A still holding their blocks, two problems
       each of 2052 x 128, 257 x 512 nd and 8197 x 16 are created and closed: their V and D (doubles 1.0 and `count`
       throughout) have the byte sizes of the u16 copies, of Dt8 and of the padded R_trunc copy.  The real problems are closed
       and the real case is built and compared again.

    No address leaves the library, so the test cannot prove that a block was reused; it makes sure that wherever the pool
    does recycle, the builders' padding writes meet non-zero memory."""
    from demethify_amd.device import Problem
    from demethify_amd.staging import indices_to_device

    c = pm.RECYCLED
    V, D, Rt = pm.grid_data(c.N, c.S, c.n_c, 17, max_count=count)
    idx, mask = _resample(c.N, c.N, 18), _mask(c.N, c.S, 19)
    t0 = time.time()
    src_m = pm.created(V, D, Rt)
    g_m, k_m = pm.gathered(src_m, idx), pm.masked(src_m, mask)
    assert src_m.ND == nd and src_m.X16 is not None
    sizes = pm.pool_sizes(c.N, c.S, c.n_c, nd)
    assert all(b >= pm.KEEP_MIN_BYTES for b in sizes.values())
    t1 = time.time()

    def build_and_compare(phase, stack):
        """-> the three problems, still open (every one is also closed by `stack`, whatever happens)"""
        src = stack.enter_context(Problem(ctx, V, D, Rt))
        _check(f"recycled {phase} created", src, src_m)
        dev = indices_to_device(idx, ctx)
        try:
            g = stack.enter_context(src.gather(dev))
        finally:
            dev.close()
        _check(f"recycled {phase} gathered", g, g_m)
        k = stack.enter_context(src.masked(mask))
        _check(f"recycled {phase} masked", k, k_m)
        return [k, g, src]

    with contextlib.ExitStack() as stack:
        # A
        poison = stack.enter_context(_poison(ctx, c.N, c.S, c.n_c, count))
        held_out = stack.enter_context(poison.masked(np.zeros((c.N, c.S), dtype=bool)))
        assert held_out.report()["n_test"] == c.N * c.S
        poison.close()     # (the source first: its non-zero D16 and X16 are kept, then the mask's W16 of ones fills the list)
        held_out.close()
        live = build_and_compare("A", stack)
        # B
        cross = []
        for N2, S2, size in ((2052, 128, sizes["D16 / X16 / W16"]), (257, 512 * nd, sizes["Dt8"]), (8197, 16, sizes["Rtp"])):
            assert N2 * S2 * 8 == size, (N2, S2, size)
            cross += [stack.enter_context(_poison(ctx, N2, S2, 0, count)) for _ in range(2)]
        for p in cross:
            p.close()
        for p in live:
            p.close()
        build_and_compare("B", stack)
    print(f"recycled nd={nd}: models {t1 - t0:.2f} s, device and comparison {time.time() - t1:.2f} s")


# ---------------------------------------------------------------------------------------------- grid-stride tails
@functools.lru_cache(maxsize=1)
def _big():
    c = pm.BIG
    V, D, Rt = pm.grid_data(c.N, c.S, c.n_c, 23)
    for a in (V, D, Rt):
        a.setflags(write=False)
    return V, D, Rt, pm.created(V, D, Rt)


def test_grid_stride_tails_created(ctx):
    """1,048,613 x 2 x 1: more workgroups asked for than the clamp of k_build_d16 (8192), k_build_dt8 (16384), k_pad_rows
    (8192), k_reduce_partial (1024, on D and on R_trunc) and k_convert_counts (8192: the counts go in as int64) allows --
    test_problem_model_host.py::test_big_case_exceeds_every_clamp -- so every one of them runs the second trip of its
    grid-stride loop.  V on a grid where v d is an integer: the model needs no Fraction."""
    from demethify_amd.device import Problem

    V, D, Rt, src_m = _big()
    assert D.dtype == np.int64 and src_m.ND == 1 and src_m.X16 is not None
    t0 = time.time()
    with Problem(ctx, V, D, Rt) as src:
        _check("big created", src, src_m)
    print(f"big created: {time.time() - t0:.2f} s")


def test_grid_stride_tails_gathered(ctx):
    """... k_gather_rows (65536), k_gather_rows_u16 (2048), k_index_range_check (1024) and k_build_dt8 again, by a seeded
    resample of N rows, with host and with device indices."""
    from demethify_amd.device import Problem
    from demethify_amd.staging import indices_to_device

    V, D, Rt, src_m = _big()
    idx = _resample(pm.BIG.N, pm.BIG.N, 24)
    t0 = time.time()
    want = pm.gathered(src_m, idx)
    with Problem(ctx, V, D, Rt) as src:
        dev = indices_to_device(idx, ctx)
        with src.gather(dev) as g:
            _check("big gathered (device indices)", g, want)
        dev.close()
        with src.gather(idx) as g:
            rep = g.report()
            same = all(np.array_equal(g.copy_out(k, rep), getattr(want, k)) for k in ("D16", "X16", "Dt8", "V", "Rtp"))
            print(f"big gathered (host indices): D16, X16, Dt8, V, Rtp equal the model: {same}; kDmax {rep['kDmax']} x16_sum {rep['x16_sum']!r}")
            assert same and rep["kDmax"] == want.consts["kDmax"] and rep["x16_sum"] == float(want.x16_sum)
    print(f"big gathered: {time.time() - t0:.2f} s")


def test_grid_stride_tails_masked(ctx):
    """... and k_mask_rows (4096), with k_build_dt8 on the masked counts."""
    from demethify_amd.device import Problem

    V, D, Rt, src_m = _big()
    mask = np.random.RandomState(25).rand(*V.shape) < 0.7
    t0 = time.time()
    want = pm.masked(src_m, mask)
    with Problem(ctx, V, D, Rt) as src, src.masked(mask) as k:
        _check("big masked", k, want)
    print(f"big masked: {time.time() - t0:.2f} s")


# ---------------------------------------------------------------------------------------------- known block of derived problems
def _known_rows(n_c):
    feats = ge.known_features(n_c)
    return feats, [ge.tri(k, l) for k, l in feats], [ge.tri(k, n_c) for k in range(n_c + 1)]


def _check_known(name, p, family, Rt, V, D, Vi, Di, Ri, nd, N, int_route):
    """gram_known() of a derived problem whose host arrays are (V, D, Rt): the dense pairs EQUAL the integer model on the
    integer route; on dyadic data every row equals the one right answer on any route; elsewhere the derived bound of
    tests/test_gpu_gram_exact.py, (N + 4) 2^-53 sum |term| against the exact rational (gram_exact.within_bound)."""
    n_c = Rt.shape[1]
    feats, dense_rows, rhs_rows = _known_rows(n_c)
    gk, text = p.gram_known()
    assert text.startswith("int_known " if int_route else "fp64 "), text
    checks = []
    if int_route:
        checks.append(("dense = integer model", gk[dense_rows], ge.want_gram(Rt, feats, Di, nd)))
    if family == "dyadic":
        d = ge.Data("dyadic", V, D, Rt, None, Vi, Di, Ri, np.zeros((N, 0), dtype=np.int64), nd)
        b, vdv = ge.dyadic_rhs(d)
        checks.append(("dense = dyadic answer", gk[dense_rows], ge.dyadic_gram(d, feats)))
        checks.append(("b_k, vDv = dyadic answer", gk[rhs_rows], np.vstack([b, vdv[None, :]])))
    for what, got, want in checks:
        bad = int((got != want).sum())
        print(f"{name} [{text}]: {what}: {bad} of {got.size} entries differ")
        assert bad == 0, (name, what)
    if family == "full":
        bounded = [("b_k", gk[rhs_rows[:-1]], [Rt], [D, V]), ("vDv", gk[rhs_rows[-1:]], [np.ones((N, 1))], [D, V, V])]
        if not int_route:
            bounded.append(("dense", gk[dense_rows], [Rt[:, [k for k, _ in feats]], Rt[:, [l for _, l in feats]]], [D]))
        for what, got, factors, weights in bounded:
            ok = ge.within_bound(got, ge.exact_sums(factors, weights), N)
            print(f"{name} [{text}]: {what}: {int((~ok).sum())} of {got.size} entries outside ({N} + 4) x 2^-53 sum|term|")
            assert ok.all(), (name, what)


@pytest.mark.parametrize("level", [0, 3])
@pytest.mark.parametrize("family", ["dyadic", "full"])
@pytest.mark.parametrize("n_c,nd", [(5, 1), (4, 2)])
def test_known_block_of_derived_problems(ctx, n_c, nd, family, level):
    """tests/gram_exact.py's two families at 130 x 70, one digit with n_c % 4 != 0 and two digits: gram_known() of the
    gathered and of the masked problem, on the integer route (level 0: the text starts with "int_known") and on the FP64
    route (level 3, set before the source is created)."""
    from demethify_amd.device import Problem

    N, S = 130, 70
    d = ge.make(family, N, S, n_c, 0, nd, seed=5 + n_c)
    idx, mask = _resample(N, N + 9, 50 + n_c), _mask(N, S, 51)
    Vi = d.Vi if d.Vi is not None else np.zeros((N, S), dtype=np.int64)
    Ri = d.Ri if d.Ri is not None else np.zeros((N, n_c), dtype=np.int64)
    with _settings(ctx, True, level):
        with Problem(ctx, d.V, d.D, d.Rt) as src:
            assert src.report()["ND"] == (nd if level == 0 else 0)
            with src.gather(idx) as g:
                _check_known(f"known gathered {family} n_c={n_c} nd={nd} level {level}", g, family, d.Rt[idx], d.V[idx], d.D[idx],
                             Vi[idx], d.Di[idx], Ri[idx], nd, len(idx), level == 0)
            with src.masked(mask) as k:
                _check_known(f"known masked {family} n_c={n_c} nd={nd} level {level}", k, family, d.Rt, d.V * mask, d.D * mask,
                             Vi * mask, d.Di * mask, Ri, nd, N, level == 0)


# ---------------------------------------------------------------------------------------------- level 3
@pytest.mark.parametrize("c", [pm.TAILS[0], pm.TAILS[3]], ids=lambda c: f"{c.N}x{c.S}-{c.n_c}")
def test_level_3_has_no_integer_copies_on_any_route(ctx, c):
    """The level is set before the source is created (and put back in a `finally`): no D16, X16, W16 or Dt8 on any route, ND = 0;
    a gather recomputes every constant from the gathered arrays, a mask carries the exactness flags and takes max(D) from the
    kept elements; the padded R_trunc copy is there as ever."""
    V, D, Rt = pm.true_data(c.N, c.S, c.n_c, 7 + c.N, 300, rt_grid=False, max_at=(c.N - 1, c.S - 1))

    def expect(m):
        for r in m.values():
            assert r.ND == 0 and r.D16 is None and r.X16 is None and r.W16 is None and r.Dt8 is None and r.Rtp is not None

    before = ctx.generic_level
    try:
        got = _routes(ctx, f"level 3 {c.N}x{c.S}-{c.n_c}", V, D, Rt, _resample(c.N, c.N + 3, 1), _mask(c.N, c.S, 2), level=3,
                      nested=True, expect=expect)
    finally:
        ctx.set_generic(before)
    assert ctx.generic_level == 0
    for rep, _ in got.values():
        assert rep["ND"] == 0 and rep["has_D16"] == 0 and rep["has_Dt8"] == 0


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(ctx):
    import ctypes as C

    from demethify_amd import _lib as L
    from demethify_amd.device import Problem

    lib = L.load()
    V, D, Rt = pm.true_data(33, 2, 0, 1, 50)
    ints, dbls = (C.c_int64 * len(L.REPORT_INTS))(), (C.c_double * len(L.REPORT_DBLS))()
    assert lib.dmf_problem_report(None, ints, dbls) == L.DMF_ERR_BAD_ARG
    out = np.zeros(33 * 2)
    assert lib.dmf_problem_copy_out(None, L.PROBLEM_ARRAYS["V"], out.ctypes.data, out.nbytes) == L.DMF_ERR_BAD_ARG
    with Problem(ctx, V, D, None) as p:
        h = p._h
        assert lib.dmf_problem_report(h, None, dbls) == L.DMF_ERR_BAD_ARG
        assert lib.dmf_problem_report(h, ints, None) == L.DMF_ERR_BAD_ARG
        assert lib.dmf_problem_copy_out(h, L.PROBLEM_ARRAYS["V"], None, out.nbytes) == L.DMF_ERR_BAD_ARG
        for wrong in (out.nbytes - 8, out.nbytes + 8, 0, -1):   # a size that is not the array's: nothing is copied
            out[:] = -7.0
            assert lib.dmf_problem_copy_out(h, L.PROBLEM_ARRAYS["V"], out.ctypes.data, wrong) == L.DMF_ERR_BAD_SHAPE
            assert (out == -7.0).all()
        assert lib.dmf_problem_copy_out(h, L.PROBLEM_ARRAYS["V"], out.ctypes.data, out.nbytes) == L.DMF_OK
        assert np.array_equal(out.reshape(33, 2), V)
        big = np.zeros(1 << 16, dtype=np.uint8)
        for absent in ("Rt", "Rtp", "W16", "mask_bits"):   # no known types, not a masked problem
            for size in (0, 8, big.nbytes):
                assert lib.dmf_problem_copy_out(h, L.PROBLEM_ARRAYS[absent], big.ctypes.data, size) == L.DMF_ERR_BAD_ARG
        for unknown in (-1, len(L.PROBLEM_ARRAYS), 99):
            assert lib.dmf_problem_copy_out(h, unknown, big.ctypes.data, 8) == L.DMF_ERR_BAD_ARG
        with pytest.raises(L.DemethifyHipError) as e:
            p.copy_out("W16")
        assert e.value.status == L.DMF_ERR_BAD_ARG
    assert lib.dmf_abi_version() == 1   # additive: no signature changed
