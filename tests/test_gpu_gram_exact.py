"""The packed Gram read back entry by entry (Solver.gram, Problem.gram_known) and held to exact integers.

Integer route (k_bu_cols / k_bu_cols2 + k_gram_i8_w8 + k_gram_v2_reduce + k_gram_v2_finish): every cross / uu entry and every
dense pair of the known block must EQUAL finish(model) of tests/gram_exact.py -- the result is predictable bit for bit on
arbitrary doubles in [0, 1] -- on a dyadic and on a full-mantissa family, over a case table that test_gram_exact_host.py
proves (through the pure dmf_gram_i8_describe) to reach, for each of the four instances of the kernel, 1, 2, 3, RING - 1, RING,
RING + 1 and >= 2 RING + 1 blocks per row range, a shorter last range, ragged tails with an odd end of u, idle sample waves,
both workgroup orders and every chunking of the reduce.  No tolerance appears on that route.

Right-hand sides and FP64 kernels.  b_u, b_k and v^T D v are FP64 sums of products that involve v; so is every entry of
k_gram_u, k_gram_mfma and k_gram.  On the dyadic family every product and every partial sum in any order is representable,
so these have one right answer too and are asserted EQUAL to it.  On the full-mantissa family they are held to

    |got - exact| <= (N + 4) 2^-53 sum_i |term_i|                                    (the derived bound)

against the exact rational sum.  Derivation (u = 2^-53): a term is a product of three doubles formed with at most two
roundings, t^_i = t_i (1 + th_i), |th_i| <= 2 u + u^2 (an FMA that adds the product saves one of them); N terms summed in ANY
order -- lanes, waves, slabs, chunks -- are N - 1 rounded additions (one more where an accumulator starts from a rounded
partial), each off by at most u times a partial sum, which is at most sum |t^_i| as all terms are non-negative:
|s^ - sum t^_i| <= N u (1 + u)^N sum |t^_i|.  Together (N + 2) u + O(N^2 u^2) <= (N + 4) u for every N here (N < 2^20).  It
is the worst case, not a measurement.  It is checked at EVERY shape: against the exact rational (big integers) where
N S rows <= 2 10^6, else against the sum in x87 extended precision, whose own error -- at most (N + 4) 2^-63 sum |term| --
is taken off the limit (gram_exact.within_bound_extended), so that passing still implies the bound above.

No FP64 kernel here scales by anything but the data, so none needed the bound on dyadic data.

Each case prints what it measured before it asserts (mismatching entries, largest difference in units of 2^-52)."""
import functools
import time

import numpy as np
import pytest

import gram_exact as ge

pytestmark = pytest.mark.gpu

FAMILIES = ("dyadic", "full")
BOUND_MAX_WORK = 2_000_000   # N x S x rows: what the exact rational sums of a case may cost (about a second)


def _cid(c):
    return f"{c.N}x{c.S}-{c.n_c}+{c.n_u}-nd{c.nd}"


@functools.lru_cache(maxsize=2)
def _data(family, N, S, n_c, n_u, nd):
    d = ge.make(family, N, S, n_c, n_u, nd, seed=1 + (N * 31 + S * 17 + n_c * 7 + n_u * 3 + nd) % 100003)
    for a in d:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _alpha0(K, S):
    return np.full((K, S), 1.0 / K)


def _report(name, got, want):
    bad = got != want
    worst = float(np.abs(got - want).max()) * 2.0 ** 52 if got.size else 0.0
    print(f"{name}: {int(bad.sum())} of {got.size} entries differ, largest difference {worst:.6g} x 2^-52")
    return not bad.any()


def _rows(feats):
    return [ge.tri(k, l) for k, l in feats]


def _check_bound(name, got, factors, weights, N):
    """The derived bound for rows got[p][s] = sum_i prod_f factors[f][i, p] prod_w weights[w][i, s]: against the exact
    rational where that is affordable, else against the extended-precision sum with its own error taken off the limit.
    One of the two always runs."""
    if N * weights[0].shape[1] * got.shape[0] <= BOUND_MAX_WORK:
        want = ge.exact_sums(factors, weights)
        ok = ge.within_bound(got, want, N)
        rel = max((abs(ge.Fraction(float(g)) - w) / w if w else 0) for g, w in zip(got.ravel().tolist(), want.ravel().tolist()))
        how = "exact rational"
    else:
        assert len(factors) == 1, "a product of two row factors is not exact in double: take the exact rational"
        ref = ge.extended_sums(factors[0], weights)
        ok = ge.within_bound_extended(got, ref, N)
        nz = ref > 0
        rel = float((np.abs(got.astype(np.longdouble) - ref)[nz] / ref[nz]).max()) if nz.any() else 0.0
        how = "extended precision"
    print(f"{name}: largest |got - reference| / sum|term| = {float(rel) * 2.0 ** 53:.3f} x 2^-53, bound {N + 4} x 2^-53 ({how})")
    assert ok.all(), (name, int((~ok).sum()))


def _check_solver_gram(lib, ctx, c, family, kind="integer", expect_text=None):
    """One solver on the case's data, built from u0 directly (gram() works on the current u; alpha0 is any point of the
    simplex): text, every u-dependent row, the known block carried over."""
    from demethify_amd.device import Problem, Solver

    t0 = time.time()
    d = _data(family, *c)
    K, feats = c.n_c + c.n_u, ge.solver_features(c.n_c, c.n_u)
    X = ge.X_of(d)
    with Problem(ctx, d.V, d.D, d.Rt) as p, Solver(p, d.u, _alpha0(K, c.S)) as s:
        gb, text = s.gram(kind)
        gk = p.gram_known()[0]
    t1 = time.time()
    if kind == "integer":
        assert text == ge.describe(lib, *c), text
    else:
        assert text.startswith(expect_text), text
    # u-dependent, V-free rows
    got = gb[_rows(feats)]
    if family == "dyadic":
        want = ge.dyadic_gram(d, feats)
        if kind == "integer":  # (the model says the same: lo = 0 there)
            assert c.N * c.S > 500_000 or np.array_equal(ge.want_gram(X, feats, d.Di, c.nd), want)
    else:
        want = ge.want_gram(X, feats, d.Di, c.nd) if kind == "integer" else None
    if want is not None:
        assert _report(f"{kind} {family} {_cid(c)} cross/uu [{text}]", got, want)
    else:   # (the FP64 kinds on the full-mantissa family; their shapes are small: the exact rational)
        assert c.N * c.S * len(feats) <= BOUND_MAX_WORK, "an FP64 case too large for the exact rational: shrink it"
        _check_bound(f"{kind} full {_cid(c)} cross/uu", got, [X[:, [k for k, _ in feats]], X[:, [l for _, l in feats]]], [d.D], c.N)
    # b_u: equality on the dyadic family, the derived bound on the other -- at every shape
    got_b = gb[[ge.tri(c.n_c + j, K) for j in range(c.n_u)]]
    if family == "dyadic":
        assert _report(f"{kind} dyadic {_cid(c)} b_u", got_b, ge.dyadic_rhs(d)[0][c.n_c:])
    else:
        _check_bound(f"{kind} full {_cid(c)} b_u", got_b, [d.u], [d.D, d.V], c.N)
    # the known block is the problem's, row for row
    for l in range(c.n_c):
        for k in range(l + 1):
            assert np.array_equal(gb[ge.tri(k, l)], gk[ge.tri(k, l)])
    for k in range(c.n_c):
        assert np.array_equal(gb[ge.tri(k, K)], gk[ge.tri(k, c.n_c)])
    assert np.array_equal(gb[ge.tri(K, K)], gk[ge.tri(c.n_c, c.n_c)])
    print(f"{_cid(c)} {family}: device {t1 - t0:.2f} s (with the data), reference {time.time() - t1:.2f} s")


@pytest.fixture(scope="module")
def lib():
    from demethify_amd import _lib as L

    return L.load()


# ---------------------------------------------------------------------------------------------- integer kind
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", ge.wrap_cases(), ids=_cid)
def test_integer_gram_wrapped_ring(lib, ctx, case, family):
    _check_solver_gram(lib, ctx, case, family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", ge.small_cases(), ids=_cid)
def test_integer_gram_few_blocks_and_sample_edges(lib, ctx, case, family):
    _check_solver_gram(lib, ctx, case, family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", ge.feature_cases() + ge.exact_count_cases(), ids=_cid)
def test_integer_gram_feature_counts_and_row_images(lib, ctx, case, family):
    _check_solver_gram(lib, ctx, case, family)


def test_step_after_gram_is_bit_identical(ctx):
    """The solver stays usable: gram() of both kinds, then two outer iterations, against the same iterations on a fresh
    solver -- u, alpha, cost and the Gram afterwards, bit for bit."""
    from demethify_amd.device import Problem, Solver

    for c in (ge.GramCase(333, 70, 4, 3, 1), ge.GramCase(257, 130, 14, 3, 2)):
        d = _data("full", *c)
        K = c.n_c + c.n_u
        with Problem(ctx, d.V, d.D, d.Rt) as p:
            with Solver(p, d.u, _alpha0(K, c.S)) as fresh:
                fresh.step(2, 5, 0.0)
                want = fresh.get()
                want_gb = fresh.gram("integer")[0]
            with Solver(p, d.u, _alpha0(K, c.S)) as s:
                first = s.gram("integer")[0]
                s.gram("fp64")
                assert np.array_equal(s.gram("integer")[0], first)   # (the scratch is left zero: a second call agrees)
                s.step(2, 5, 0.0)
                got = s.get()
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2:] == want[2:]
                assert np.array_equal(s.gram("integer")[0], want_gb)
                # a converged solver computes too
                s.step(50, 5, 1e30)
                it, conv = s.step(0, 5, 1e30)
                assert conv
                u_now = s.get()[0]
                feats = ge.solver_features(c.n_c, c.n_u)
                gb = s.gram("integer")[0]
                X = np.hstack([d.Rt, u_now])
                assert np.array_equal(gb[_rows(feats)], ge.want_gram(X, feats, d.Di, c.nd))


# ---------------------------------------------------------------------------------------------- known block
KNOWN_SMALL = [(n_c, nd) for n_c in (1, 4, 5, 16, 17, 32) for nd in (1, 2)]
KNOWN_WRAP = [(4571, 2017, 5, 1), (4571, 2017, 5, 2), (4571, 2017, 17, 1), (3581, 2048, 17, 2)]


def _check_known(lib, ctx, N, S, n_c, nd, family, level):
    from demethify_amd.device import Problem

    d = _data(family, N, S, n_c, 0, nd)
    feats = ge.known_features(n_c)
    before = ctx.generic_level
    ctx.set_generic(level)
    try:
        with Problem(ctx, d.V, d.D, d.Rt) as p:
            gk, text = p.gram_known()
    finally:
        ctx.set_generic(before)
    name = f"known {family} {N}x{S}-{n_c}-nd{nd} level {level} [{text}]"
    if level == 0:   # (the dense pairs on the integer matrix cores, then the stream kernel of b_k, v^T D v with it or after it)
        lead = "int_known " + ge.describe(lib, N, S, n_c, 0, nd)
        if S >= 128 and n_c <= 16:   # (two samples per lane: v^T D v rides along)
            assert text == lead + " + k_bu_cols2 with vDv", text
        else:                        # (v^T D v by a kernel of its own: the stream kernel where its slab fits, else k_gram)
            assert text == lead + " + k_bu_cols + k_vdv_cols" or text.startswith(lead + " + k_bu_cols + k_gram launches=1 "), text
    else:
        assert text.startswith("fp64 k_gram_mfma<") and text.endswith(" + k_vdv_cols"), text
    got = gk[_rows(feats)]
    rhs_rows = [ge.tri(k, n_c) for k in range(n_c + 1)]
    if family == "dyadic":
        assert _report(name + " dense", got, ge.dyadic_gram(d, feats))
        b, vdv = ge.dyadic_rhs(d)
        assert _report(name + " b_k, vDv", gk[rhs_rows], np.vstack([b, vdv[None, :]]))
    elif level == 0:
        assert _report(name + " dense", got, ge.want_gram(d.Rt, feats, d.Di, nd))
    if family == "full":
        if level != 0:
            assert N * S * len(feats) <= BOUND_MAX_WORK, "an FP64 case too large for the exact rational: shrink it"
            _check_bound(name + " dense", got, [d.Rt[:, [k for k, _ in feats]], d.Rt[:, [l for _, l in feats]]], [d.D], N)
        _check_bound(name + " b_k", gk[rhs_rows[:-1]], [d.Rt], [d.D, d.V], N)
        _check_bound(name + " vDv", gk[rhs_rows[-1:]], [np.ones((N, 1))], [d.D, d.V, d.V], N)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n_c,nd", KNOWN_SMALL)
def test_known_block_integer_route_small(lib, ctx, n_c, nd, family):
    _check_known(lib, ctx, 130, 70, n_c, nd, family, 0)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N,S,n_c,nd", KNOWN_WRAP)
def test_known_block_integer_route_wrapped_ring(lib, ctx, N, S, n_c, nd, family):
    _check_known(lib, ctx, N, S, n_c, nd, family, 0)


def test_known_block_nine_launches_wrapped_ring(lib, ctx):
    """32 known types: 528 dense pairs, nine launches over nine blocks per range (dyadic: the reference is one GEMM)."""
    _check_known(lib, ctx, 4571, 2017, 32, 1, "dyadic", 0)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n_c,nd", [(1, 1), (5, 2), (17, 1)])
def test_known_block_fp64_route(lib, ctx, n_c, nd, family):
    """Level 3 (set before the problem is created): k_gram_mfma + the v^T D v stream kernel."""
    _check_known(lib, ctx, 130, 70, n_c, nd, family, 3)


def test_known_block_rows_are_not_transposed(ctx):
    """Three known types whose columns differ by powers of two, so that all six dense rows are distinct: row tri(k, l) =
    l (l + 1) / 2 + k holds the pair (k, l); any other packing order fails."""
    from demethify_amd.device import Problem

    d = _data("dyadic", 130, 70, 3, 0, 1)
    Rt = d.Rt * np.array([1.0, 0.5, 0.125])
    with Problem(ctx, d.V, d.D, Rt) as p:
        gk, text = p.gram_known()
    assert text.startswith("int_known ")
    base = ge.dyadic_gram(d, ge.known_features(3))
    want = {(k, l): base[i] * (1.0, 0.5, 0.125)[k] * (1.0, 0.5, 0.125)[l] for i, (k, l) in enumerate(ge.known_features(3))}
    rows = list(want.values())
    assert all(not np.array_equal(rows[i], rows[j]) for i in range(6) for j in range(i))
    for (k, l), w in want.items():
        assert np.array_equal(gk[l * (l + 1) // 2 + k], w), (k, l)
    b, _ = ge.dyadic_rhs(d)
    for k in range(3):
        assert np.array_equal(gk[3 * 4 // 2 + k], b[k] * (1.0, 0.5, 0.125)[k])


# ---------------------------------------------------------------------------------------------- refusals
def test_integer_kind_refuses_what_it_cannot_take(ctx):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    d = _data("dyadic", 130, 70, 2, 3, 2)
    D = np.array(d.D)
    D[3, 3] = 32640.0          # one count beyond the two digit planes: no integer copies
    with Problem(ctx, d.V, D, d.Rt) as p, Solver(p, d.u, _alpha0(5, 70)) as s:
        with pytest.raises(L.DemethifyHipError) as e:
            s.gram("integer")
        assert e.value.status == L.DMF_ERR_UNSUPPORTED
        gb, text = s.gram("fp64")    # (the FP64 kind still answers)
        assert text.startswith("k_gram")
    d = _data("dyadic", 130, 70, 29, 1, 1)   # padded 32 + 1 doubles per row
    with Problem(ctx, d.V, d.D, d.Rt) as p, Solver(p, d.u, _alpha0(30, 70)) as s:
        with pytest.raises(L.DemethifyHipError) as e:
            s.gram("integer")
        assert e.value.status == L.DMF_ERR_UNSUPPORTED
    with Problem(ctx, d.V, d.D, d.Rt) as p, Solver(p, d.u, _alpha0(30, 70)) as s:
        with pytest.raises(ValueError):
            s.gram("fp32")


# ---------------------------------------------------------------------------------------------- FP64 kernels
FP64 = [
    # level, expected kernel, N, S, n_c, n_u
    (0, "k_gram_u<4,3>", 77, 13, 2, 3), (0, "k_gram_u<0,4>", 161, 65, 0, 4), (0, "k_gram_u<16,1>", 100, 64, 16, 1),
    (0, "k_gram_u<8,5>", 333, 70, 5, 5), (3, "k_gram_u<4,3>", 77, 13, 2, 3),
    (0, "k_gram_mfma<", 99, 33, 17, 2), (0, "k_gram_mfma<", 130, 67, 0, 14), (0, "k_gram_mfma<", 161, 40, 12, 8),
    (0, "k_gram_mfma<", 70, 36, 20, 20),      # 630 jobs: more than the 512 that eight waves of four tiles hold
    (1, "k_gram ", 77, 13, 2, 3), (1, "k_gram ", 130, 67, 0, 5), (1, "k_gram ", 99, 33, 17, 2), (2, "k_gram ", 161, 40, 3, 2),
]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("level,kernel,N,S,n_c,n_u", FP64, ids=[f"L{f[0]}-{f[1].strip('< ')}-{f[2]}x{f[3]}-{f[4]}+{f[5]}" for f in FP64])
def test_fp64_gram_kernels(lib, ctx, level, kernel, N, S, n_c, n_u, family):
    """k_gram_u, k_gram_mfma and k_gram through the same accessor: equality on the dyadic family, the derived bound against
    the exact rational on the full-mantissa one (odd S, N % 16 != 0, n_c = 0, more jobs than one k_gram_mfma launch)."""
    before = ctx.generic_level
    ctx.set_generic(level)
    try:
        _check_solver_gram(lib, ctx, ge.GramCase(N, S, n_c, n_u, 2), family, kind="fp64", expect_text=kernel)
    finally:
        ctx.set_generic(before)


def test_fp64_mfma_takes_more_than_one_launch(ctx):
    from demethify_amd.device import Problem, Solver

    d = _data("dyadic", 70, 36, 20, 20, 2)
    with Problem(ctx, d.V, d.D, d.Rt) as p, Solver(p, d.u, _alpha0(40, 36)) as s:
        text = s.gram("fp64")[1]
    assert int(text.split("launches=")[1].split()[0]) >= 2, text
