"""The cost plan and the exact cost fixture, without a GPU: the fixture's integer is what float64 gives in any order of sums,
dmf_cost_describe answers what the rules say, and the case table of tests/test_gpu_cost_exact.py reaches every instance of the
cost kernels (csrc/dmf_kernels_stream.hip)."""
import itertools

import numpy as np
import pytest

import cost_exact as ce


@pytest.fixture(scope="module")
def lib():
    from demethify_amd import _build, _lib

    _build.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------- the fixture
def _pairwise(x):
    x = list(x)
    while len(x) > 1:
        x = [x[i] + x[i + 1] if i + 1 < len(x) else x[i] for i in range(0, len(x), 2)]
    return x[0]


@pytest.mark.parametrize("N,S,n_c,n_u,dmax,scale", [
    (129, 33, 3, 8, 127, 1), (600, 257, 16, 4, 32639, 1), (333, 130, 0, 16, 3000, 1), (77, 7, 6, 1, 40, 1),
    (67, 129, 4, 2, 127, 4), (1, 1, 0, 1, 40000, 1), (3, 2, 7, 0, 32639, 1),
])
def test_fixture_integer_is_the_float64_sum_in_any_order(N, S, n_c, n_u, dmax, scale):
    c = ce.exact_case(N, S, n_c, n_u, dmax, seed=N + S, count_scale=scale)
    assert c.alpha.shape == (n_c + n_u, S) and (c.alpha.sum(axis=0) == 1.0).all() and c.alpha.min() >= 0.0
    assert c.V.min() >= 0.0 and c.V.max() <= 1.0 and c.Di.max() == dmax
    assert 0.05 < (c.Di == 0).mean() < 0.15 or N * S < 200
    R = c.Ri / 16.0
    assert (c.Rt is None) == (n_c == 0) and (c.u is None) == (n_u == 0)
    if n_c:
        assert np.array_equal(c.Rt, R[:, :n_c])
    if n_u:
        assert np.array_equal(c.u, R[:, n_c:])
    D = np.asarray(c.D, dtype=np.float64)
    pred = np.zeros((N, S))
    for k in range(n_c + n_u):  # the kernels' own chain, one known / unknown type after the other
        pred = R[:, k:k + 1] * c.alpha[k:k + 1, :] + pred
    e = c.V - pred
    assert np.array_equal(e * 1024, c.Vi - c.Ri @ c.Ai)
    t = D * e * e
    unit = ce.UNITS * scale
    by_rows = 0.0
    for i in range(N):
        row = 0.0
        for s in range(S):
            row += t[i, s]
        by_rows += row
    by_cols = 0.0
    for s in range(S):
        by_cols += float(np.add.reduce(t[:, s][::-1]))
    pairwise = _pairwise(t.ravel())
    assert by_rows * unit == c.want and by_cols * unit == c.want and pairwise * unit == c.want
    assert isinstance(c.want, int) and c.want > 0


def test_fixture_refuses_a_sum_beyond_2_to_53():
    # N S dmax = 2^33.6: the total of such a case can pass 2^53 units, and every E = 1024 here makes it do so
    N, S, dmax = 2048, 2048, 3000
    Di = np.full((N, S), dmax, dtype=np.int64)
    Vi = np.full((N, S), 1024, dtype=np.int64)
    with pytest.raises(AssertionError, match="2\\^53"):
        ce.exact_sum(Di, Vi, np.zeros((N, 1), dtype=np.int64), np.full((1, S), 64, dtype=np.int64))
    # ... and just inside the bound it answers
    assert ce.exact_sum(Di[:1024], Vi[:1024], np.zeros((1024, 1), dtype=np.int64), np.full((1, S), 64, dtype=np.int64)) \
        == 1024 * S * dmax * ce.UNITS


# ---------------------------------------------------------------------------------------------- the describe rule
S_GRID = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049, 65536, 65537, 131072, 131073)
NC_GRID = (0, 1, 3, 4, 5, 15, 16, 17, 48, 49)
NU_GRID = (0, 1, 4, 5, 15, 16, 17)


def test_describe_rule_over_a_grid(lib):
    n = 0
    for S, n_c, n_u, u16, level, v_align in itertools.product(S_GRID, NC_GRID, NU_GRID, (False, True), range(5), (0, 8)):
        if n_c + n_u < 1 or n_c + n_u > 64:
            continue
        got = ce.pure_describe(lib, S, n_c, n_u, u16, level, v_align=v_align)
        assert got == ce.expected_describe(S, n_c, n_u, u16, level, v_align=v_align), (S, n_c, n_u, u16, level, v_align)
        if level in (1, 2):
            assert got.startswith("cost=k_cost alpha="), got
        n += 1
    assert n > 10000


def test_describe_boundaries(lib):
    d = lambda *a, **k: ce.pure_describe(lib, *a, **k)  # noqa: E731  (S, n_c, n_u, u16, level)
    # two samples per lane from 128 samples on (u16 counts), one sample per lane below
    assert d(127, 8, 2, True, 0) == "cost=k_cost_cols<2,2,u16>"
    assert d(128, 8, 2, True, 0) == "cost=k_cost_cols2<2,2,even>"
    assert d(129, 7, 2, True, 0) == "cost=k_cost_cols2<2,2,odd>"
    assert d(129, 7, 2, False, 0) == "cost=k_cost_cols<2,2,f64>"
    assert d(128, 8, 2, True, 3) == "cost=k_cost_cols2<2,2,even>" and d(128, 8, 2, True, 4) == "cost=k_cost_cols2<2,2,even>"
    # V 8 bytes off a 16-byte boundary: the same kernels (their 16-byte loads take 8-byte-aligned rows)
    assert d(128, 8, 2, True, 0, v_align=8) == "cost=k_cost_cols2<2,2,even>"
    assert d(129, 8, 5, True, 0, v_align=8) == "cost=k_cost_cols2<2,5,odd>"
    assert d(128, 8, 2, True, 0, v_align=4) == "cost=k_cost_cols<2,2,u16>"
    # the wide form: 5..16 unknowns, from 32 samples on, level 0, u16 counts only
    assert d(31, 4, 5, True, 0) == ce.LDS and d(32, 4, 5, True, 0) == "cost=k_cost_cols2<1,5,even>"
    assert d(33, 4, 5, True, 0) == "cost=k_cost_cols2<1,5,odd>"
    assert d(64, 4, 4, True, 0) == "cost=k_cost_cols<1,4,u16>" and d(64, 4, 5, True, 0) == "cost=k_cost_cols2<1,5,even>"
    assert d(64, 4, 16, True, 0) == "cost=k_cost_cols2<1,16,even>" and d(64, 4, 17, True, 0) == ce.LDS
    assert d(64, 4, 5, False, 0) == ce.LDS and d(64, 4, 5, True, 3) == ce.LDS and d(64, 4, 5, True, 4) == ce.LDS
    # known types: 16 / 17
    assert d(64, 16, 1, True, 0) == "cost=k_cost_cols<4,1,u16>" and d(64, 17, 1, True, 0) == ce.LDS
    assert d(200, 16, 6, True, 0) == "cost=k_cost_cols2<4,6,even>" and d(200, 17, 6, True, 0) == ce.LDS
    assert d(64, 16, 0, True, 0) == "cost=k_cost_cols<4,0,u16>" and d(64, 0, 4, False, 4) == "cost=k_cost_cols<0,4,f64>"
    # without the padded R_trunc copy: the any-shape kernel
    assert d(64, 8, 2, True, 0, rtp=False) == ce.LDS and d(64, 0, 2, True, 0, rtp=False) == "cost=k_cost_cols<0,2,u16>"
    # the scratch holds 1024 partials: ceil(S / 64) (two samples per lane: ceil(S / 128)) partial columns must fit
    assert d(65536, 1, 1, False, 0) == "cost=k_cost_cols<1,1,f64>" and d(65537, 1, 1, False, 0) == ce.GLOBAL
    assert d(65600, 1, 1, False, 0) == ce.GLOBAL
    assert d(65537, 1, 1, True, 0) == "cost=k_cost_cols2<1,1,odd>"
    assert d(131072, 1, 1, True, 0) == "cost=k_cost_cols2<1,1,even>" and d(131073, 1, 1, True, 0) == ce.GLOBAL
    assert d(131072, 1, 5, True, 0) == "cost=k_cost_cols2<1,5,even>" and d(131073, 1, 5, True, 0) == ce.GLOBAL
    # alpha in LDS while K S 8 <= 48 KiB
    assert d(6144, 0, 1, False, 1) == ce.LDS and d(6145, 0, 1, False, 1) == ce.GLOBAL
    assert d(256, 20, 4, False, 0) == ce.LDS and d(257, 20, 4, False, 0) == ce.GLOBAL
    # levels 1 and 2: always the any-shape kernel
    for level in (1, 2):
        for S, n_c, n_u in ((64, 4, 2), (128, 4, 2), (129, 0, 1), (200, 8, 8), (2, 16, 4)):
            assert d(S, n_c, n_u, True, level) == ce.LDS and d(S, n_c, n_u, False, level) == ce.LDS


def test_describe_refuses_bad_keys(lib):
    import ctypes

    buf = ctypes.create_string_buffer(64)
    for args in ((0, 1, 1, 0, 0, 0, 1, 0), (64, 0, 0, 0, 0, 0, 1, 0), (64, 60, 5, 0, 0, 0, 1, 0), (64, 1, 1, 0, 0, 0, 1, 5),
                 (64, 1, 1, 1, 0, 0, 1, 0), (64, -1, 2, 0, 0, 0, 1, 0), (64, 1, 1, 0, 0, 16, 1, 0)):
        assert lib.dmf_cost_describe(*args, buf, len(buf)) == 1, args
    assert lib.dmf_cost_describe(64, 1, 1, 0, 0, 0, 1, 0, None, 0) == 1


# ---------------------------------------------------------------------------------------------- coverage
def test_case_table_reaches_every_instance(lib):
    """100 % of the 48 + 48 + 120 column-resident instances and both forms of k_cost, by the pure describe function on the
    key each case's problem has; every k_cost_cols2 (NKC, NU) with both parities of S."""
    cases = ce.instance_cases()
    got = set()
    for c in cases:
        desc = ce.describe_case(lib, c)
        assert desc == c.expect == ce.expected_describe(c.S, c.n_c, c.n_u, ce.has_u16(c), c.level), c
        assert c.N * c.S * c.dmax <= 1 << 33, c
        got.add(desc)
        if ce.has_u16(c):  # the same problem at level 1: the any-shape kernel on the f64 counts
            assert ce.describe_case(lib, c, level=1).startswith("cost=k_cost alpha="), c
    assert got == ce.all_column_instances(), got ^ ce.all_column_instances()
    assert len(cases) == 216
    # both forms of k_cost, and the shapes of the other tables
    generic = {ce.describe_case(lib, c) for c in ce.generic_cases()}
    assert generic == {ce.LDS, ce.GLOBAL}
    for c in ce.generic_cases() + ce.grid_cap_cases() + [ce.WIDE_S_CASE]:
        assert ce.describe_case(lib, c) == c.expect, c
        assert c.N * c.S * c.dmax <= 1 << 33, c
    # what the shapes are chosen for
    assert {c.N for c in cases} == set(ce.ROWS)
    assert {c.n_c % 4 for c in cases if c.n_c} == {0, 3}
    u16 = [c for c in cases if ce.has_u16(c)]
    assert {c.dmax for c in u16} == {127, 32639}
    assert {(c.dmax, c.count_scale, c.level) for c in cases if not ce.has_u16(c)} == {(40000, 1, 0), (127, 4, 0), (127, 1, 4)}
    assert {c.S for c in cases if "cols<" in c.expect and "u16" in c.expect} == set(ce.S_COLS_U16)
    assert {c.S for c in cases if "f64" in c.expect} == set(ce.S_COLS_F64)
    narrow = [c for c in cases if "cols2" in c.expect and c.n_u <= 4]
    wide = [c for c in cases if "cols2" in c.expect and c.n_u >= 5]
    assert {c.S for c in narrow} == set(ce.S_NARROW["even"] + ce.S_NARROW["odd"])
    assert {c.S for c in wide} == set(ce.S_WIDE["even"] + ce.S_WIDE["odd"])
