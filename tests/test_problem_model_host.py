"""tests/problem_model.py without a GPU: the model is closed under its own operations (digits decode back to counts, a
permutation and its inverse are the identity, an all-ones mask changes nothing), accepts true x / d data and rejects the
three planted elements of tests/test_gpu_x16.py, the comparison function notices one wrong element of every class, and
every case of the GPU table reaches what its comment claims -- computed here from the shapes."""
from fractions import Fraction

import numpy as np
import pytest

import problem_model as pm

QUIET = lambda *a, **k: None
INT_CASES = [c for c in pm.TAILS if c.S >= 2]


def _source(c, max_count=100, seed=3, **kw):
    V, D, Rt = pm.true_data(c.N, c.S, c.n_c, seed, max_count, max_at=(c.N - 1, c.S - 1), **kw)
    return pm.created(V, D, Rt)


def _same(a, b, what=pm.ARRAYS):
    for k in what:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), k
        assert x is None or (x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y)), k
    assert a.consts == b.consts and a.rt_sumsq == b.rt_sumsq
    assert (a.ND, a.SD, a.N16, a.plane_stride) == (b.ND, b.SD, b.N16, b.plane_stride)
    assert a.x16_dev == b.x16_dev and a.x16_sum == b.x16_sum


# ---------------------------------------------------------------------------------------------- closure
@pytest.mark.parametrize("max_count", [127, 128, 32639])
@pytest.mark.parametrize("c", INT_CASES, ids=lambda c: f"{c.N}x{c.S}-{c.n_c}")
def test_digits_decode_back_to_the_counts(c, max_count):
    m = _source(c, max_count)
    assert m.ND == (1 if max_count <= 127 else 2) and m.Dt8.shape == (m.ND, (c.N + 31) // 32, m.SD // 32, 32, 32)
    assert m.Dt8.nbytes == m.plane_stride * m.ND
    back = pm.dt8_decode(m.Dt8)
    assert np.array_equal(back[:c.N, :c.S], m.D.astype(np.int64)) and np.array_equal(back[:c.N], m.D16[:c.N])
    assert not back[c.N:].any() and not back[:, c.S:].any()
    assert np.array_equal(m.D16[:c.N, :c.S], m.D.astype(np.int64)) and not m.D16[c.N:].any() and not m.D16[:, c.S:].any()
    assert int(m.D16.sum(dtype=np.int64)) == int(m.D.sum())
    # one element, by hand: count d at (row, sample) sits at [plane, row // 32, sample // 32, sample % 32, row % 32]
    i, s = c.N - 1, c.S - 1
    d = int(m.D[i, s])
    assert d == max_count
    b0 = int(m.Dt8[0, i // 32, s // 32, s % 32, i % 32])
    b1 = int(m.Dt8[1, i // 32, s // 32, s % 32, i % 32]) if m.ND == 2 else 0
    assert b0 + 256 * b1 == d and (m.ND == 1 or b0 == ((d + 128) % 256) - 128)


@pytest.mark.parametrize("c", INT_CASES, ids=lambda c: f"{c.N}x{c.S}-{c.n_c}")
def test_a_permutation_and_its_inverse_are_the_identity(c):
    m = _source(c, 300)
    perm = np.random.RandomState(1).permutation(c.N)
    inv = np.argsort(perm)
    back = pm.gathered(pm.gathered(m, perm), inv)
    _same(back, m)
    pm.compare("identity", *pm.as_readback(back), m, say=QUIET)


@pytest.mark.parametrize("c", pm.TAILS, ids=lambda c: f"{c.N}x{c.S}-{c.n_c}")
def test_an_all_ones_mask_gives_the_source(c):
    m = _source(c, 300)
    k = pm.masked(m, np.ones((c.N, c.S), dtype=bool))
    _same(k, m, what=("V", "D", "Rt", "Rtp", "D16", "X16", "Dt8"))
    assert k.n_test == 0 and np.array_equal(k.mask_bits, pm.pack_bits(np.ones((c.N, c.S), dtype=bool)))
    assert (k.W16 is None) == (m.D16 is None) and (k.W16 is None or (k.W16.shape == m.D16.shape and not k.W16.any()))


def test_an_everything_held_out_mask_leaves_zeros():
    c = pm.TAILS[0]
    m = _source(c, 300)
    k = pm.masked(m, np.zeros((c.N, c.S), dtype=bool))
    assert k.ND == 2 and not k.D16.any() and not k.X16.any() and not k.Dt8.any() and not k.V.any() and not k.D.any()
    assert k.consts["kDmax"] == 0.0 and k.consts["kDsq"] == 0.0 and k.consts["kIntCountMax"] == 0.0 and k.x16_sum == 0
    assert k.n_test == c.N * c.S and int(k.W16.sum()) == c.N * c.S and k.x16_dev == m.x16_dev


def test_gathered_model_follows_the_contract_not_a_recreation():
    """The maximum's row avoided: ND, the exactness flags and x16_dev stay the source's, kDmax and x16_sum are the rows'."""
    V, D, Rt, row = pm.planted_source(70, 40, 2, 5, 7, 300)
    src = pm.created(V, D, Rt)
    idx = pm.avoiding(70, row, 90, 2)
    g, again = pm.gathered(src, idx), pm.created(V[idx], D[idx], Rt[idx])
    assert src.ND == 2 and g.ND == 2 and again.ND == 1
    assert g.consts["kDmax"] == again.consts["kDmax"] == float(D[idx].max()) < src.consts["kDmax"]
    assert g.x16_sum == again.x16_sum == int(np.rint(V[idx] * D[idx]).sum())
    assert g.x16_dev == src.x16_dev >= again.x16_dev
    assert not g.Dt8[1].any() and np.array_equal(g.Dt8[0], again.Dt8[0]) and np.array_equal(g.D16, again.D16)
    # a source without integer copies: the gathered problem is a created one
    D2 = D.astype(np.float64)
    D2[row, 1] = 2.5
    src2 = pm.created(V, D2, Rt)
    assert src2.ND == 0 and src2.consts["kIntCountMax"] == float("inf")
    _same(pm.gathered(src2, idx), pm.created(V[idx], D2[idx], Rt[idx]))
    assert pm.gathered(src2, idx).ND == 1   # (the fractional count was in the avoided row)


# ---------------------------------------------------------------------------------------------- X16
def test_true_data_is_accepted_within_half_an_ulp():
    V, D, Rt = pm.true_data(300, 37, 2, 11, 32639)
    X, dev, xsum, n_bad = pm.x16_of(V, D)
    assert n_bad == 0 and X is not None and dev <= 2.0 ** -53
    assert np.array_equal(X[D > 0], np.rint(V * D)[D > 0].astype(np.int64)) and xsum == int(X.sum()) and (X <= D).all()
    # d = 0 with v = 0.7: x = 0, whatever v is
    V[3, 3], D[3, 3] = 0.7, 0
    X2, dev2, _, n_bad2 = pm.x16_of(V, D)
    assert n_bad2 == 0 and X2[3, 3] == 0 and dev2 == dev


@pytest.mark.parametrize("what", ["perturbed", "non_integral", "x_above_d"])
def test_planted_bad_elements_are_rejected(what):
    V, D, Rt = pm.true_data(300, 37, 2, 12, 200, zero_fraction=0.0)
    D = np.maximum(D, 1)
    V = np.rint(V * D) / D
    assert pm.x16_of(V, D)[3] == 0
    if what == "perturbed":
        V[100, 7] += 1e-9
    elif what == "non_integral":
        V[5, 3] = (np.rint(V[5, 3] * D[5, 3]) + 0.3) / D[5, 3]
    else:
        V[299, 36] = 1.0 + 1.0 / D[299, 36]
    X, dev, xsum, n_bad = pm.x16_of(V, D)
    assert X is None and n_bad == 1
    assert pm.created(V, D, Rt).X16 is None and pm.created(V, D, Rt).D16 is not None


def test_the_rounded_difference_is_the_fma_not_a_product():
    """v = fl(1 / 3), d = 3: the float product is exactly 1.0 (difference 0), the exact v d - 1 is -2^-54."""
    v = 1.0 / 3.0
    assert v * 3.0 == 1.0 and pm._exact_dev(v, 3, 1) == -(2.0 ** -54)
    X, dev, _, _ = pm.x16_of(np.array([[v, 0.25]]), np.array([[3.0, 4.0]]))
    assert dev == 2.0 ** -54 and X.tolist() == [[1, 1]]
    # on the grid the float arithmetic is the exact arithmetic: the same answers either way
    V, D, _ = pm.grid_data(200, 3, 0, 4)
    X, dev, xsum, n_bad = pm.x16_of(V, D)
    assert n_bad == 0 and dev == 0.0 and xsum == sum(int(Fraction(float(v)) * int(d)) for v, d in zip(V.ravel(), D.ravel()))


def test_rt_sumsq_grid_and_bound():
    rs = np.random.RandomState(0)
    R = rs.randint(0, 1025, size=(50, 3)) / 1024.0
    exact, grid = pm.rt_sumsq_of(R)
    assert grid and float(exact) == float((R * R).sum()) and exact == sum(Fraction(float(x)) ** 2 for x in R.ravel())
    R2 = rs.rand(50, 3)
    exact2, grid2 = pm.rt_sumsq_of(R2)
    assert not grid2
    m = pm.created(np.zeros((50, 2)), np.ones((50, 2)), R2)
    assert pm.rt_sumsq_ok(float((R2 * R2).sum()), m) and pm.rt_sumsq_ok(float(exact2), m)
    assert not pm.rt_sumsq_ok(float(exact2) * (1 + 200 * 2.0 ** -53), m)


# ---------------------------------------------------------------------------------------------- sensitivity
def _altered(m, how):
    rep, arr = pm.as_readback(m)
    how(rep, arr)
    return rep, arr


def test_comparison_fails_on_one_wrong_element_of_every_class():
    V, D, Rt, row = pm.planted_source(77, 13, 3, 9, 7, 300)
    src = pm.created(V, D, Rt)
    idx = pm.avoiding(77, row, 45, 3)
    g = pm.gathered(src, idx)
    mask = np.random.RandomState(2).rand(77, 13) < 0.6
    k = pm.masked(src, mask)
    pm.compare("gathered", *pm.as_readback(g), g, say=QUIET)
    pm.compare("masked", *pm.as_readback(k), k, say=QUIET)
    assert g.N16 == 48 and g.SD == 64 and g.rtp_width == 4 and src.consts["kDmax"] == 300.0 > g.consts["kDmax"]

    def at(name, index, value):
        def how(rep, arr):
            assert arr[name][index] != value
            arr[name][index] = value
        return how

    def scalar(name, value):
        def how(rep, arr):
            assert rep[name] != value
            rep[name] = value
            if name in pm.CONSTS:   # (a builder that gets a constant wrong uploads the same wrong value)
                arr["consts"][pm.CONSTS.index(name)] = value
        return how

    classes = {
        "a padding row of D16": (g, at("D16", (46, 5), 1)),
        "a padding row of X16": (g, at("X16", (47, 0), 1)),
        "a padding column of D16": (g, at("D16", (3, 13), 7)),
        "a padding column of W16": (k, at("W16", (3, 63), 1)),
        "a padding row of W16": (k, at("W16", (79, 0), 1)),
        "one Dt8 byte": (g, at("Dt8", (0, 1, 0, 12, 3), 5)),
        "one Dt8 byte of the padding rows": (g, at("Dt8", (1, 1, 1, 31, 31), -128)),
        "one Rtp padding entry": (g, at("Rtp", (44, 3), 1.0)),
        "x16_sum off by 1": (g, scalar("x16_sum", float(g.x16_sum + 1))),
        "kDmax of the source": (g, scalar("kDmax", src.consts["kDmax"])),
        "kDsq of the source": (g, scalar("kDsq", src.consts["kDsq"])),
        "n_test off by 1": (k, scalar("n_test", k.n_test + 1)),
        "x16_dev zeroed": (k, scalar("x16_dev", 0.0) if k.x16_dev else scalar("x16_dev", 1e-20)),
        "an array that must be absent": (g, lambda rep, arr: arr.__setitem__("W16", np.zeros((g.N16, g.SD), dtype=np.uint16))),
        "the device copy of a constant": (g, lambda rep, arr: arr["consts"].__setitem__(2, 300.0)),
    }
    for name, (m, how) in classes.items():
        lines = []
        with pytest.raises(AssertionError):
            pm.compare(name, *_altered(m, how), m, say=lines.append)
        assert any("differ" in l and " 0 of" not in l or "want" in l for l in lines), (name, lines)


# ---------------------------------------------------------------------------------------------- reach of the case table
def test_tail_cases_reach_what_they_claim():
    shapes = {(c.N, c.S, c.n_c) for c in pm.TAILS}
    assert shapes == {(77, 13, 3), (33, 2, 0), (1, 2, 1), (257, 130, 2), (96, 300, 1), (50, 1, 2), (64, 64, 4)}
    assert {c.n_c % 4 for c in pm.TAILS if c.n_c} == {0, 1, 2, 3} and any(c.n_c == 0 for c in pm.TAILS)
    ints = [c for c in pm.TAILS if c.S >= 2]
    assert len(ints) == len(pm.TAILS) - 1 and pm.created(*pm.true_data(50, 1, 2, 1, 50)).D16 is None
    row_tail16 = {(-c.N) % 16 for c in ints}
    row_tail32 = {(-c.N) % 32 for c in ints}
    assert row_tail16 == {0, 3, 15} and row_tail32 == {0, 19, 31}                     # N = 1: 31 digit rows to zero
    assert any((-c.N) % 32 >= 16 and (-c.N) % 16 != 0 for c in ints)                  # a tail in both: 77 -> 80 and 96
    blocks = sorted({pm.count_shapes(c.N, c.S)[0] // 32 for c in ints})
    assert blocks[0] == 2 and blocks[-1] == 10 and len(blocks) >= 3, blocks
    assert {(-c.S) % 64 for c in ints} >= {0, 62, 51, 20}
    # (64, 64, 4): nothing to pad, and Rtp is R_trunc
    m = _source(pm.TAILS[-1])
    assert (m.N16, m.SD, m.rtp_width, m.rtp_borrows_rt) == (64, 64, 4, True) and m.Dt8.shape[1:3] == (2, 2)
    for c in pm.TAILS:   # tile counts as the comments say
        SD, N16, ps = pm.count_shapes(c.N, c.S)
        assert ps == ((c.N + 31) // 32) * (SD // 32) * 1024
    assert pm.count_shapes(77, 13) == (64, 80, 3 * 2 * 1024) and pm.count_shapes(1, 2) == (64, 16, 2048)
    assert pm.count_shapes(257, 130) == (192, 272, 9 * 6 * 1024) and pm.count_shapes(96, 300) == (320, 96, 3 * 10 * 1024)


def test_big_case_exceeds_every_clamp():
    c = pm.BIG
    got = pm.clamps(c.N, c.S, c.n_c)
    assert set(got) == {"k_gather_rows", "k_gather_rows_u16", "k_mask_rows", "k_build_d16", "k_build_dt8", "k_pad_rows",
                        "k_reduce_partial", "k_convert_counts", "k_index_range_check"}
    for kernel, (asked, clamp) in got.items():
        assert asked > clamp, (kernel, asked, clamp)
    SD, N16, ps = pm.count_shapes(c.N, c.S)
    assert 130e6 < N16 * SD * 2 < 140e6 and 16e6 < c.N * c.S * 8 < 18e6
    # and the small cases stay below every clamp: the grid-stride tails are this case's alone
    for t in pm.TAILS:
        small = pm.clamps(t.N, t.S, t.n_c)
        assert sum(asked > clamp for asked, clamp in small.values()) == 0, t


def test_recycled_case_reaches_the_keep_threshold():
    c = pm.RECYCLED
    one, two = pm.pool_sizes(c.N, c.S, c.n_c, 1), pm.pool_sizes(c.N, c.S, c.n_c, 2)
    assert one == {"D16 / X16 / W16": 8208 * 128 * 2, "Dt8": 257 * 4 * 1024, "Rtp": 8197 * 16 * 8}
    assert one["Rtp"] == 1_049_216 and one["Dt8"] == 1_052_672
    for sizes in (one, two):
        for name, b in sizes.items():
            assert b >= pm.KEEP_MIN_BYTES, (name, b)
    # the three u16 copies of a closed masked problem fill the kept list of their size exactly: D16, X16, W16
    assert pm.KEEP_PER_SIZE == 3
    # padding exists in every one of them: 11 rows and 1 sample in the u16 copies, 27 digit rows, 3 columns of Rtp
    assert (-c.N) % 16 == 11 and (-c.S) % 64 == 1 and (-c.N) % 32 == 27 and (-c.n_c) % 4 == 3
    # ... and V, D (8197 x 127 doubles) and Rt (8197 x 13) are kept too, but have no padding


def test_gather_lengths_change_the_padding_and_the_tiles():
    shapes = {n: pm.count_shapes(n, 13) for n in pm.GATHER_LENGTHS}
    assert [shapes[n][1] for n in (1, 15, 16, 17, 31, 33)] == [16, 16, 16, 32, 32, 48]
    assert [shapes[n][2] // 2048 for n in (1, 15, 16, 17, 31, 33, 1000, 2500)] == [1, 1, 1, 1, 1, 2, 32, 79]
    assert min(pm.GATHER_LENGTHS) == 1 and max(pm.GATHER_LENGTHS) > pm.GATHER_SOURCE_N in pm.GATHER_LENGTHS


@pytest.mark.parametrize("name,top,x16,nd_src,nd_again", pm.LOSE_MAX)
def test_lose_max_cases_drop_the_maximum(name, top, x16, nd_src, nd_again):
    V, D, Rt, row = pm.planted_source(200, 64, 2, 21, 7, top)
    if not x16:
        V = np.round(V, 2)
    src = pm.created(V, D, Rt)
    idx = pm.avoiding(200, row, 200, 4)
    assert row not in idx and D[idx].max() < top and len(np.unique(idx)) < 200
    g, again = pm.gathered(src, idx), pm.created(V[idx], D[idx], Rt[idx])
    assert (src.ND, g.ND, again.ND) == (nd_src, nd_src, nd_again)
    assert (src.X16 is not None) == x16 and (g.X16 is not None) == x16
    assert g.consts["kDmax"] == again.consts["kDmax"] < src.consts["kDmax"]


@pytest.mark.parametrize("max_count,nd", pm.THRESHOLDS)
def test_digit_thresholds(max_count, nd):
    V, D, Rt, row = pm.planted_source(70, 40, 2, 6, 5, max_count)
    m = pm.created(V, D, Rt)
    assert m.ND == nd and (m.D16 is not None) == (nd > 0) and m.consts["kIntCountMax"] == float(max_count)
    if nd == 2:   # the row (or its large elements) left out: two planes kept, the second all zeros
        g = pm.gathered(m, pm.avoiding(70, row, 70, 1))
        k = pm.masked(m, D <= 127)
        for d in (g, k):
            assert d.ND == 2 and d.consts["kDmax"] <= 127 and not d.Dt8[1].any() and d.Dt8[0].any()
    for bad, value in (("fractional", 2.5), ("negative", -1.0)):
        D2 = D.astype(np.float64)
        D2[3, 3] = value
        m2 = pm.created(V, D2, Rt)
        assert m2.ND == 0 and m2.consts["kIntCountMax"] == float("inf") and m2.Rtp is not None
    Rt2 = Rt.copy()
    Rt2[4, 1] = 1.0 + 2.0 ** -52
    m3 = pm.created(V, D, Rt2)
    assert m3.ND == 0 and m3.consts["kRtOutsideUnit"] == 1.0 and not m3.rt_on_grid
