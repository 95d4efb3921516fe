"""The model of the integer Gram (tests/gram_exact.py) against brute-force rational arithmetic, and -- through the pure
dmf_gram_i8_describe -- the proof that the case table of tests/test_gpu_gram_exact.py reaches every class it claims.  No GPU."""
import collections
from fractions import Fraction

import numpy as np
import pytest

import gram_exact as ge


@pytest.fixture(scope="module")
def lib():
    from demethify_amd import _lib as L

    return L.load()


def _pairs():
    rs = np.random.RandomState(5)
    xa = np.concatenate([rs.rand(4000), ge.planted_values(), [1.0, 0.5, 0.5, 0.5, 0.25, 2.0 ** -30, 2.0 ** -52, 2.0 ** -53, 0.75]])
    xb = np.concatenate([rs.rand(4000), np.ones(len(ge.planted_values())),
                         [1.0, 3 / float(ge.TWO52), 5 / float(ge.TWO52), 7 / float(ge.TWO52), 6 / float(ge.TWO52), 2.0 ** -23,
                          0.5, 1.0, 2.0 ** -1000]])
    small = rs.rand(500) * 2.0 ** -rs.randint(0, 70, 500)
    return np.concatenate([xa, small, small]), np.concatenate([xb, rs.rand(500), small[::-1]])


def test_z_int_is_the_once_rounded_exact_product():
    xa, xb = _pairs()
    got = ge.z_int(xa, xb)
    want = [ge.z_int_scalar(a, b) for a, b in zip(xa.tolist(), xb.tolist())]
    assert got.tolist() == want
    # the ties: 1/2 x (2 m + 1) 2^-52 lies on a half and goes to the even neighbour, both parities
    assert ge.z_int(0.5, 3 / float(ge.TWO52)) == 2 and ge.z_int(0.5, 5 / float(ge.TWO52)) == 2
    assert ge.z_int(0.5, 7 / float(ge.TWO52)) == 4 and ge.z_int(0.5, 1 / float(ge.TWO52)) == 0
    assert ge.z_int(1.0, 1.0) == ge.TWO52 and ge.z_int(1.0, 2.0 ** -60) == 0 and ge.z_int(0.0, 1.0) == 0
    # a double rounding (product to double first, then rint) would differ somewhere on random data: the model does not take it
    twice = np.rint(xa[:4000] * xb[:4000] * float(ge.TWO52)).astype(np.int64)
    assert (twice != got[:4000]).any()


def test_digits_recombine():
    rs = np.random.RandomState(6)
    z = np.concatenate([rs.randint(0, ge.TWO52, size=5000, dtype=np.int64), [0, 1, 127, 128, 255, 256, ge.TWO52, ge.TWO52 - 1],
                        [(1 << k) - 1 for k in ge.SEAM_K], [1 << k for k in ge.SEAM_K]]).astype(np.int64)
    digits = ge.balanced_digits(z)
    assert len(digits) == 7
    for t, a in enumerate(digits):
        assert (a.min() >= -128 and a.max() <= 127) if t < 6 else (a.min() >= 0 and a.max() <= 16)
    assert ge.recombine(digits).tolist() == z.tolist()
    assert [int(a[-len(ge.SEAM_K) * 2 - 2]) for a in digits] == [0, 0, 0, 0, 0, 0, 16]  # z = 2^52: digit 6 = 16
    for nd, top in ((1, 127), (2, 32639)):
        d = np.concatenate([rs.randint(0, top + 1, size=3000), [0, 127, top] + ([128, 255, 256, 32511] if nd == 2 else [])])
        planes = ge.count_digits(d, nd)
        assert len(planes) == nd and all(p.min() >= -128 and p.max() <= 127 for p in planes)
        assert ge.recombine(planes).tolist() == d.tolist()


@pytest.mark.parametrize("nd", [1, 2])
@pytest.mark.parametrize("N,S,n_c,n_u", [(37, 5, 2, 3), (70, 9, 0, 4), (33, 6, 5, 1)])
def test_model_against_brute_force(N, S, n_c, n_u, nd):
    """lo and hi digit by digit in Python ints; hi 2^32 + lo == sum z_int d; finish == the correctly rounded exact sum (here
    N max(d) < 2^22: both conversions are exact) -- for both count digit counts."""
    d = ge.full_mantissa(N, S, n_c, n_u, nd, seed=N + nd)
    feats = ge.solver_features(n_c, n_u)
    X = ge.X_of(d)
    Z = ge.feature_matrix(X, feats)
    assert Z.tolist() == [[ge.z_int_scalar(float(X[i, k]), float(X[i, l])) for k, l in feats] for i in range(N)]
    lo, hi = ge.model(Z, d.Di, nd)
    A = [a.tolist() for a in ge.balanced_digits(Z)]
    Cp = [c.tolist() for c in ge.count_digits(d.Di, nd)]
    ex = ge.exact(Z, d.Di)
    assert N * int(d.Di.max()) < (1 << 22)
    for p in range(len(feats)):
        for s in range(S):
            blo = bhi = 0
            for t in range(7):
                for c in range(nd):
                    dot = sum(A[t][i][p] * Cp[c][i][s] for i in range(N))
                    if t + c < 4:
                        blo += dot * 256 ** (t + c)
                    else:
                        bhi += dot * 256 ** (t + c - 4)
            assert (int(lo[p, s]), int(hi[p, s])) == (blo, bhi)
            total = sum(int(Z[i, p]) * int(d.Di[i, s]) for i in range(N))
            assert bhi * (1 << 32) + blo == total == ex[p, s]
            got = ge.finish(lo[p:p + 1, s:s + 1], hi[p:p + 1, s:s + 1])[0, 0]
            assert got == ge.finish_scalar(blo, bhi) == float(Fraction(total, ge.TWO52))
    # and it is NOT what a float64 GEMM of the rounded products gives: a tolerance test could not see a low digit
    plain = np.stack([X[:, k] * X[:, l] for k, l in feats], axis=1).T @ d.D
    assert (plain != ge.finish(lo, hi)).mean() > 0.3


def test_finish_rounds_three_times_beyond_2_22():
    """Large sums: the conversions of hi and lo round; finish() still equals the scalar chain of correctly rounded steps."""
    rs = np.random.RandomState(9)
    lo = rs.randint(-(1 << 61), 1 << 61, size=2000, dtype=np.int64)
    hi = rs.randint(-(1 << 40), 1 << 60, size=2000, dtype=np.int64)
    got = ge.finish(lo, hi)
    assert got.tolist() == [ge.finish_scalar(a, b) for a, b in zip(lo.tolist(), hi.tolist())]


def test_dyadic_family_has_one_right_answer():
    """On dyadic data the model, the exact sum and the plain float64 GEMM coincide (lo = 0: digits 0..4 of z_int are zero)."""
    for nd in (1, 2):
        d = ge.dyadic(130, 12, 3, 4, nd, seed=3)
        feats = ge.solver_features(3, 4)
        X = ge.X_of(d)
        Z = ge.feature_matrix(X, feats)
        lo, hi = ge.model(Z, d.Di, nd)
        want = ge.dyadic_gram(d, feats)
        assert not lo.any()
        assert np.array_equal(ge.finish(lo, hi), want)
        assert np.array_equal(np.stack([X[:, k] * X[:, l] for k, l in feats], axis=1).T @ d.D, want)
        b, vdv = ge.dyadic_rhs(d)
        assert np.array_equal(X.T @ (d.D * d.V), b) and np.array_equal((d.D * d.V * d.V).sum(axis=0), vdv)
        ex = ge.exact_sums([X[:, [k for k, _ in feats]], X[:, [l for _, l in feats]]], [d.D])
        assert all(float(e) == w for e, w in zip(ex.ravel().tolist(), want.ravel().tolist()))


def test_extended_reference_keeps_the_bound_honest():
    """extended_sums lies within (N + 4) 2^-63 of the exact rational, and the limit it is used with is the derived bound less
    that error: what passes against it passes against the exact rational, and a result 400 ulps off fails both."""
    N = 300
    d = ge.full_mantissa(N, 40, 2, 3, 2, seed=3)
    ex = ge.exact_sums([d.u], [d.D, d.V])
    ref = ge.extended_sums(d.u, [d.D, d.V])
    lim = Fraction(N + 4, 1 << 63)
    for r, e in zip(ref.ravel().tolist(), ex.ravel().tolist()):
        m, x = np.frexp(r)   # (the longdouble as an exact rational: its 64-bit significand, then the exponent)
        hi = np.floor(np.ldexp(m, 32))
        lo = np.ldexp(m, 64) - np.ldexp(hi, 32)
        assert abs(((int(hi) << 32) + int(lo)) * Fraction(2) ** (int(x) - 64) - e) <= lim * e
    plain = d.u.T @ (d.D * d.V)
    live = np.array([[e > 0 for e in row] for row in ex.tolist()])
    assert ge.within_bound_extended(plain, ref, N).all() and ge.within_bound(plain, ex, N).all()
    off = plain * (1 + 400 * 2.0 ** -53)
    assert not ge.within_bound_extended(off, ref, N)[live].any() and not ge.within_bound(off, ex, N)[live].any()


def test_planted_rows_are_there():
    d = ge.full_mantissa(300, 8, 2, 4, 2, seed=1)
    Z = ge.feature_matrix(ge.X_of(d), ge.solver_features(2, 4))
    cross = set(Z[:, :2 + 0].ravel().tolist()) | set(Z.ravel().tolist())
    for k in ge.SEAM_K:
        assert (1 << k) in cross and (1 << k) - 1 in cross
    assert ge.TWO52 in cross and 0 in cross
    feats = ge.solver_features(2, 4)
    small = [p for p, (k, l) in enumerate(feats) if l == 5]
    assert int(Z[:, small].max()) < (1 << 22)     # a whole feature column on digits 0..2 alone
    assert (d.Di[150] == 0).all() and (d.Di[:, 4] == 0).all() and {128, 32639} <= set(d.Di.ravel().tolist())
    # two count digits: every 32 x 32 tile of the second plane is non-zero, every tile of the first holds negative bytes --
    # in both families, the last (ragged) row block and the last sample block included
    for fam, (N, S) in (("full", (1000, 300)), ("dyadic", (1000, 300)), ("full", (4571, 2017)), ("dyadic", (8223, 2048))):
        Di = ge.make(fam, N, S, 1, 1, 2, seed=7).Di
        p0, p1 = ge.count_digits(Di, 2)
        for plane, hit in ((p1, p1 != 0), (p0, p0 < 0)):
            pad = np.zeros(((N + 31) // 32 * 32, (S + 31) // 32 * 32), dtype=bool)
            pad[:N, :S] = hit
            tiles = pad.reshape(pad.shape[0] // 32, 32, pad.shape[1] // 32, 32).any(axis=(1, 3))
            assert tiles.all(), (fam, N, S, np.argwhere(~tiles)[:4])
        assert (p1[N - 1] != 0).any() and (p0[N - 1] < 0).any() and (p1[:, S - 1] != 0).any() and (p0[:, S - 1] < 0).any()
    d1 = ge.full_mantissa(300, 8, 0, 3, 1, seed=1)
    assert d1.Rt is None and 127 in set(d1.Di.ravel().tolist()) and d1.Di.max() == 127
    assert ge.tri(0, 0) == 0 and ge.tri(1, 2) == 4 and ge.tri(2, 2) == 5
    assert ge.solver_features(1, 2) == [(0, 1), (1, 1), (0, 2), (1, 2), (2, 2)]
    assert ge.known_features(2) == [(0, 0), (0, 1), (1, 1)]


# ---------------------------------------------------------------------------------------------- the case table
def test_describe_is_the_plan_written_down_independently(lib):
    for N in (1, 31, 32, 33, 70, 2000, 4101, 4571, 4608, 8709, 9217, 100000):
        for S in (1, 4, 33, 64, 65, 129, 255, 512, 1000, 2017, 2048):
            for n_c, n_u in ((0, 1), (4, 3), (13, 3), (13, 4), (17, 6), (0, 17), (0, 32), (16, 16), (29, 1), (28, 4), (5, 0),
                             (17, 0), (32, 0), (33, 0), (0, 33)):
                for nd in (1, 2):
                    assert ge.describe(lib, N, S, n_c, n_u, nd) == ge.expected_describe(N, S, n_c, n_u, nd), (N, S, n_c, n_u, nd)
    assert ge.describe(lib, 4571, 2017, 17, 6, 2) == "k_gram_i8_w8<2,2,6> launches=2 nsh=16 ny=16 blocks=9 last=8 tail=27 xcd=1"
    import ctypes

    buf = ctypes.create_string_buffer(160)
    for bad in ((0, 4, 1, 1, 1), (10, 0, 1, 1, 1), (10, 4, -1, 1, 1), (10, 4, 0, 0, 1), (10, 4, 60, 5, 1)):
        assert lib.dmf_gram_i8_describe(*bad, buf, len(buf)) == 1, bad
    assert lib.dmf_gram_i8_describe(10, 4, 1, 1, 1, None, 0) == 1
    assert lib.dmf_gram_i8_describe(10, 4, 1, 1, 3, buf, len(buf)) == 5 and lib.dmf_gram_i8_describe(10, 4, 1, 1, 0, buf, len(buf)) == 5


def test_the_gpu_case_table_reaches_every_class(lib):
    """The binding part of the table: every class below, for each of the four instances, is reached by some case of
    gram_exact.all_cases() as dmf_gram_i8_describe describes it."""
    reached = collections.defaultdict(set)
    feats, ways = collections.defaultdict(set), set()
    for c in ge.all_cases():
        assert c.N * c.S <= 2 * 10 ** 7, c
        text = ge.describe(lib, *c)
        assert text is not None, c
        d = ge.parse(text)
        inst, classes = ge.classes_of(c, d)
        reached[inst] |= classes
        nf = ge.n_feat(c)
        assert d["launches"] == (nf + 63) // 64
        feats[nf].add(inst)
        nct = (c.n_c + 3) // 4 * 4
        if d["xl"] == 2:
            ways.add("13..16+>=4" if 13 <= c.n_c <= 16 and c.n_u >= 4 else "17+6" if (c.n_c, c.n_u) == (17, 6)
                     else "0+17..32" if c.n_c == 0 else "other")
        if nct + c.n_u == 32:
            ways.add("image=32")
    assert set(reached) == set(ge.INSTANCES)
    for inst in ge.INSTANCES:
        assert ge.PER_INSTANCE - reached[inst] == set(), (inst, sorted(ge.PER_INSTANCE - reached[inst]))
    # feature counts: 1, below 32, 33, 63 / 65 around the seam of a launch, the largest the support rule admits
    assert 1 in feats and 33 in feats and 63 in feats and 65 in feats and any(nf < 32 for nf in feats)
    assert max(feats) == 528 and feats[528] == {(2, 1, 8), (2, 2, 6)}
    assert feats[65] == {(2, 1, 8), (2, 2, 6)} and {i[0] for i in feats[33]} == {1, 2}
    assert {"13..16+>=4", "17+6", "0+17..32", "image=32"} <= ways
    # ... and no shape has exactly 64 features, nor more than 528
    counts = {n_c * n_u + n_u * (n_u + 1) // 2 for n_c in range(0, 65) for n_u in range(1, 65)
              if ge.expected_describe(100, 64, n_c, n_u, 1) is not None}
    assert 64 not in counts and max(counts) == 528
    assert 64 not in {n * (n + 1) // 2 for n in range(64)}
