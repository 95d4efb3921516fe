"""The integer Gram (k_gram_i8_w8 + k_gram_v2_reduce + k_gram_v2_finish, csrc/dmf_kernels_gram_i8.hip) predicted bit for bit,
and the case table that reaches every class of its block loop.  A plain helper module like tests/cost_exact.py:
tests/test_gram_exact_host.py checks it without a GPU, tests/test_gpu_gram_exact.py runs it.

The model.  A feature value is z = xa * xb with xa, xb doubles in [0, 1] (a column of R_trunc or of u each).  The kernel
forms y = fma(xa, xb, 1.0): ONE rounding, half to even, of the exact 106-bit product, at the ulp of [1, 2) -- so the
mantissa of y is z_int = rint(xa xb 2^52), an integer in [0, 2^52].  z_int is written as seven balanced base-256 digits
a_0..a_6 (a_t in [-128, 127] for t < 6, a_6 in [0, 16]), a count d as one digit (d <= 127) or two (d + 128 = b0 + 256 b1,
digits b0 - 128 and b1, d <= 32639).  Every digit product is summed exactly in i32 by the matrix cores; feature digit t
and count digit c land at weight 256^(t + c).  The epilogue splits the weights at the seam 4:

    lo = sum_{t + c < 4}  256^(t + c)     sum_i a_t[i] c_c[i]
    hi = sum_{t + c >= 4} 256^(t + c - 4) sum_i a_t[i] c_c[i]         so that  hi 2^32 + lo = sum_i z_int[i] d[i]  exactly,

both summed over row ranges in 64-bit integers.  k_gram_v2_finish returns fma((double)hi, 2^32, (double)lo) * 2^-52: two
int64 -> double conversions (each correctly rounded), one FMA whose product hi 2^32 is a scaling by a power of two -- so the
FMA is ONE correctly rounded addition of two doubles, which numpy's float64 addition reproduces -- and an exact scaling by
2^-52.  `finish` is that, vectorised; test_gram_exact_host.py holds it to Python's float(int) / Fraction arithmetic.  While
N max(d) < 2^22 both conversions are exact and the entry is simply the correctly rounded exact sum.

A plain float64 (xa * xb).T @ D differs from this in most entries, so no tolerance could tell a wrong low digit from the
expected difference; equality with the model can.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple
from fractions import Fraction

import numpy as np

TWO52 = 1 << 52
NSL = 7            # balanced digits of z_int
SEAM = 4           # weights below go to lo, from here on to hi
RING = {(1, 1): 8, (1, 2): 8, (2, 1): 8, (2, 2): 6}
INSTANCES = ((1, 1, 8), (1, 2, 8), (2, 1, 8), (2, 2, 6))
MAX_FEAT = 576


def tri(k, l):
    """Row of (k <= l) in a packed Gram: dmf::tri."""
    assert k <= l
    return l * (l + 1) // 2 + k


def solver_features(n_c, n_u):
    """The (k, l) of the u-dependent V-free entries in the order of the solver's job table (JobTable::build: l-major,
    k-minor, l = n_c .. K - 1): cross (k < n_c) and uu."""
    return [(k, l) for l in range(n_c, n_c + n_u) for k in range(l + 1)]


def known_features(n_c):
    """The dense pairs of the known block in job order (l-major, k-minor, l < n_c)."""
    return [(k, l) for l in range(n_c) for k in range(l + 1)]


# ------------------------------------------------------------------------------------------------ z_int
def _mantissa(x):
    """x = M 2^(e - 53) with M an integer below 2^53 (0 for x = 0), from np.frexp."""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    M = np.ldexp(m, 53).astype(np.int64).astype(np.uint64)  # (exact: m has 53 significant bits)
    return M, e.astype(np.int64)


def z_int(xa, xb):
    """rint(xa * xb * 2^52), rounded ONCE from the exact product, half to even; int64, elementwise.  xa, xb in [0, 1]."""
    xa, xb = np.broadcast_arrays(np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64))
    assert xa.size == 0 or (xa.min() >= 0.0 and xa.max() <= 1.0 and xb.min() >= 0.0 and xb.max() <= 1.0)
    Ma, ea = _mantissa(xa)
    Mb, eb = _mantissa(xb)
    # the 106-bit product P = Ma Mb as H 2^54 + L with L < 2^54, from 26 / 27-bit halves
    m27 = np.uint64((1 << 27) - 1)
    a0, a1, b0, b1 = Ma & m27, Ma >> np.uint64(27), Mb & m27, Mb >> np.uint64(27)
    mid = a1 * b0 + a0 * b1                                   # < 2^54
    T = a0 * b0 + ((mid & m27) << np.uint64(27))              # < 2^55
    L = T & np.uint64((1 << 54) - 1)
    H = a1 * b1 + (mid >> np.uint64(27)) + (T >> np.uint64(54))
    # xa xb 2^52 = P / 2^sh with sh = 54 - ea - eb >= 52 (ea, eb <= 1)
    sh = 54 - ea - eb
    zero = (Ma == 0) | (Mb == 0)
    sh = np.where(zero, 200, sh)
    assert int(sh.min()) >= 52
    s1 = sh - 54
    one = np.uint64(1)
    # s1 in -2 .. -1: q = (H << k) | (L >> (54 - k)), remainder = low 54 - k bits of L
    k = np.clip(-s1, 1, 2).astype(np.uint64)
    qB = (H << k) | (L >> (np.uint64(54) - k))
    remB = L & ((one << (np.uint64(54) - k)) - one)
    halfB = one << (np.uint64(53) - k)
    gtB, eqB = remB > halfB, remB == halfB
    # s1 = 0: q = H, remainder L of 2^54
    half0 = np.uint64(1 << 53)
    gt0, eq0 = L > half0, L == half0
    # s1 in 1 .. 63: q = H >> s1, remainder (low s1 bits of H, L)
    c = np.clip(s1, 1, 63).astype(np.uint64)
    qA = H >> c
    remA = H & ((one << c) - one)
    halfA = one << (c - one)
    gtA = (remA > halfA) | ((remA == halfA) & (L > 0))
    eqA = (remA == halfA) & (L == 0)
    q = np.where(s1 < 0, qB, np.where(s1 == 0, H, np.where(s1 <= 63, qA, 0)))
    gt = np.where(s1 < 0, gtB, np.where(s1 == 0, gt0, np.where(s1 <= 63, gtA, False)))
    eq = np.where(s1 < 0, eqB, np.where(s1 == 0, eq0, np.where(s1 <= 63, eqA, False)))
    z = q + (gt | (eq & ((q & one) == one))).astype(np.uint64)
    z = np.where(zero, np.uint64(0), z).astype(np.int64)
    assert z.size == 0 or (int(z.min()) >= 0 and int(z.max()) <= TWO52)
    return z


def z_int_scalar(xa, xb):
    """The same for two Python floats, in rational arithmetic (round() of a Fraction rounds half to even)."""
    return round(Fraction(xa) * Fraction(xb) * TWO52)


def feature_matrix(X, feats):
    """z_int of every feature: X = [R_trunc | u] (N x K doubles), feats = [(k, l)] -> N x F int64."""
    X = np.asarray(X, dtype=np.float64)
    ks = np.array([k for k, _ in feats]), np.array([l for _, l in feats])
    return z_int(X[:, ks[0]], X[:, ks[1]])


# ------------------------------------------------------------------------------------------------ digits
def balanced_digits(z):
    """Seven balanced base-256 digits of z (int64 in [0, 2^52]): a_t in [-128, 127] for t < 6, a_6 the rest (0 .. 16);
    sum_t a_t 256^t = z.  -> list of int64 arrays."""
    r = np.asarray(z, dtype=np.int64).copy()
    out = []
    for _ in range(NSL - 1):
        a = ((r + 128) & 255) - 128
        out.append(a)
        r = (r - a) >> 8
    assert r.size == 0 or (int(r.min()) >= 0 and int(r.max()) <= 16)
    out.append(r)
    return out


def count_digits(D, nd):
    """The digit planes of integer counts: nd = 1: [d] (d <= 127); nd = 2: d + 128 = b0 + 256 b1 -> [b0 - 128, b1]
    (d <= 32639, so b1 <= 127)."""
    D = np.asarray(D, dtype=np.int64)
    assert D.size == 0 or int(D.min()) >= 0
    if nd == 1:
        assert D.size == 0 or int(D.max()) <= 127
        return [D]
    assert nd == 2 and (D.size == 0 or int(D.max()) <= 32639)
    b = D + 128
    return [(b & 255) - 128, b >> 8]


def recombine(digits):
    return sum(d.astype(object) * (256 ** t) for t, d in enumerate(digits))


def _exact_matmul(A, B):
    """A.T @ B for small-integer matrices through float64 BLAS; exact because every partial sum stays below 2^53."""
    amax = int(np.abs(A).max()) if A.size else 0
    bmax = int(np.abs(B).max()) if B.size else 0
    assert amax * bmax * A.shape[0] < (1 << 53)
    return np.rint(A.T.astype(np.float64) @ B.astype(np.float64)).astype(np.int64)


def model(Z, D, nd):
    """-> (lo, hi), F x S int64: what the slabs of k_gram_i8_w8 sum to (see the module docstring)."""
    A, Cd = balanced_digits(Z), count_digits(D, nd)
    F, S = Z.shape[1], D.shape[1]
    # (a digit product is below 2^14 N, a weight at most 256^3, at most 7 terms each: 64-bit integers hold them, as the
    # kernels' do)
    assert 7 * (1 << 14) * Z.shape[0] * (256 ** 3) < (1 << 62)
    lo, hi = np.zeros((F, S), dtype=np.int64), np.zeros((F, S), dtype=np.int64)
    for t, a in enumerate(A):
        for c, cd in enumerate(Cd):
            prod = _exact_matmul(a, cd)
            if t + c < SEAM:
                lo += prod * (256 ** (t + c))
            else:
                hi += prod * (256 ** (t + c - SEAM))
    return lo, hi


def finish(lo, hi):
    """k_gram_v2_finish: fma((double)hi, 2^32, (double)lo) * 2^-52 -- three correctly rounded operations; the FMA's product is
    a power-of-two scaling, so it is one rounded addition."""
    h = np.asarray(hi, dtype=np.int64).astype(np.float64) * 4294967296.0
    return (h + np.asarray(lo, dtype=np.int64).astype(np.float64)) * 2.0 ** -52


def finish_scalar(lo, hi):
    """The same through Python's correctly rounded int -> float and Fraction -> float."""
    return float(Fraction(float(int(hi))) * (1 << 32) + Fraction(float(int(lo)))) * 2.0 ** -52


def exact(Z, D):
    """sum_i z_int[i, p] d[i, s] as Python ints (F x S object array), from three 18-bit pieces of z_int."""
    Z = np.asarray(Z, dtype=np.int64)
    D = np.asarray(D, dtype=np.int64)
    m = (1 << 18) - 1
    out = np.zeros((Z.shape[1], D.shape[1]), dtype=object)
    for piece in range(3):
        out += _exact_matmul((Z >> (18 * piece)) & m, D).astype(object) * (1 << (18 * piece))
    return out


def want_gram(X, feats, D, nd):
    """The rows the integer route must deliver for these features: finish(model), F x S float64."""
    return finish(*model(feature_matrix(X, feats), D, nd))


# ------------------------------------------------------------------------------------------------ data
Data = namedtuple("Data", "family V D Rt u Vi Di Ri Ui nd")


def counts(rs, N, S, nd, hi=32639):
    """Poisson-like integer counts with about 10 % zeros, one all-zero row and one all-zero sample (row N // 2, sample
    S // 2), the planted values 127 (nd = 1) or 128 and 32639 (nd = 2), and -- outside that row and sample -- the last row
    and the last sample non-zero and different from their neighbours.  nd = 2: about 4 % of the cells, spread over all rows
    and samples (the last row and the last sample included), are uniform in [128, hi], so that every 32 x 32 tile of the
    second digit plane b1 = (d + 128) >> 8 is non-zero and every tile of the first holds negative bytes b0 - 128."""
    assert N >= 6 and S >= 4 and 128 < hi <= 32639
    top = 127 if nd == 1 else 32639
    half = 13 if nd == 1 else 41   # (the sum of two uniform draws: a peaked distribution at a fraction of Poisson's cost)
    Di = (rs.randint(0, half, size=(N, S)) + rs.randint(0, half, size=(N, S))).astype(np.int64)
    Di[rs.rand(N, S) < 0.1] = 0
    if nd == 2:
        big = rs.rand(N, S) < 0.04
        Di[big] = rs.randint(128, hi + 1, size=int(big.sum()))
    Di[N - 1] = 1 + (np.arange(S) % 7)     # the last row ...
    Di[:, S - 1] = 2 + (np.arange(N) % 5)  # ... and the last sample weigh something
    if nd == 2:
        Di[N - 1, 3::5] = 128 + (np.arange(S)[3::5] * 977) % (hi - 127)
        Di[4::9, S - 1] = 128 + (np.arange(N)[4::9] * 613) % (hi - 127)
    same = Di[:, S - 1] == Di[:, S - 2]
    Di[same, S - 1] += 1
    same = Di[N - 1] == Di[N - 2]
    Di[N - 1, same] += 1
    Di[N // 2, :] = 0                      # an all-zero row
    Di[:, S // 2] = 0                      # an all-zero sample
    Di[0, 0] = top
    Di[N - 1, S - 1] = top
    if nd == 2:
        Di[1, 1] = 128
        Di[N - 2, S - 1] = 128
    rows, cols = np.arange(N) != N // 2, np.arange(S) != S // 2
    assert Di.max() == top and Di.min() == 0 and (Di[N - 1, cols] > 0).all() and (Di[rows, S - 1] > 0).all()
    assert (Di[rows, S - 1] != Di[rows, S - 2]).all() and (Di[N - 1, cols] != Di[N - 2, cols]).all()
    assert not Di[N // 2].any() and not Di[:, S // 2].any()
    return Di


def dyadic(N, S, n_c, n_u, nd, seed):
    """Rt = Ri / 16, u = Ui / 16, V = Vi / 1024, integer counts: every product and every partial sum, in any order, of
    sum R R d (units 2^-8), sum R d v (2^-14) and sum d v^2 (2^-20) is representable -- fewer than 2^53 units in all, asserted
    -- so b_u, b_k, v^T D v and every FP64 Gram kernel have one right answer too."""
    rs = np.random.RandomState(seed)
    K = n_c + n_u
    Xi = rs.randint(0, 17, size=(N, K)).astype(np.int64)
    Xi[N - 1] = 16 - (np.arange(K) % 3)
    Vi = rs.randint(0, 1025, size=(N, S)).astype(np.int64)
    Di = counts(rs, N, S, nd, hi=8000)   # (high counts capped so that the sums below stay under 2^53 units)
    assert int(Di.sum()) * (1 << 20) < (1 << 53), "the sums of the dyadic family must stay below 2^53 units"
    X = Xi / 16.0
    return Data("dyadic", Vi / 1024.0, Di.astype(np.float64), np.ascontiguousarray(X[:, :n_c]) if n_c else None,
                np.ascontiguousarray(X[:, n_c:]) if n_u else None, Vi, Di, Xi[:, :n_c], Xi[:, n_c:], nd)


def dyadic_gram(d, feats):
    """The one right answer of a feature row on dyadic data: sum_i Xi_k Xi_l d / 256 (exact: fewer than 2^53 units)."""
    Xi = np.hstack([d.Ri, d.Ui])
    Z = np.stack([Xi[:, k] * Xi[:, l] for k, l in feats], axis=1)
    return _exact_matmul(Z, d.Di) / 256.0


def dyadic_rhs(d):
    """b rows (one per column of [Rt | u]) and v^T D v on dyadic data: sum X d v / 2^14, sum d v^2 / 2^20."""
    Xi = np.hstack([d.Ri, d.Ui])
    DV = d.Di * d.Vi
    assert int(DV.max()) * 16 * d.Di.shape[0] < (1 << 53)
    b = _exact_matmul(Xi, DV) / 16384.0
    vdv = (d.Di * d.Vi * d.Vi).sum(axis=0)
    assert int(vdv.max()) < (1 << 53)
    return b, vdv / float(1 << 20)


SEAM_K = (8, 16, 24, 31, 32, 40, 48)


def planted_values():
    """Doubles v with v 2^52 an integer whose digits carry: 1 (digit 6 = 16), 0, 2^-60 (rounds to 0), and 2^k - 1, 2^k for
    the k that straddle the balanced digits and the lo / hi seam."""
    vals = [1.0, 0.0, 2.0 ** -60]
    for k in SEAM_K:
        vals += [((1 << k) - 1) / float(TWO52), (1 << k) / float(TWO52)]
    return vals


def full_mantissa(N, S, n_c, n_u, nd, seed):
    """Rt, u, V uniform doubles in [0, 1] plus planted rows.  A planted row has a 'unit' factor -- every R_trunc entry, or
    u's first column without known types -- equal to 1, so that the feature values ARE the other factor: the values of
    planted_values() rotate through the u columns.  Two more rows have the unit factor 1/2 and u = (2 m + 1) 2^-52 with m
    even and odd: the product lies exactly on a half and ties to even, both parities.  With at least two unknown types the
    last u column is below 2^-30 throughout: z_int < 2^22, only digits 0..2 carry the result."""
    rs = np.random.RandomState(seed)
    K = n_c + n_u
    X = rs.rand(N, K)
    vals = planted_values()
    n_pl = min(len(vals), max(N // 2 - 2, 1))
    rows = np.unique(np.linspace(0, N - 1, n_pl).astype(int))  # spread over the blocks, the first and last row included
    j0 = 0 if n_c else 1   # (without known types u's column 0 is the unit factor)
    for r, i in enumerate(rows):
        X[i, :n_c if n_c else 1] = 1.0
        for j in range(j0, n_u):
            X[i, n_c + j] = vals[(r + j) % len(vals)]
    ties = [i for i in (1, N - 2) if i not in set(rows.tolist())]
    for t, i in enumerate(ties):
        X[i, :n_c if n_c else 1] = 0.5
        for j in range(j0, n_u):
            m = 2 * int(rs.randint(1, 1 << 40)) + (t + j) % 2   # parity alternates over rows and columns
            X[i, n_c + j] = (2 * m + 1) / float(TWO52)
    if n_u >= 2:
        X[:, K - 1] = rs.rand(N) * 2.0 ** -31
        X[rows[0], K - 1] = 2.0 ** -60
    V = rs.rand(N, S)
    Di = counts(rs, N, S, nd)
    return Data("full", V, Di.astype(np.float64), np.ascontiguousarray(X[:, :n_c]) if n_c else None,
                np.ascontiguousarray(X[:, n_c:]) if n_u else None, None, Di, None, None, nd)


def make(family, N, S, n_c, n_u, nd, seed):
    return {"dyadic": dyadic, "full": full_mantissa}[family](N, S, n_c, n_u, nd, seed)


def X_of(d):
    return np.hstack([a for a in (d.Rt, d.u) if a is not None])


# ------------------------------------------------------------------------------------------------ exact rationals (small shapes)
def _to_ints(x):
    """x (non-negative doubles) = ints 2^-k: -> (object array of Python ints, k)."""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(x)
    M = np.ldexp(m, 53).astype(np.int64)
    nz = M != 0
    k = max(int(53 - e[nz].min()), 0) if nz.any() else 0
    sh = np.where(nz, e.astype(np.int64) + (k - 53), 0)
    assert int(sh.min()) >= 0
    return M.astype(object) << sh.astype(object), k


def exact_sums(factors, W):
    """sum_i prod_f factors[f][i, p] * W[i, s] in exact rational arithmetic: factors = list of N x F double arrays,
    W = list of N x S double arrays multiplied elementwise (counts, meth_frequency).  -> F x S object array of Fractions.
    Every term is non-negative here, so this is also the sum of the |terms| that the rounding-error bounds scale with."""
    A, ka = None, 0
    for f in factors:
        fi, k = _to_ints(f)
        A, ka = (fi if A is None else A * fi), ka + k
    B, kb = None, 0
    for w in W:
        wi, k = _to_ints(w)
        B, kb = (wi if B is None else B * wi), kb + k
    G = A.T.dot(B)
    den = 1 << (ka + kb)
    return np.array([Fraction(int(g), den) for g in G.ravel().tolist()], dtype=object).reshape(G.shape)


def within_bound(got, want, N):
    """|got - exact| <= (N + 4) 2^-53 sum |term|, entry by entry, in rational arithmetic (terms are non-negative: the sum
    of their magnitudes is `want` itself).  Derivation: test_gpu_gram_exact.py's docstring.  -> bool array."""
    g = np.asarray(got, dtype=np.float64)
    out = np.empty(g.shape, dtype=bool)
    lim = Fraction(N + 4, 1 << 53)
    for idx in np.ndindex(g.shape):
        w = want[idx]
        out[idx] = abs(Fraction(float(g[idx])) - w) <= lim * w
    return out


def extended_sums(A, W):
    """sum_i A[i, p] * prod_w W[w][i, s] in x87 extended precision (64-bit significands), for the shapes where the exact
    rational costs too much: -> F x S longdouble.  At most three roundings per term and N - 1 per sum, each 2^-64 relative
    to a value that the (non-negative) total bounds: |result - exact| <= (N + 3) 2^-64 sum |term|."""
    ld = np.longdouble
    assert np.finfo(ld).nmant >= 63, "this platform's long double is no wider than double: no cheap accurate reference"
    Wl = W[0].astype(ld)
    for w in W[1:]:
        Wl = Wl * w.astype(ld)
    A = np.asarray(A, dtype=np.float64)
    return np.stack([(A[:, p, None].astype(ld) * Wl).sum(axis=0) for p in range(A.shape[1])])


def within_bound_extended(got, ref, N):
    """The same bound against extended_sums' reference, with that reference's own error taken OFF the limit:
    |got - ref| <= (N + 4) (2^-53 - 2^-62) ref implies |got - exact| <= (N + 4) 2^-53 exact, since |ref - exact| <=
    (N + 4) 2^-63 exact.  The comparison itself runs in extended precision (its roundings, 2^-64 relative, sit inside the
    2^-63 of slack that remains).  -> bool array."""
    ld = np.longdouble
    lim = ld(N + 4) * (ld(2.0) ** -53 - ld(2.0) ** -62)
    return np.abs(np.asarray(got, dtype=np.float64).astype(ld) - ref) <= lim * ref


# ------------------------------------------------------------------------------------------------ the plan, from Python
def describe(lib, N, S, n_c, n_u, nd):
    """dmf_gram_i8_describe, or None where it answers DMF_ERR_UNSUPPORTED."""
    buf = ctypes.create_string_buffer(160)
    st = lib.dmf_gram_i8_describe(N, S, n_c, n_u, nd, buf, len(buf))
    if st == 5:
        return None
    assert st == 0, (st, N, S, n_c, n_u, nd)
    return buf.value.decode()


def parse(text):
    """'k_gram_i8_w8<2,2,6> launches=3 nsh=16 ...' -> dict with xl, nd, ring and the integer fields."""
    head, *fields = text.split()
    assert head.startswith("k_gram_i8_w8<") and head.endswith(">"), text
    xl, nd, ring = (int(x) for x in head[len("k_gram_i8_w8<"):-1].split(","))
    out = {"xl": xl, "nd": nd, "ring": ring}
    out.update({k: int(v) for k, v in (f.split("=") for f in fields)})
    return out


def expected_describe(N, S, n_c, n_u, nd):
    """gram_i8_plan written down independently (None: unsupported)."""
    SD = (S + 63) // 64 * 64
    SB = SD // 32
    nct = (n_c + 3) // 4 * 4
    nf = n_c * n_u + n_u * (n_u + 1) // 2 if n_u else n_c * (n_c + 1) // 2
    nsh = (SB + 3) // 4
    want = max(256 // nsh, 1)
    rpw = max(((N + want - 1) // want + 31) // 32 * 32, 32)
    ny = (N + rpw - 1) // rpw
    if nct + n_u > 32 or not 1 <= nf <= MAX_FEAT or nd not in (1, 2) or rpw * 128 * 128 * nd >= 1 << 31:
        return None
    xl = 2 if nct + n_u > 16 else 1
    return (f"k_gram_i8_w8<{xl},{nd},{RING[(xl, nd)]}> launches={(nf + 63) // 64} nsh={nsh} ny={ny} blocks={rpw // 32} "
            f"last={(N - (ny - 1) * rpw + 31) // 32} tail={N % 32} xcd={int(ny % 8 == 0)}")


GramCase = namedtuple("GramCase", "N S n_c n_u nd")


def n_feat(c):
    return c.n_c * c.n_u + c.n_u * (c.n_u + 1) // 2


# Feature shapes per row-image width: XL = 1 (padded n_c + n_u <= 16) and XL = 2.
NARROW = (4, 3)   # 18 features, n_u odd
WIDE = (14, 3)    # padded 16 + 3 = 19 doubles per row: 48 features, n_u odd


def wrap_cases():
    """The steady state of the block loop, per instance: ring - 1, ring, ring + 1 and >= 2 ring + 1 blocks per range, a last
    range with fewer blocks, N % 32 in {0, 1, 31} with N and n_u odd, ny = 16 (the XCD reordering) and ny % 8 != 0.  Blocks
    per range grow with N S, so these stay below 2 10^7 elements only at many samples (S ~ 2048: 16 ranges of N / 16 rows)."""
    cases = []
    for xl in (1, 2):
        n_c, n_u = NARROW if xl == 1 else WIDE
        for nd in (1, 2):
            if RING[(xl, nd)] == 8:
                shapes = [(3361, 2048),    # 7 blocks, last 1, N % 32 = 1
                          (4608, 2048),    # 9, last 9, N % 32 = 0
                          (4571, 2017),    # 9, last 8, S odd
                          (8223, 2048),    # 17, last 2, N % 32 = 31
                          (9217, 1000)]    # 10 blocks of 32 ranges: ny = 29, no XCD reordering
            else:
                shapes = [(2401, 2048),    # 5 blocks, last 1, N % 32 = 1
                          (3072, 2048),    # 6, last 6, N % 32 = 0
                          (3525, 2017),    # 7, last 6
                          (6303, 2048),    # 13, last 2, N % 32 = 31
                          (7169, 1000)]    # 8 blocks, ny = 29
            cases += [GramCase(N, S, n_c, n_u, nd) for N, S in shapes]
    return cases


def small_cases():
    """Few blocks per range (1, 2, 3: the prologue's clamps and the repeat DMAs), every sample-side edge, per instance:
    S < 32, S = 1 mod 64, SB % 4 == 2 (two idle sample waves), ny < 16, = 16, > 16.  (8197 x 512: 5 blocks, last range 2;
    4799 x 512: 3 blocks in every range, N % 32 = 31.)"""
    cases = []
    for xl in (1, 2):
        n_c, n_u = NARROW if xl == 1 else WIDE
        for nd in (1, 2):
            shapes = [(70, 4), (33, 33), (2000, 255), (4101, 129), (8197, 512), (4799, 512), (12289, 65), (511, 200)]
            cases += [GramCase(N, S, n_c, n_u, nd) for N, S in shapes]
    return cases


def feature_cases():
    """Feature counts 1, < 32 (feature half 1 idle), 33, 63, 65 (a second launch with one feature), the largest the support
    rule admits (0 + 32: 528; 576 = kMaxFeat is not reached by any n_c + n_u within 32 padded doubles), XL = 2 by each of
    its ways (n_c = 13..16 with n_u >= 4, 17 + 6, 0 + 17..32), a row image of exactly 32 doubles (16 + 16, 0 + 32)."""
    shapes = [
        (0, 1, 70, 4), (0, 1, 2000, 255),       # 1 feature
        (1, 1, 33, 33),                         # 2
        (3, 6, 4101, 129),                      # 18 + 21 = 39 (> 32: both halves), n_u even
        (4, 6, 511, 200),                       # 24 + 21 = 45
        (0, 7, 333, 70),                        # 28 < 32
        (5, 5, 99, 40), (12, 2, 333, 70),       # 40; 27
        (10, 3, 257, 130),                      # 36; padded 12 + 3
        (3, 8, 300, 64), (6, 6, 161, 96),       # 24 + 36 = 60; 36 + 21 = 57
        (13, 4, 300, 64), (16, 4, 161, 96),     # XL = 2 from 16 padded known types: 62, 74 features
        (0, 10, 257, 130),                      # 55
        (9, 5, 99, 40),                         # 45 + 15 = 60
        (27, 2, 99, 40), (5, 8, 99, 40),        # 57; 40 + 36 = 76
        (0, 11, 161, 96),                       # 66
        (6, 7, 333, 70),                        # 42 + 28 = 70
        (8, 4, 70, 36),                         # 32 + 10 = 42
        (28, 1, 70, 36),                        # 28 + 1 = 29, row image 28 + 1
        (7, 6, 300, 64),                        # 42 + 21 = 63: the last slot of a launch but one
        (17, 6, 257, 130),                      # 102 + 21 = 123: two launches
        (0, 17, 161, 96), (0, 32, 130, 70),     # 153; 528 = nine launches (the last with 16), row image of exactly 32 doubles
        (16, 16, 130, 70),                      # 256 + 136 = 392, row image of exactly 32 doubles
    ]
    extra = []
    for n_c, n_u, N, S in shapes:
        for nd in (1, 2):
            extra.append(GramCase(N, S, n_c, n_u, nd))
    return extra


def exact_count_cases():
    """Feature counts at the seam of a launch (64 features): 33 (one feature in the second half), 63, 65 (a second launch
    with ONE feature, p0 = 64).  Exactly 64 is reached by no shape: n_c n_u + n_u (n_u + 1) / 2 = 64 has no solution with
    n_u <= 11 (n_u = 1: n_c = 63; 4 n_c = 54; 5 n_c = 49; 7 n_c = 36; 8 n_c = 28; 9 n_c = 19; 10 n_c = 9; n_u = 2, 6: odd;
    n_u = 3: 3 n_c = 58), and the known block's n_c (n_c + 1) / 2 skips it too (55, 66); test_gram_exact_host.py asserts this.
    63 and 65 stand on either side."""
    return [GramCase(99, 40, 15, 2, 1), GramCase(161, 96, 9, 3, 2),           # 33: XL = 2 and XL = 1
            GramCase(99, 40, 19, 3, 2), GramCase(70, 36, 19, 3, 1),           # 63, XL = 2
            GramCase(161, 96, 10, 5, 1), GramCase(333, 70, 10, 5, 2)]         # 65


def all_cases():
    seen, out = set(), []
    for c in wrap_cases() + small_cases() + feature_cases() + exact_count_cases():
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def classes_of(c, d):
    """The classes of section 'what the table reaches' that a case with parsed describe `d` belongs to, as strings."""
    ring, inst = d["ring"], (d["xl"], d["nd"], d["ring"])
    out = set()
    for nb in {d["blocks"], d["last"]} if d["ny"] > 1 else {d["last"]}:
        for name, hit in (("nb=1", nb == 1), ("nb=2", nb == 2), ("nb=3", nb == 3), ("nb=ring-1", nb == ring - 1),
                          ("nb=ring", nb == ring), ("nb=ring+1", nb == ring + 1), ("nb>=2ring+1", nb >= 2 * ring + 1)):
            if hit:
                out.add(name)
    if d["ny"] > 1 and d["last"] < d["blocks"]:
        out.add("last<blocks")
    odd = c.N % 2 == 1 and c.n_u % 2 == 1
    if d["tail"] == 0:
        out.add("tail=0")
    if d["tail"] == 1 and odd:
        out.add("tail=1,odd")
    if d["tail"] == 31 and odd:
        out.add("tail=31,odd")
    SB = (c.S + 63) // 64 * 2
    if SB % 4 == 2:
        out.add("idle-sample-waves")
    if c.S % 64 == 1:
        out.add("S=1mod64")
    if c.S < 32:
        out.add("S<32")
    out.add("xcd=1" if d["xcd"] else "xcd=0")
    ny = d["ny"]
    out.add("ny<16" if ny < 16 else "ny=16" if ny == 16 else "ny>16,ny%16!=0" if ny % 16 else "ny%16==0")
    return inst, out


PER_INSTANCE = {"nb=1", "nb=2", "nb=3", "nb=ring-1", "nb=ring", "nb=ring+1", "nb>=2ring+1", "last<blocks", "tail=0", "tail=1,odd",
                "tail=31,odd", "idle-sample-waves", "S=1mod64", "S<32", "xcd=1", "xcd=0", "ny<16", "ny=16", "ny>16,ny%16!=0"}
