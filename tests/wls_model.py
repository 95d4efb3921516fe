"""The reference-based regression as its kernels (csrc/dmf_kernels_wls.hip) must deliver it: the first moments of
k_wls_moments / k_wls_reduce as exact sums, a restatement of k_nnls_intercept's active-set loop that COUNTS what the loop
does, and the case tables of tests/test_wls_model_host.py (no GPU) and tests/test_gpu_wls_exact.py.  A plain helper module
like tests/cm_exact.py and tests/fp64_rowpass.py.

The moments.  mom is (2 K + 2) x S: m_k = sum_i d R_k, r_k = sum_i d t R_k, sw = sum_i d, st = sum_i d t per sample, t = v
or d v, R = [R_trunc | u].  On the DYADIC family -- integer counts d, integer methylated counts x <= d with v = x / d,
R_trunc and u multiples of 2^-8 in [0, 1], and every d a power of two (or zero) so that v is dyadic and d v = x holds in
f64 as well -- every term is a non-negative multiple of 2^-8, so every partial sum in any order is at most the whole sum:
where the largest entry of the table, in units of 2^-8, is below 2^53 (`dyadic_headroom`) every product, fma and addition of
either kernel form is exact and the table has ONE right answer, `exact_moments(...).table`, computed in integers.
On general inputs `exact_moments` gives an x87 extended sum and the sum of the absolute values of the terms; a kernel
result passes through `moment_terms(N)` rounded operations -- the fmas of the rows one lane accumulates, the three additions
of the other waves, the additions of the slabs a thread group takes and the three of the other groups -- each of which
commits at most 2^-53 of a quantity that the absolute sum bounds, and a handful more inside a term (v = x / d rounded, the
products d v and d (d v), or x in place of d v on the u16 form): (n_terms + 8) 2^-53 sum|terms|, the chain-of-fma bound of
tests/test_gpu_momentum.py.  The extended sum's own error, (N + 4) 2^-64 sum|terms|, is taken off the limit.

The solver.  `active_set_events(A, b)` follows the kernel line by line -- enter the largest positive dual, lowest index on
a tie; reject a candidate whose own coefficient comes out non-positive; step back by the smallest ratio, lowest passive
ordinal on a tie; pivots against K 2^-52 A_jj; at most 3 K factorisations -- in float64 without fused multiply-adds, so its
numbers agree with the kernel's to rounding only.  It is used to CHOOSE and CERTIFY inputs (which branch a system reaches)
and for the status of systems that are singular by twenty orders of magnitude; the expected coefficients are always
scipy.optimize.nnls's.

Searches (tests/test_wls_model_host.py documents how to repeat them): over 200 200 random systems of the recipes below (K = 2
.. 12, the correlated recipe and a near-collinear one) the model counted NO rejected candidate -- in exact arithmetic the
entering variable's own coefficient is positive, so a rejection is a rounding-only event -- and NO emptied passive set (the
variable that has just entered moves from zero towards a positive value, so it survives the step back unless its ratio
rounds to zero); neither has a case.  The 3 K cap has no known reachable input either.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

# ------------------------------------------------------------------------------------------------ the moments' plan
ROWS_PER_WG = 16     # four waves, four rows in flight each
GRID_MAX = 512       # wls_moments_grid's cap: a second trip of the grid-stride loop beyond 8192 rows
SLICE = 16           # columns of R per grid.z slice


def moments_grid(N):
    return max(1, min(GRID_MAX, (N + ROWS_PER_WG - 1) // ROWS_PER_WG))


def moments_trips(N):
    """Trips of the grid-stride loop of the busiest wave."""
    per_trip = ROWS_PER_WG * moments_grid(N)
    return (N + per_trip - 1) // per_trip


def moment_terms(N):
    """Rounded operations behind one entry of the table (module docstring)."""
    g = moments_grid(N)
    return 4 * moments_trips(N) + 3 + (g + 3) // 4 + 3


Moments = namedtuple("Moments", "table abs_sum exact")


def _methylated_counts(V, D):
    X = np.rint(V * D)
    assert np.array_equal(X, V * D), "v d is not an integer: not the dyadic family"
    return X.astype(np.int64)


def _int_dot(Ri, W):
    """Ri^T W in int64 for non-negative integer arrays, Ri <= 256: row chunks short enough that a chunk's sums stay below 2^52
    WHATEVER the data (256 max(W) rows <= 2^52), so the float64 matrix product of a chunk is exact in any order; the chunks
    are added as integers."""
    assert Ri.min() >= 0 and Ri.max() <= 256 and W.min() >= 0
    step = max(1, (1 << 44) // max(int(W.max()), 1))
    out = np.zeros((Ri.shape[1], W.shape[1]), dtype=np.int64)
    for a in range(0, Ri.shape[0], step):
        out += np.rint(Ri[a:a + step].T.astype(np.float64) @ W[a:a + step].astype(np.float64)).astype(np.int64)
    return out


def exact_moments(V, D, R, target):
    """The (2 K + 2) x S table of [V, D, R = [R_trunc | u]].  Dyadic family (R a multiple of 2^-8, D integer powers of two
    or zero, V D integer): integer sums, exact=True, table exact float64.  Otherwise: np.longdouble sums, exact=False, and
    abs_sum = the sums of the absolute values of the terms (float64, rounded up by a relative 2^-50)."""
    assert target in ("v", "dv")
    V, D, R = np.asarray(V, dtype=np.float64), np.asarray(D, dtype=np.float64), np.asarray(R, dtype=np.float64)
    K = R.shape[1]
    Ri = R * 256.0
    dyadic = (np.array_equal(Ri, np.rint(Ri)) and np.array_equal(D, np.rint(D)) and
              np.array_equal(V * D, np.rint(V * D)) and bool(np.all((D == 0) | (np.frexp(D)[0] == 0.5))))
    if dyadic:
        Di, Xi, Ri = D.astype(np.int64), _methylated_counts(V, D), Ri.astype(np.int64)
        Wt = Di * Xi if target == "dv" else Xi
        units = np.vstack([_int_dot(Ri, Di), _int_dot(Ri, Wt), 256 * Di.sum(axis=0, keepdims=True),
                           256 * Wt.sum(axis=0, keepdims=True)])
        assert units.min() >= 0 and int(units.max()) < 1 << 62
        return Moments(units.astype(np.float64) / 256.0, units.astype(np.float64) / 256.0, True)
    ld = np.longdouble
    Dl, Vl, Rl = D.astype(ld), V.astype(ld), R.astype(ld)
    Wt = Dl * (Dl * Vl) if target == "dv" else Dl * Vl
    table = np.vstack([Rl.T @ Dl, Rl.T @ Wt, Dl.sum(axis=0, keepdims=True), Wt.sum(axis=0, keepdims=True)])
    Ra = np.abs(Rl)
    abs_sum = np.vstack([Ra.T @ np.abs(Dl), Ra.T @ np.abs(Wt), np.abs(Dl).sum(axis=0, keepdims=True),
                         np.abs(Wt).sum(axis=0, keepdims=True)])
    assert table.shape == (2 * K + 2, V.shape[1])
    return Moments(table, (abs_sum * (1 + ld(2.0) ** -50)).astype(np.float64), False)


def dyadic_headroom(V, D, R, target):
    """log2 of the room left under 2^53 by the largest entry of the exact table in units of 2^-8 (positive: exact)."""
    m = exact_moments(V, D, R, target)
    assert m.exact
    return 53.0 - float(np.log2(max(m.table.max() * 256.0, 1.0)))


def moment_ratio(got, m, N):
    """max over the table of |got - reference| / limit for general inputs (at most 1 passes)."""
    assert not m.exact
    ld = np.longdouble
    limit = ((moment_terms(N) + 8) * ld(2.0) ** -53 - (N + 4) * ld(2.0) ** -64) * m.abs_sum.astype(ld)
    err = np.abs(np.asarray(got).astype(ld) - m.table)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(limit > 0, err / limit, np.where(err == 0, 0.0, np.inf))
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------ the moments' cases
# form: "u16" (the problem carries X16 / D16), "f64_flag" (it does, f64_arrays=True), "f64_plain" (it does not: one sample,
# more than 48 known types, or a planted count beyond the u16 range)
MomentCase = namedtuple("MomentCase", "N S n_c n_u target form hole")

MOMENT_N = (1, 3, 4, 15, 16, 17, 8191, 8192, 8193, 16385)
MOMENT_S = (1, 63, 64, 65, 128, 129)
MOMENT_SPLITS = ((1, 0), (15, 0), (16, 0), (17, 0), (32, 0), (33, 0), (48, 0), (49, 0), (64, 0),   # the slice boundaries
                 (15, 2), (16, 1), (17, 3),                                                         # the split in / across a slice
                 (0, 3), (0, 17),                                                                    # no known columns
                 (48, 1), (48, 16))                                                                  # K = 49, 64 with integer copies
MOMENT_FORMS = ("u16", "f64_flag", "f64_plain")
MAX_CASE_ELEMENTS = 16385 * 129 * 64


def moment_case_allowed(c):
    if c.form != "f64_plain" and (c.S < 2 or c.n_c > 48):
        return False  # no integer copies to read / to ignore
    if c.hole and c.N < 15:
        return False
    # (keeps the suite quick: the big row counts meet the wide shapes once, in the corner case below)
    return c.N * c.S * (c.n_c + c.n_u) <= MAX_CASE_ELEMENTS // 8


def _moment_cases():
    """Every value of every dimension with every form and with both targets (pairs with form / target, not the full
    pairwise table, which the 16 splits x 10 row counts alone would put at 160 cases), chosen greedily from the allowed
    product in a fixed order, plus the corner 16385 x 129 x 64."""
    import itertools

    dims = (MOMENT_N, MOMENT_S, MOMENT_SPLITS, ("v", "dv"), MOMENT_FORMS, (False, True))
    cands = [MomentCase(N, S, sp[0], sp[1], t, f, h) for N, S, sp, t, f, h in itertools.product(*dims)]
    cands = [c for c in cands if moment_case_allowed(c)]

    def pairs(c):
        vals = (("N", c.N), ("S", c.S), ("split", (c.n_c, c.n_u)), ("hole", c.hole))
        out = {(v, ("form", c.form)) for v in vals} | {(v, ("target", c.target)) for v in vals}
        out.add((("form", c.form), ("target", c.target)))
        return out

    want = set().union(*(pairs(c) for c in cands))
    chosen = [MomentCase(16385, 129, 48, 16, "dv", "u16", True)]
    want -= pairs(chosen[0])
    while want:
        best = max(cands, key=lambda c: len(pairs(c) & want))  # (max keeps the first of equals: deterministic)
        chosen.append(best)
        want -= pairs(best)
    return tuple(chosen)


MOMENT_CASES = _moment_cases()
# general real inputs: second and third trip, ragged rows, the slice boundaries, both forms
GENERAL_MOMENT_CASES = (
    MomentCase(17, 65, 17, 3, "dv", "u16", False), MomentCase(8193, 5, 16, 1, "v", "u16", False),
    MomentCase(16385, 3, 33, 0, "dv", "u16", False), MomentCase(8193, 1, 6, 2, "dv", "f64_plain", False),
    MomentCase(16385, 64, 49, 0, "v", "f64_plain", False), MomentCase(4099, 129, 15, 2, "v", "f64_flag", False),
)


def moment_case_id(c):
    return f"{c.N}x{c.S}-{c.n_c}+{c.n_u}-{c.target}-{c.form}" + ("-hole" if c.hole else "")


def dyadic_moment_data(c, seed=0):
    """(V, D int64, Rt or None, u or None) of a dyadic case: counts in {0, 1, 2, 4, 8} (one 256 where the problem keeps
    integer copies: two digit planes), x uniform in 0 .. d, R_trunc and u multiples of 2^-8 in [0, 1] with both ends
    present, a block of rows without coverage where the case asks for one, and for "f64_plain" on a shape that would carry
    integer copies a single count of 2^16 with x = 3."""
    rs = np.random.RandomState(1000 + seed)
    N, S, K = c.N, c.S, c.n_c + c.n_u
    D = rs.choice(np.array([0, 1, 2, 4, 8], dtype=np.int64), size=(N, S), p=[0.1, 0.2, 0.2, 0.25, 0.25])
    D[0] = np.maximum(D[0], 1)  # every sample has weight
    if c.hole:
        a = N // 3
        D[a:a + max(1, min(N // 4, 40))] = 0
    if N >= 2 and c.form != "f64_plain":
        D[N - 1, S - 1] = 256
    X = rs.randint(0, 1 << 30, size=(N, S)) % (D + 1)
    if c.form == "f64_plain" and S >= 2 and c.n_c <= 48:
        D[N // 2, S // 2], X[N // 2, S // 2] = 1 << 16, 3
    V = np.where(D > 0, X / np.maximum(D, 1), 0.0)
    R = rs.randint(0, 257, size=(N, K)) / 256.0
    R[rs.randint(0, N, size=K), np.arange(K)] = 1.0
    if N > 1:
        R[(rs.randint(0, N, size=K) + 1) % N, np.arange(K)] = 0.0
    Rt = np.ascontiguousarray(R[:, :c.n_c]) if c.n_c else None
    u = np.ascontiguousarray(R[:, c.n_c:]) if c.n_u else None
    return V, D, Rt, u


def general_moment_data(c, seed=0):
    """Uniform R_trunc and u, Poisson depth 50, binomial methylated counts (a count of 70000 planted for "f64_plain" on a
    shape that would carry integer copies)."""
    rs = np.random.RandomState(2000 + seed)
    N, S, K = c.N, c.S, c.n_c + c.n_u
    R = rs.uniform(size=(N, K))
    D = rs.poisson(50, size=(N, S)).astype(np.int64) + 1
    X = rs.binomial(D, rs.uniform(size=(N, S)))
    if c.form == "f64_plain" and S >= 2 and c.n_c <= 48:
        D[N // 2, S // 2], X[N // 2, S // 2] = 70000, 12345
    V = X / D
    Rt = np.ascontiguousarray(R[:, :c.n_c]) if c.n_c else None
    u = np.ascontiguousarray(R[:, c.n_c:]) if c.n_u else None
    return V, D, Rt, u


def full_R(Rt, u):
    return np.concatenate([a for a in (Rt, u) if a is not None], axis=1)


# ------------------------------------------------------------------------------------------------ the active-set loop
Events = namedtuple("Events", "status x entries rejections drops multi_drops second_trips emptied reentries dual_ties "
                              "iterations order")


def _factor(A, plist, tol_k):
    """wls_factor: left-looking Cholesky of A[plist][:, plist]; None where a pivot is not above tol_k A_jj."""
    n = len(plist)
    L = np.zeros((n, n))
    Ap = A[np.ix_(plist, plist)]
    for j in range(n):
        v = np.zeros(n)
        v[j:] = Ap[j:, j]
        for k in range(j):  # (in the kernel's order, every row at once)
            v[j:] -= L[j:, k] * L[j, k]
        if not (v[j] > tol_k * A[plist[j], plist[j]]):
            return None
        d = np.sqrt(v[j])
        L[j, j] = d
        L[j + 1:, j] = v[j + 1:] / d
    return L


def _solve(L, rhs):
    """wls_solve: L L^T s = rhs, column-oriented forward and backward substitution."""
    n = len(rhs)
    acc, z = np.zeros(n), np.zeros(n)
    for j in range(n):
        z[j] = (rhs[j] - acc[j]) / L[j, j]
        acc[j + 1:] += L[j + 1:, j] * z[j]
    acc, sol = np.zeros(n), np.zeros(n)
    for j in range(n - 1, -1, -1):
        sol[j] = (z[j] - acc[j]) / L[j, j]
        acc[:j] += L[j, :j] * sol[j]
    return sol


def active_set_events(A, b):
    """k_nnls_intercept's loop on the K x K system (A, b) with counters: entries, rejections (candidates whose own coefficient
    came out non-positive), drops (variables removed by a step back), multi_drops (step backs that removed more than one),
    second_trips (step backs that followed another within one outer iteration), emptied (step backs that left no passive
    variable), reentries (entries of a variable dropped before), dual_ties (entries chosen among exactly equal largest
    duals), iterations (factorisations charged against the cap), order (the variables in the order they entered); status as
    the kernel reports it (0 solved, 1 not solved here) and x, the unnormalised coefficients (status 0)."""
    A, b = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64)
    K = b.size
    assert A.shape == (K, K) and 1 <= K <= 64
    tol_k, cap = K * 2.0 ** -52, 3 * K
    cnt = dict(entries=0, rejections=0, drops=0, multi_drops=0, second_trips=0, emptied=0, reentries=0, dual_ties=0)
    order, dropped = [], set()
    xs = np.zeros(K)
    plist, it, code, optimal = [], 0, 0, False
    if _factor(A, list(range(K)), tol_k) is None:
        code = 1
    for _outer in range(cap + 1):
        if code:
            break
        free = [i for i in range(K) if i not in plist]
        w = {}
        for i in free:
            acc = b[i]
            for j in plist:
                acc -= A[i, j] * xs[j]
            w[i] = acc
        rejected, entered, sol = set(), False, None
        for _c in range(K):
            cand = [i for i in free if i not in rejected]
            wm, im = -1.0, -1
            for i in cand:  # (rising index: the lowest index wins a tie)
                if w[i] > wm:
                    wm, im = w[i], i
            if not (wm > 0.0):
                break
            ties = sum(1 for i in cand if w[i] == wm)
            trial = plist + [im]
            it += 1
            L = _factor(A, trial, tol_k) if it <= cap else None
            if L is None:
                code = 1
                break
            sol = _solve(L, b[trial])
            if sol[-1] > 0.0:
                plist = trial
                entered = True
                cnt["entries"] += 1
                cnt["dual_ties"] += ties > 1
                cnt["reentries"] += im in dropped
                order.append(im)
                break
            rejected.add(im)
            cnt["rejections"] += 1
        if code:
            break
        if not entered:
            optimal = True
            break
        settled = False
        for inner in range(K + 1):
            n = len(plist)
            xq = xs[plist]
            bad = ~(sol > 0.0)
            if not bad.any():
                xs[plist] = sol
                settled = True
                break
            cnt["second_trips"] += inner >= 1
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(bad, np.where(xq > 0.0, xq / (xq - sol), 0.0), 2.0)
            qa = int(np.argmin(ratio))  # (the first of equals: the lowest passive ordinal)
            rm = ratio[qa]
            xn = xq + rm * (sol - xq)
            xn[qa] = 0.0
            keep = xn > 0.0
            gone = [plist[q] for q in range(n) if not keep[q]]
            cnt["drops"] += len(gone)
            cnt["multi_drops"] += len(gone) > 1
            dropped.update(gone)
            xs[plist] = np.where(keep, xn, 0.0)
            plist = [plist[q] for q in range(n) if keep[q]]
            if not plist:
                cnt["emptied"] += 1
                settled = True
                break
            it += 1
            L = _factor(A, plist, tol_k) if it <= cap else None
            if L is None:
                code = 1
                break
            sol = _solve(L, b[plist])
        if code == 0 and not settled:
            code = 1
    if code == 0 and not optimal:
        code = 1
    return Events(status=code, x=xs if code == 0 else None, iterations=it, order=tuple(order), **cnt)


def centred_system(G, mom_col):
    """(A, b) as the kernel forms them from a dense Gram G (K x K) and one column of a moments table."""
    K = G.shape[0]
    m, r, sw, st = mom_col[:K], mom_col[K:2 * K], mom_col[2 * K], mom_col[2 * K + 1]
    return G - np.outer(m, m) / sw, r - m * st / sw


def proportions(x):
    """The kernel's normalisation of a coefficient vector."""
    x = np.asarray(x, dtype=np.float64)
    return x / max(x.sum(), 1e-10)


def scipy_proportions(M, y):
    from scipy.optimize import nnls

    return proportions(nnls(M, y)[0])


def plain_moments(B):
    """The moments table that leaves the systems as they are: m = 0, sw = 1, st = 0 and r = B (K x S)."""
    K, S = B.shape
    mom = np.zeros((2 * K + 2, S))
    mom[K:2 * K] = B
    mom[2 * K] = 1.0
    return mom


# ------------------------------------------------------------------------------------------------ the solver's cases
System = namedtuple("System", "A b M y")  # A = M^T M and b = M^T y as the kernel is given them; (M, y) for scipy


def system_from_factors(M, y):
    return System(M.T @ M, M.T @ y, M, y)


def system_from_normal(A, b):
    """(M, y) with M^T M = A and M^T y = b to rounding (A positive definite): what scipy is given for a system that was
    written down as normal equations."""
    A, b = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64)
    M = np.linalg.cholesky(A).T
    return System(A, b, M, np.linalg.solve(M.T, b))


SYSTEMS_PER_K = 32


def correlated_system(rs, K):
    """Strongly correlated positive columns, a target with 30 % zeros: K + 2 .. K + 6 rows."""
    rows = K + rs.randint(2, 7)
    M = 0.7 * rs.uniform(size=(rows, 1)) + 0.3 * rs.uniform(size=(rows, K))
    y = rs.uniform(size=rows)
    y[rs.uniform(size=rows) < 0.3] = 0.0
    return system_from_factors(M, y)


def collinear_system(rs, K):
    """Columns that differ from one common column by a relative 1e-2 .. 1e-7 only: where rounding decides."""
    rows = K + rs.randint(2, 7)
    eps = 10.0 ** -rs.uniform(2.0, 7.0)
    M = (0.2 + rs.uniform(size=(rows, 1))) * (1.0 + eps * rs.uniform(-1.0, 1.0, size=(rows, K)))
    y = rs.uniform(size=rows)
    y[rs.uniform(size=rows) < 0.3] = 0.0
    return system_from_factors(M, y)


RECIPES = {"correlated": correlated_system, "collinear": collinear_system}


def search_events(seeds, recipe="correlated", ks=range(2, 13)):
    """The model's counters over one system per (seed, K) -> {counter: [(K, seed), ...]} of the systems with status 0 that
    count a rejection, an emptied passive set, a re-entry or a second trip (the first few of each), and the number tried."""
    hits = {"rejections": [], "emptied": [], "reentries": [], "second_trips": []}
    tried = 0
    for seed in seeds:
        for K in ks:
            s = RECIPES[recipe](np.random.RandomState(seed), K)
            e = active_set_events(s.A, s.b)
            tried += 1
            for name, where in hits.items():
                if getattr(e, name) and len(where) < 8 and (e.status == 0 or name in ("rejections", "emptied")):
                    where.append((K, seed, e.status))
    return hits, tried


def correlated_batch(K):
    rs = np.random.RandomState(7000 + K)
    return [correlated_system(rs, K) for _ in range(SYSTEMS_PER_K)]


def two_drop_system():
    """A step back that removes two variables at once, exactly.  A = [[1, 0, 1/4], [0, 1, 1/4], [1/4, 1/4, 9/64]], b = (4, 4,
    5/2): 0 enters (the tie of b_0 = b_1 goes to the lower index) with x_0 = 4, then 1 with x_1 = 4, then 2 (dual 5/2 - 2 = 1/2);
    the passive solve is (-4, -4, 32) -- every pivot (1, 1, 1/64) a dyadic square, every operation exact -- both ratios are
    4 / 8 = 1/2, ordinal 0 is taken and ordinal 1 comes out at 4 + (-8) / 2 = 0 exactly, so both leave; x = (0, 0, 160 / 9).
    A fourth variable, decoupled (A_33 = 1, b_3 = 1/2: it ties with variable 2's dual and enters behind it), keeps the
    proportions from being the trivial (0, 0, 1)."""
    A = np.array([[1.0, 0.0, 0.25, 0.0], [0.0, 1.0, 0.25, 0.0], [0.25, 0.25, 9.0 / 64.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    return system_from_normal(A, np.array([4.0, 4.0, 2.5, 0.5]))


def dual_tie_system():
    """The two largest duals of the first round are equal (b_1 = b_2 exactly): variable 1 enters first, as scipy's argmax
    chooses."""
    rs = np.random.RandomState(11)
    M = 0.5 * rs.uniform(size=(9, 1)) + 0.5 * rs.uniform(size=(9, 5))
    A = np.rint(M.T @ M * 1024.0) / 1024.0 + np.eye(5) / 8.0
    b = np.array([1.0, 3.5, 3.5, 2.0, 0.25])
    return system_from_normal(A, b)


# (name, K, seed) of systems drawn by `searched_system`: found by the search of tests/test_wls_model_host.py's docstring,
# certified there by the model's counters
SEARCHED = {"two_inner_trips": (9, 100673), "drop_then_reentry": (8, 102784)}


def searched_system(name):
    K, seed = SEARCHED[name]
    return correlated_system(np.random.RandomState(seed), K)


def named_systems():
    out = {"two_drops_at_once": two_drop_system(), "dual_tie": dual_tie_system()}
    out.update({name: searched_system(name) for name in SEARCHED})
    return out


# what the model must count on each named system (test_wls_model_host.py asserts it, test_gpu_wls_exact.py runs them)
NAMED_EVIDENCE = {
    "two_drops_at_once": lambda e: e.multi_drops >= 1 and e.drops >= 2,
    "dual_tie": lambda e: e.dual_ties >= 1 and e.order[0] == 1,
    "two_inner_trips": lambda e: e.second_trips >= 1,
    "drop_then_reentry": lambda e: e.reentries >= 1,
}


# ---- statuses
def status_batch(S):
    """S systems with the statuses 0, 1 and 2 interleaved -> (G (S, K, K), mom, expected status, systems or None): sample s
    takes kind s % 6 of: solvable; an exactly duplicated column; a duplicate perturbed by a relative 1e-10; sw = 0; sw < 0;
    sw = NaN.  K = 32.  Column 1 duplicates column 0 IN THE NORMAL EQUATIONS (row and column 1 of G are copies of row and column
    0, times 1 + 1e-10 for the perturbed kind, and b alike), so the first pivot behind it, A_11 - L_10^2, is rounding noise
    alone: L_10 = A_01 / sqrt(A_00) carries two roundings, its square five units of 2^-53, the scaling by 1 + 1e-10 three more --
    at most 8 x 2^-53 = 4 x 2^-52 of A_11 against the threshold 32 x 2^-52 A_11, whether or not the products are fused.  (In
    exact arithmetic the pivot is 0, and about 1e-20 A_11.)"""
    K = 32
    rs = np.random.RandomState(300 + S)
    G = np.empty((S, K, K))
    B = np.empty((K, S))
    systems, want = [], np.empty(S, dtype=np.intc)
    for s in range(S):
        kind = s % 6
        sysm = correlated_system(rs, K)
        G[s], B[:, s] = sysm.A, sysm.b
        if kind in (1, 2):
            f = 1.0 if kind == 1 else 1.0 + 1e-10
            G[s][1, :] = G[s][0, :]
            G[s][:, 1] = G[s][:, 0]
            G[s][1, :] *= f
            G[s][:, 1] *= f
            B[1, s] = B[0, s] * f
        want[s] = 0 if kind == 0 else 1 if kind in (1, 2) else 2
        systems.append(sysm if kind == 0 else None)
    mom = plain_moments(B)
    for s in range(S):
        if s % 6 >= 3:
            mom[2 * K, s] = (0.0, -1.0, np.nan)[s % 6 - 3]
    return G, mom, want, systems


# ------------------------------------------------------------------------------------------------ the public route
ROUTE_K = (3, 8, 17, 33, 64)
ROUTE_S = 64


def route_problem(K):
    """(V, D, R) of N = K + 6 rows and 64 samples whose regressions drop variables: R = round(256 (0.7 common + 0.3 noise)) /
    256, counts 1 .. 8, x binomial with 30 % of the elements at zero."""
    rs = np.random.RandomState(501 + K)
    N = K + 6
    R = np.rint(256.0 * (0.7 * rs.uniform(size=(N, 1)) + 0.3 * rs.uniform(size=(N, K)))) / 256.0
    D = rs.randint(1, 9, size=(N, ROUTE_S)).astype(np.int64)
    X = rs.binomial(D, rs.uniform(size=(N, ROUTE_S)))
    X[rs.uniform(size=X.shape) < 0.3] = 0
    return X / D, D, R


def route_systems(V, D, R, target):
    """The centred normal equations of every sample, in float64, as the device forms them (for the model's counters)."""
    out = []
    for s in range(V.shape[1]):
        d = D[:, s].astype(np.float64)
        t = d * V[:, s] if target == "dv" else V[:, s]
        sw, st = d.sum(), (d * t).sum()
        m, r = R.T @ d, R.T @ (d * t)
        G = (R * d[:, None]).T @ R
        out.append((G - np.outer(m, m) / sw, r - m * st / sw))
    return out
