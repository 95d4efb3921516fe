"""The purity-constrained solver (dmf_solver_set_purity, deconvolution.py:228-337): both Frank-Wolfe alpha kernels,
k_alpha_frank_wolfe_row16 (K = n_c + n_u <= 16, one sample per 16-lane row) and k_alpha_frank_wolfe (K = 17..64, one
thread per sample), behind every row pass and Gram kernel the selection table can put in front of them.

Leg 1 takes the alpha kernel alone: after every outer iteration the GPU's own u and the alpha from before the step go
through the reference Frank-Wolfe loop (:280-302) in np.longdouble, gradients as -W^T (D * (V - W a)).  Given the same
vertex choices alpha is a fixed chain of convex updates a = (1 - g) a + g v with entries in [0, 1], two roundings each:
|alpha_gpu - alpha_ref| <= 4 n_iter2 2^-53, where ONE wrong vertex costs at least 2 / (n_iter2 + 1) of a block's mass.
With one Frank-Wolfe iteration (g = 1) alpha is the vertex itself, bit for bit.

Near ties.  The kernels form the gradient as G a - b: first-order error about 3 (K + 2) 2^-53 scale (2e-14 scale at
K = 64), plus that of the Gram entries (worst u deviation on record: 1.8e-12).  A decision whose two best gradient
entries lie closer than GAP = 1e-9 scale_s (scale_s = max_k (R^T (D * V))_ks) cannot be called either way; 1e-9 leaves
100x over both errors.  No case is excused on that account: every case asserts that its smallest gap is at least GAP,
on the reference of leg 1 and -- without a GPU, test_no_case_has_a_near_tie -- on the f64 oracle trajectory, and the
seeds were chosen so that it is.

Leg 2 is the whole solve against the oracle at the bars of tests/test_gpu_solver.py.  test_matrix_covers_the_selection_table
(no GPU) holds the matrix to every (alpha kernel, row pass, Gram kernel) triple the selection table can produce under
purity for integer counts."""
import ctypes as C
import functools
import itertools
import re
from collections import namedtuple

import numpy as np
import pytest

from oracle import solver as osol

from conftest import rel_err

TIGHT = 1e-8  # oracle parity, as in tests/test_gpu_solver.py
GAP = 1e-9    # smallest relative gap between the two best gradient entries of a block that is a decision (see above)
UNIT = 2.0 ** -53

ROW16, GENERAL = "k_alpha_frank_wolfe_row16", "k_alpha_frank_wolfe"

# level: dmf_context_set_generic; x16: the context's X16 switch (matters at level 0); zero: zero-coverage stripes;
# row / gram: what Solver.describe must name (template arguments and the /w8 suffix left out, " x16" kept)
Case = namedtuple("Case", "N S n_c n_u n_iter2 level x16 depth zero seed T1 row gram")

V2, V2X = "k_rowpass_v2", "k_rowpass_v2 x16"
CM_BU, CM_ROWS = "k_cm_i8+k_inner_bu", "k_cm_i8+k_u_inner_rows"
SPLIT, MFMA, BIG, UGRAM, DIRECT, FUSED = ("k_u_phase_mfma(split)+k_u_inner_rows", "k_u_phase_mfma", "k_u_phase_big",
                                          "k_u_phase_gram", "k_u_step_direct", "k_rowpass_fused")
I8, BU_I8, GU, GMFMA, GRAM, INROW = "k_gram_i8", "k_bu_cols+k_gram_i8", "k_gram_u", "k_gram_mfma", "k_gram", "fused"

# The axes (each value somewhere, cycled against the others):
#   row16   (n_c, n_u): (1,1) (1,2) (2,1) (3,1) (4,2) (2,3) (7,5) (12,4) (8,8) (1,15) (15,1)   S: 1 2 3 5 7 63 64 65 130 257
#   general (n_c, n_u): (16,1) (12,5) (1,16) (20,12) (9,26) (40,24) (32,32) (48,16)            S: 1 3 63 64 65 130 257
#   n_iter2 1 2 7 20 50 51 70 500 (50 | 51: kSplitInnerSteps), levels 0..4, X16 on and off at level 0, one and two count
#   digits (depth 40 / 400), zero-coverage stripes.  The 500-step cases are small: the longdouble reference has no BLAS.
MATRIX = [
    # ---- k_alpha_frank_wolfe_row16
    Case(403, 2, 1, 1, 1, 0, True, 40, 0, 101, 3, V2X, I8),       # K = 2: lanes 0 and n_c against 14 lanes of +inf
    Case(400, 1, 1, 1, 20, 0, True, 40, 0, 102, 3, MFMA, GU),     # one sample: three of the block's four rows clamped
    Case(517, 3, 1, 2, 2, 0, False, 40, 0, 103, 3, V2, I8),
    Case(450, 5, 2, 1, 7, 0, True, 400, 0, 104, 3, V2X, I8),
    Case(409, 7, 3, 1, 50, 0, False, 40, 0, 105, 3, V2, I8),
    Case(431, 63, 3, 1, 51, 0, True, 40, 0, 106, 2, SPLIT, GU),
    Case(4100, 130, 4, 2, 20, 0, True, 40, 1, 107, 3, V2X, I8),   # 65..256 samples on X16: the pair schedule
    Case(400, 64, 4, 2, 7, 4, True, 40, 0, 108, 3, FUSED, INROW),
    Case(405, 65, 2, 3, 500, 0, True, 40, 0, 109, 2, SPLIT, GU),
    Case(420, 257, 2, 3, 20, 0, False, 400, 0, 110, 2, V2, I8),
    Case(411, 63, 7, 5, 70, 0, True, 40, 0, 111, 2, CM_BU, I8),
    Case(402, 257, 7, 5, 2, 0, True, 40, 1, 112, 3, CM_ROWS, BU_I8),
    Case(440, 1, 7, 5, 7, 0, True, 40, 0, 113, 3, SPLIT, GU),
    Case(770, 64, 12, 4, 50, 0, True, 400, 0, 114, 2, V2X, I8),   # K = 16: no lane is padding
    Case(416, 1, 12, 4, 2, 0, True, 40, 0, 115, 3, MFMA, GU),
    Case(433, 65, 12, 4, 51, 0, False, 40, 0, 116, 2, SPLIT, BU_I8),
    Case(400, 5, 8, 8, 500, 0, True, 40, 0, 117, 2, CM_BU, I8),
    Case(407, 130, 8, 8, 1, 0, True, 40, 0, 118, 3, CM_BU, I8),
    Case(412, 3, 1, 15, 20, 0, True, 400, 0, 119, 3, CM_BU, I8),  # the unknown block's argmin over lanes 1..15
    Case(400, 1, 1, 15, 50, 0, True, 40, 0, 120, 2, BIG, GMFMA),
    Case(423, 7, 1, 15, 7, 3, True, 40, 0, 121, 3, BIG, GMFMA),
    Case(401, 2, 15, 1, 70, 0, True, 40, 0, 122, 2, SPLIT, GU),   # the known block's argmin over lanes 0..14
    Case(400, 257, 15, 1, 7, 0, True, 40, 0, 123, 3, V2X, I8),
    Case(419, 63, 2, 1, 20, 1, True, 40, 0, 124, 3, UGRAM, GRAM),
    Case(400, 65, 3, 1, 2, 2, True, 400, 0, 125, 3, DIRECT, GRAM),
    Case(406, 64, 1, 2, 50, 3, True, 40, 1, 126, 2, MFMA, GU),
    Case(400, 64, 15, 1, 1, 4, True, 40, 0, 127, 3, FUSED, INROW),
    # ---- k_alpha_frank_wolfe
    Case(404, 3, 16, 1, 20, 0, True, 40, 0, 201, 3, V2X, I8),
    Case(430, 130, 16, 1, 7, 0, False, 40, 0, 202, 3, V2, I8),    # last block of 64 threads: 2 live
    Case(400, 64, 16, 1, 2, 4, True, 40, 0, 203, 3, FUSED, INROW),
    Case(413, 1, 16, 1, 50, 0, True, 40, 0, 204, 2, MFMA, GU),    # 1 live thread
    Case(400, 65, 16, 1, 51, 0, True, 400, 0, 205, 2, SPLIT, GU),
    Case(408, 63, 12, 5, 70, 0, True, 40, 0, 206, 2, CM_BU, I8),  # 63 live threads
    Case(400, 257, 12, 5, 1, 0, True, 40, 1, 207, 3, CM_ROWS, BU_I8),
    Case(400, 1, 12, 5, 500, 0, True, 40, 0, 208, 2, SPLIT, GU),
    Case(421, 1, 1, 16, 7, 0, True, 40, 0, 209, 3, BIG, GMFMA),
    Case(400, 64, 1, 16, 20, 3, True, 40, 0, 210, 2, BIG, GMFMA),  # 64 live threads
    Case(410, 3, 1, 16, 2, 0, True, 400, 0, 211, 3, CM_BU, I8),
    Case(400, 1, 20, 12, 20, 0, True, 40, 0, 212, 2, UGRAM, GMFMA),
    Case(415, 65, 20, 12, 7, 1, True, 40, 0, 213, 3, UGRAM, GRAM),
    Case(400, 63, 20, 12, 50, 3, True, 40, 0, 214, 2, UGRAM, GMFMA),
    Case(402, 130, 20, 12, 2, 0, True, 40, 1, 215, 3, CM_BU, I8),
    Case(400, 64, 9, 26, 20, 0, True, 40, 0, 216, 2, CM_ROWS, GMFMA),
    Case(427, 3, 9, 26, 1, 2, True, 40, 0, 217, 3, DIRECT, GRAM),
    Case(400, 1, 40, 24, 2, 0, True, 40, 0, 218, 3, DIRECT, GMFMA),  # K = 64: a[] and grad[] full
    Case(400, 130, 40, 24, 7, 0, True, 40, 0, 219, 2, CM_ROWS, GMFMA),
    Case(400, 3, 40, 24, 500, 0, True, 40, 0, 220, 2, CM_ROWS, GMFMA),
    Case(405, 65, 32, 32, 20, 0, True, 40, 0, 221, 2, CM_ROWS, GMFMA),
    Case(400, 257, 32, 32, 2, 3, True, 400, 0, 222, 2, DIRECT, GMFMA),
    Case(414, 63, 48, 16, 7, 0, True, 400, 0, 223, 3, CM_ROWS, GMFMA),
    Case(400, 64, 48, 16, 50, 1, True, 40, 0, 224, 2, UGRAM, GRAM),
]


def _cid(c):
    x = "" if c.level else ("x" if c.x16 else "v")
    return f"{c.n_c}+{c.n_u}-S{c.S}-i{c.n_iter2}-L{c.level}{x}"


IDS = [_cid(c) for c in MATRIX]
assert len(set(IDS)) == len(IDS)


def _alpha_kernel(n_c, n_u):
    return ROW16 if n_c + n_u <= 16 and n_c >= 1 else GENERAL


def _kinds(desc):
    """(alpha kernel, row pass, Gram kernel) of a describe string, without template arguments; the row pass's X16 form
    keeps its " x16"."""
    row, gram, alpha = re.fullmatch(r"rowpass=(.*) gram=(\S+) alpha=(\S+)", desc).groups()
    kind = re.sub(r"<[^>]*>", "", row).split(" ")[0]
    if kind == V2 and row.endswith(" x16"):
        kind = V2X
    return alpha, kind, re.sub(r"<[^>]*>", "", gram).replace("/w8", "")


def _purity(S, seed):
    """Uniform in (0.05, 0.95) with an exact 1.0 and an exact 0.0 planted, one of them in the last sample (the clamped
    last block of either kernel); one sample: 0.0 (with 1.0 the unknown block of the whole problem is empty: l_w = 0)."""
    rs = np.random.RandomState(seed)
    p = rs.uniform(0.05, 0.95, S)
    if S == 1:
        p[0] = 0.0
    else:
        first, last = (0.0, 1.0) if seed % 2 else (1.0, 0.0)
        p[S - 1] = last
        p[(S // 2) if S > 2 else 0] = first
    return p


def _problem(N, S, n_c, n_u, depth, zero, seed):
    """(V, D, Rt, purity, u0, alpha0)"""
    V, D, Rt = osol.synthetic_problem(N, S, n_c, n_u, seed=seed, depth=depth)
    if zero:
        rs = np.random.RandomState(seed + 7)
        D[rs.randint(0, 5)::rs.randint(3, 9), rs.randint(0, 2)::rs.randint(2, 5)] = 0
        V = np.where(D == 0, 0.0, V)
    purity = _purity(S, seed + 11)
    u0, _, a0 = osol.init_partial_purity("uniform_", V, D, Rt, n_u, purity, seed=seed + 1)
    return V, D, Rt, purity, u0, a0


def _data(c):
    return _problem(c.N, c.S, c.n_c, c.n_u, c.depth, c.zero, c.seed)


def _oracle(data, T1, n_iter2, tol=0.0):
    """(u, alpha, cost trace, smallest gap) of the f64 oracle trajectory."""
    V, D, Rt, purity, u0, a0 = data
    trace, gaps = [], []
    wu, wa = osol.solve_partial_purity(u0.copy(), np.c_[Rt, u0], a0.copy(), V, D, Rt, u0.shape[1], purity, T1, n_iter2, tol,
                                       trace=trace, gaps=gaps)
    return wu, wa, trace, min(gaps)


@functools.lru_cache(maxsize=None)
def _case_oracle(i):
    c = MATRIX[i]
    return _oracle(_data(c), c.T1, c.n_iter2)


# ----------------------------------------------------------------------------------------- no GPU
def test_gap_bookkeeping_leaves_the_oracle_alone():
    """frank_wolfe_alpha_gaps in f64 is frank_wolfe_alpha bit for bit, and its gap is the distance between the two
    smallest gradient entries of the closest decision."""
    V, D, Rt, purity, u0, a0 = _problem(300, 9, 3, 4, 25, 0, 5)
    a1, a2 = osol.frank_wolfe_alpha(Rt, u0, V, a0[:3], a0[3:], purity, 30, D)
    b1, b2, gap = osol.frank_wolfe_alpha_gaps(Rt, u0, V, a0[:3], a0[3:], purity, 30, D)
    assert np.array_equal(a1, b1) and np.array_equal(a2, b2) and 0 < gap < 1
    c1, c2, gap_ld = osol.frank_wolfe_alpha_gaps(Rt, u0, V, a0[:3], a0[3:], purity, 30, D, dtype=np.longdouble)
    assert c1.dtype == np.longdouble and np.abs(c1 - a1).max() <= 4 * 30 * UNIT and np.abs(c2 - a2).max() <= 4 * 30 * UNIT
    assert gap_ld == pytest.approx(gap, rel=1e-6)
    # one iteration by hand
    W = np.c_[Rt, u0]
    g = -W.T @ (D * (V - W @ a0))
    scale = (W.T @ (D * V)).max(axis=0)
    want = min(np.diff(np.sort(g[:3], axis=0)[:2], axis=0).ravel() / scale).item(), \
        min(np.diff(np.sort(g[3:], axis=0)[:2], axis=0).ravel() / scale).item()
    assert osol.frank_wolfe_alpha_gaps(Rt, u0, V, a0[:3], a0[3:], purity, 1, D)[2] == pytest.approx(min(want), rel=1e-12)
    # a block of one row has no decision to take
    assert osol.frank_wolfe_alpha_gaps(Rt[:, :1], u0[:, :1], V, a0[:1], a0[3:4], purity, 3, D)[2] == np.inf


@pytest.mark.parametrize("i", range(len(MATRIX)), ids=IDS)
def test_no_case_has_a_near_tie(i, record_property):
    """The precondition of every assertion on alpha below, on the f64 oracle trajectory: a seed that puts a decision
    inside GAP shows up here, before anything reaches a GPU.  (A new seed is the remedy, never a skip.)"""
    c = MATRIX[i]
    gap = _case_oracle(i)[3]
    record_property("smallest_gap", gap)
    assert gap >= GAP, (IDS[i], gap)  # (inf where neither block has a decision to take)
    purity = _purity(c.S, c.seed + 11)
    assert 0.0 in purity and (c.S == 1 or 1.0 in purity) and purity[-1] in (0.0, 1.0)


def _select_describe(lib, N, S, n_c, n_u, nd, level, n_iter2, x16):
    from demethify_amd import _lib as L

    flags = L.DMF_SELECT_COUNTS_F32_EXACT | L.DMF_SELECT_PURITY | (L.DMF_SELECT_X16 if x16 else 0)
    buf = C.create_string_buffer(512)
    st = lib.dmf_select_describe(N, S, n_c, n_u, nd, level, n_iter2, flags, buf, len(buf))
    return buf.value.decode() if st == L.DMF_OK else None


def test_matrix_covers_the_selection_table():
    """Every case describes (dmf_select_describe with DMF_SELECT_PURITY) as the kernels it names, and the matrix holds
    every (alpha kernel, row pass, Gram kernel) triple -- hence every pair of alpha kernel x row pass and every Gram kernel
    behind either alpha kernel -- that the table gives anywhere on a grid of shapes, levels, count digits, X16 flags and
    inner-step counts, enumerated here as tests/golden/make_kernel_selection.py enumerates its own.  The grid has one
    and two count digit planes (nd = 1, 2: integer counts up to 32639, what the cases are made of); without integer
    copies (nd = 0) the table only loses the integer routes and reaches a subset of the same triples, asserted below.
    The pair schedule of k_rowpass_v2 is no row kind of the table: the 130-sample X16 case counts its pair launches."""
    from demethify_amd import _lib as L

    lib = L.load()
    seen = set()
    for cid, c in zip(IDS, MATRIX):
        nd = 2 if c.depth > 127 else 1
        got = _select_describe(lib, c.N, c.S, c.n_c, c.n_u, nd, c.level, c.n_iter2, c.x16 and c.level == 0)
        assert got is not None and _kinds(got) == (_alpha_kernel(c.n_c, c.n_u), c.row, c.gram), (cid, got)
        assert (_alpha_kernel(c.n_c, c.n_u) == GENERAL) == (c.n_c + c.n_u > 16), cid
        # (a one-sample problem carries no integer copies of its counts: the table must not name an integer kernel)
        assert c.S > 1 or "i8" not in got, (cid, got)
        seen.add(_kinds(got))
    types = sorted({(c.n_c, c.n_u) for c in MATRIX})
    samples = sorted({c.S for c in MATRIX})
    steps = sorted({c.n_iter2 for c in MATRIX})
    assert steps == [1, 2, 7, 20, 50, 51, 70, 500] and samples == [1, 2, 3, 5, 7, 63, 64, 65, 130, 257] and len(types) == 19
    assert {c.level for c in MATRIX} == set(range(5)) and {c.x16 for c in MATRIX if c.level == 0} == {True, False}
    assert {c.depth for c in MATRIX} == {40, 400} and any(c.zero for c in MATRIX)
    reachable, without_ints = set(), set()
    for (n_c, n_u), S, level, nd, x16, n_iter2, N in itertools.product(types, samples, range(5), (0, 1, 2), (False, True), steps,
                                                                     (10, 400, 4100)):
        got = _select_describe(lib, N, S, n_c, n_u, nd, level, n_iter2, x16)
        if got is not None:
            (reachable if nd else without_ints).add(_kinds(got))
    assert without_ints <= reachable, sorted(without_ints - reachable)
    assert {k[0] for k in reachable} == {ROW16, GENERAL}
    assert seen == reachable, (sorted(reachable - seen), sorted(seen - reachable))


# ----------------------------------------------------------------------------------------- the matrix on the GPU
def _reference_step(V, D, Rt, u, a_prev, purity, n_iter2):
    """One alpha phase by the reference's formulas in longdouble from the GPU's own u: (alpha, smallest gap)."""
    n_c = Rt.shape[1]
    a1, a2, gap = osol.frank_wolfe_alpha_gaps(Rt, u, V, a_prev[:n_c], a_prev[n_c:], purity, n_iter2, D, dtype=np.longdouble)
    return np.vstack((a1, a2)), gap


def _check_alpha_step(name, V, D, Rt, purity, u, a_prev, alpha, cost, n_iter2):
    """The assertions of leg 1 on one outer iteration; returns (deviation / bound, gap)."""
    n_c, K = Rt.shape[1], alpha.shape[0]
    ref, gap = _reference_step(V, D, Rt, u, a_prev, purity, n_iter2)
    bound = 4 * n_iter2 * UNIT
    dev = float(np.abs(alpha.astype(np.longdouble) - ref).max())
    s1 = float(np.abs(alpha[:n_c].sum(axis=0) - purity).max())
    s2 = float(np.abs(alpha[n_c:].sum(axis=0) - (1 - purity)).max())
    want = osol.weighted_cost(V, np.c_[Rt, u], alpha, D)
    print(f"purity {name}: alpha dev {dev:.3e} = {dev / bound:.3f} bound, gap {gap:.3e}, sums {s1:.2e} {s2:.2e}, "
          f"cost rel {abs(cost - want) / want:.2e}")
    assert gap >= GAP, (name, gap)  # the precondition (module docstring)
    assert dev <= bound, (name, dev, bound)
    if n_iter2 == 1:
        assert np.array_equal(alpha, ref.astype(np.float64)), name
    assert s1 <= K * bound and s2 <= K * bound, (name, s1, s2)
    assert cost == pytest.approx(want, rel=1e-9), (name, cost, want)
    return dev / bound, gap


def _check_against_oracle(name, Rt, purity, u, alpha, wu, wa):
    """The bars of leg 2; returns the three TIGHT quantities."""
    n_c = Rt.shape[1]
    ea, da, du = rel_err(alpha, wa), float(np.abs(alpha - wa).max()), float(np.abs(u - wu).max())
    print(f"purity {name}: oracle rel_err(alpha) {ea:.2e} max|dalpha| {da:.2e} max|du| {du:.2e}")
    assert ea < TIGHT and da < TIGHT and du < TIGHT, (name, ea, da, du)
    assert np.allclose(alpha[:n_c].sum(axis=0), purity, atol=1e-12), name
    assert np.allclose(alpha[n_c:].sum(axis=0), 1 - purity, atol=1e-12), name
    return ea, da, du


def _stepwise(ctx, data, level, x16, n_iter2, T1, expect, name):
    """Problem + Solver under (level, x16) with the purity set: describe must name `expect`; T1 single steps, leg 1 after
    each; then the whole solve through solve_problem.  Returns (trail of (u, alpha, cost), solve_problem's result,
    row-pass launches, worst deviation / bound, smallest gap)."""
    from demethify_amd import _lib as L
    from demethify_amd.deconvolution import solve_problem
    from demethify_amd.device import Problem, Solver

    V, D, Rt, purity, u0, a0 = data
    trail, worst, gap = [], 0.0, np.inf
    ctx.set_generic(level)
    ctx.set_x16(x16)
    try:
        with Problem(ctx, V, D, Rt) as p:
            with Solver(p, u0, a0) as s:
                s.set_purity(purity)
                desc = s.describe(n_iter2)
                assert _kinds(desc) == expect, (name, desc)
                prev = a0
                for t in range(T1):
                    it, _ = s.step(1, n_iter2, 0.0)
                    u, alpha, cost, it2 = s.get()
                    assert it == it2 == t + 1, (name, it, it2)
                    w, g = _check_alpha_step(f"{name} step {t}", V, D, Rt, purity, u, prev, alpha, cost, n_iter2)
                    worst, gap = max(worst, w), min(gap, g)
                    trail.append((u, alpha, cost))
                    prev = alpha
                launches = s.rowpass_launches()
            whole = solve_problem(p, u0, a0, L.DMF_MODE_PARTIAL, T1, n_iter2, 0.0, return_info=True, purity=purity)
    finally:
        ctx.set_generic(0)
        ctx.set_x16(True)
    return trail, whole, launches, worst, gap


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(MATRIX)), ids=IDS)
def test_matrix_against_reference_and_oracle(ctx, record_property, i):
    """Legs 1 and 2 of one case.  Measured on an MI355X over the 51 cases: worst alpha deviation of leg 1 0.083 of its
    bound (7+5-S257-i2), bit-equal at one Frank-Wolfe iteration; smallest gap 3.2e-8 (2+3-S65-i500); leg 2 rel_err(alpha)
    6.2e-16, max|dalpha| 1.1e-15, max|du| 5.9e-11.

    40+24-S3-i500-L0x (24 unknown profiles from 3 samples, 2 x 500 inner steps, k_cm_i8 + k_u_inner_rows) is the case that
    found the scale of k_cm_i8's P digits: alpha_j alpha_l went into M_i as rint(P 2^52), an ABSOLUTE 2^-53, which at
    K = 64 is 1e-13 .. 1e-12 of the product; with more unknowns than samples u is not identified, the momentum steps
    integrate that perturbation, and max|du| came to 4.99e-8 (alpha 1.4e-17; the schedule-faithful kernels 8.6e-11; a numpy
    Gram-form u phase with P rounded that way 4.99e-8 too).  The digits now carry every alpha row scaled by a power of
    two to [1/2, 1]: 5.9e-11 on the GPU (the same emulation gives 7.4e-11)."""
    c = MATRIX[i]
    data = _data(c)
    V, D, Rt, purity, u0, a0 = data
    assert (D.max() > 127) == (c.depth > 127)
    expect = (_alpha_kernel(c.n_c, c.n_u), c.row, c.gram)
    trail, whole, launches, worst, gap = _stepwise(ctx, data, c.level, c.x16, c.n_iter2, c.T1, expect, IDS[i])
    record_property("alpha_dev_over_bound", worst)
    record_property("smallest_gap", gap)
    if c.row in (V2, V2X):
        nw = (c.S + 63) // 64  # (the pair schedule: X16 at two to four waves, except two waves with four unknowns)
        pairs = c.row == V2X and 2 <= nw <= 4 and not (nw == 2 and c.n_u == 4)
        assert launches == (c.T1, c.T1 if pairs else 0), launches
    else:
        assert launches == (0, 0)
    # leg 2: the whole solve, in one call, against the oracle -- and against the single steps bit for bit
    gu, ga, gcost, iters = whole
    assert iters == c.T1
    assert np.array_equal(gu, trail[-1][0]) and np.array_equal(ga, trail[-1][1]) and gcost == trail[-1][2]
    wu, wa, trace, wgap = _case_oracle(i)
    assert wgap >= GAP
    ea, da, du = _check_against_oracle(IDS[i], Rt, purity, gu, ga, wu, wa)
    for k, v in (("oracle_rel_alpha", ea), ("oracle_da", da), ("oracle_du", du)):
        record_property(k, v)
    assert gcost == pytest.approx(trace[-1], rel=1e-9)


# ----------------------------------------------------------------------------------------- natural stop
# 20 Frank-Wolfe steps per outer iteration leave alpha far enough from its optimum that the cost differences of this
# shape hover between 1 and 300 for hundreds of iterations (at the CLI's 1e-2 the oracle is still running at 400).  The
# threshold sits where the trajectory crosses it with room on both sides: the differences before iteration 17 are all
# 68 or more, the one at 17 is 30.6 -- against 1e-4 of error in a Gram-form cost of 1.5e5.
NATURAL = dict(N=4096, S=100, n_c=6, n_u=2, depth=25, seed=301, n_iter2=20, tol=50.0, cap=400, stop=17)


@functools.lru_cache(maxsize=None)
def _natural_oracle():
    n = NATURAL
    data = _problem(n["N"], n["S"], n["n_c"], n["n_u"], n["depth"], 0, n["seed"])
    return data, _oracle(data, n["cap"], n["n_iter2"], n["tol"])


def test_natural_stop_case_has_no_near_tie():
    _, (_, _, trace, gap) = _natural_oracle()
    assert gap >= GAP and len(trace) == NATURAL["stop"] < NATURAL["cap"], (gap, len(trace))
    steps = np.abs(np.diff(trace))
    assert steps[:-1].min() > 1.3 * NATURAL["tol"] and steps[-1] < 0.7 * NATURAL["tol"], steps  # (a clear crossing)


@pytest.mark.gpu
def test_natural_stop_under_purity(ctx):
    """The stop test |cf - cf_0| < tol under purity at a fast-path shape: the same iteration as the oracle."""
    from demethify_amd import _lib as L
    from demethify_amd.deconvolution import solve_problem
    from demethify_amd.device import Problem, Solver

    n = NATURAL
    (V, D, Rt, purity, u0, a0), (wu, wa, trace, gap) = _natural_oracle()
    assert gap >= GAP
    with Problem(ctx, V, D, Rt) as p:
        with Solver(p, u0, a0) as s:
            s.set_purity(purity)
            assert _kinds(s.describe(n["n_iter2"])) == (ROW16, V2X, I8), s.describe(n["n_iter2"])
            it, converged = s.step(n["cap"], n["n_iter2"], n["tol"])
            u, alpha, cost, it2 = s.get()
        gu, ga, gcost, giters = solve_problem(p, u0, a0, L.DMF_MODE_PARTIAL, n["cap"], n["n_iter2"], n["tol"],
                                              return_info=True, purity=purity)
    print(f"purity natural stop: {it} iterations, oracle {len(trace)}, gap {gap:.3e}")
    assert converged and it == it2 == giters == len(trace) < n["cap"], (it, it2, giters, len(trace))
    assert cost == pytest.approx(trace[-1], rel=1e-9) and gcost == cost
    assert np.array_equal(ga, alpha) and np.array_equal(gu, u)
    _check_against_oracle("natural stop", Rt, purity, u, alpha, wu, wa)


# ----------------------------------------------------------------------------------------- exact ties
# two identical columns k1 < k2 of R_trunc: every decision of the known block between them is an exact tie
TIES = {ROW16: dict(N=500, S=7, n_c=4, n_u=2, k1=0, k2=2, n_iter2=20, seed=401, expect=(ROW16, V2X, I8)),
        GENERAL: dict(N=500, S=67, n_c=12, n_u=5, k1=3, k2=7, n_iter2=20, seed=402, expect=(GENERAL, CM_BU, I8))}
TIE_STEPS = 3


def _tie_problem(t):
    V, D, Rt, purity, u0, a0 = _problem(t["N"], t["S"], t["n_c"], t["n_u"], 40, 0, t["seed"])
    Rt = Rt.copy()
    Rt[:, t["k2"]] = Rt[:, t["k1"]]
    return V, D, Rt, purity, u0, a0


def _merged(alpha, k1, k2):
    """alpha with row k2 added to row k1 and taken out."""
    out = np.delete(alpha, k2, axis=0)
    out[k1] = alpha[k1] + alpha[k2]
    return out


@pytest.mark.parametrize("kernel", list(TIES))
def test_tie_cases_have_no_other_near_tie(kernel):
    """The same problem with the duplicate column taken out (its alpha row merged into the first) has the decisions of
    the tie problem except the tie itself: those must be clear of GAP."""
    t = TIES[kernel]
    V, D, Rt, purity, u0, a0 = _tie_problem(t)
    data = (V, D, np.delete(Rt, t["k2"], axis=1), purity, u0, _merged(a0, t["k1"], t["k2"]))
    assert _oracle(data, TIE_STEPS, t["n_iter2"])[3] >= GAP


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", list(TIES))
def test_exact_ties_go_to_the_first_index(ctx, kernel):
    """np.argmin takes the first of equal minima (deconvolution.py:292-293).  The packed Gram rows of two identical
    columns are bit-identical (the integer Gram's sums are exact) and both kernels add a row's products in column order,
    so the two gradient entries are equal bit for bit and row k2 must never be chosen: exactly 0 after every step.
    Against the oracle (whose BLAS need not keep the tie exact) the merged row and every other row hold TIGHT."""
    from demethify_amd.device import Problem, Solver

    t = TIES[kernel]
    k1, k2 = t["k1"], t["k2"]
    V, D, Rt, purity, u0, a0 = data = _tie_problem(t)
    wu, wa, _, _ = _oracle(data, TIE_STEPS, t["n_iter2"])
    with Problem(ctx, V, D, Rt) as p, Solver(p, u0, a0) as s:
        s.set_purity(purity)
        assert _kinds(s.describe(t["n_iter2"])) == t["expect"], s.describe(t["n_iter2"])
        for step in range(TIE_STEPS):
            s.step(1, t["n_iter2"], 0.0)
            u, alpha, _, _ = s.get()
            print(f"purity tie {kernel} step {step}: max alpha[k2] {alpha[k2].max():.3e}, max alpha[k1] {alpha[k1].max():.3e}")
            assert np.all(alpha[k2] == 0.0), (step, alpha[k2])
            assert alpha[k1].max() > 0.0  # (the pair is chosen at all: the tie is exercised)
    assert np.abs(_merged(alpha, k1, k2) - _merged(wa, k1, k2)).max() < TIGHT and np.abs(u - wu).max() < TIGHT
    assert rel_err(_merged(alpha, k1, k2), _merged(wa, k1, k2)) < TIGHT


# ----------------------------------------------------------------------------------------- what belongs with it
GATHERED = dict(N=1200, S=40, n_c=5, n_u=2, depth=40, seed=501, n_iter2=30, T1=3, resample=17)


def _gathered_problem():
    g = GATHERED
    V, D, Rt, purity, _, _ = _problem(g["N"], g["S"], g["n_c"], g["n_u"], g["depth"], 0, g["seed"])
    idx = osol.bootstrap_indices(g["resample"], g["N"])
    Vg, Dg, Rg = V[idx], D[idx], Rt[idx]
    u0, _, a0 = osol.init_partial_purity("uniform_", Vg, Dg, Rg, g["n_u"], purity, seed=g["seed"] + 1)
    return (V, D, Rt, idx), (Vg, Dg, Rg, purity, u0, a0)


def test_gathered_case_has_no_near_tie():
    assert _oracle(_gathered_problem()[1], GATHERED["T1"], GATHERED["n_iter2"])[3] >= GAP


@pytest.mark.gpu
def test_purity_on_a_gathered_problem(ctx):
    """bootstrap.py:28 under purity: Problem.gather keeps X16, and the solve matches the oracle on the fancy-indexed
    arrays."""
    from demethify_amd.device import Problem, Solver

    g = GATHERED
    (V, D, Rt, idx), data = _gathered_problem()
    Vg, Dg, Rg, purity, u0, a0 = data
    wu, wa, trace, gap = _oracle(data, g["T1"], g["n_iter2"])
    assert gap >= GAP
    with Problem(ctx, V, D, Rt) as p, p.gather(idx) as q, Solver(q, u0, a0) as s:
        s.set_purity(purity)
        assert _kinds(s.describe(g["n_iter2"])) == (ROW16, V2X, I8), s.describe(g["n_iter2"])
        it, _ = s.step(g["T1"], g["n_iter2"], 0.0)
        u, alpha, cost, _ = s.get()
    assert it == g["T1"]
    _check_against_oracle("gathered", Rg, purity, u, alpha, wu, wa)
    assert cost == pytest.approx(trace[-1], rel=1e-9)


@pytest.mark.gpu
def test_set_purity_refusals(ctx):
    """Partial-reference mode only (DMF_ERR_BAD_ARG otherwise); one value per sample."""
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    V, D, Rt = osol.synthetic_problem(300, 6, 2, 2, seed=3, depth=25)
    u0, a0 = osol.init_unsupervised("uniform_", V, 2, seed=1)
    with Problem(ctx, V, D, None) as p, Solver(p, u0, a0, L.DMF_MODE_UNSUPERVISED) as s:
        with pytest.raises(L.DemethifyHipError) as err:
            s.set_purity(np.full(6, 0.5))
        assert err.value.status == 1  # DMF_ERR_BAD_ARG
        assert "frank_wolfe" not in s.describe(20)
        s.step(1, 20, 0.0)  # (the solver is still the unsupervised one)
    u0, _, a0 = osol.init_partial_purity("uniform_", V, D, Rt, 2, None, seed=1)
    with Problem(ctx, V, D, Rt) as p, Solver(p, u0, a0) as s:
        for n in (5, 7, 0):
            with pytest.raises(ValueError):
                s.set_purity(np.full(n, 0.5))
        assert "frank_wolfe" not in s.describe(20)
        s.set_purity(np.full(6, 0.5))
        assert "alpha=k_alpha_frank_wolfe_row16" in s.describe(20)


@pytest.mark.gpu
@pytest.mark.parametrize("n_c,n_u,S,expect", [(4, 2, 13, (ROW16, V2X, I8)), (12, 5, 70, (GENERAL, CM_BU, I8))])
def test_step_is_resumable_under_purity(ctx, n_c, n_u, S, expect):
    """step(2) then step(1) equals step(3) bit for bit: nothing of the Frank-Wolfe phase lives on the host."""
    from demethify_amd.device import Problem, Solver

    V, D, Rt, purity, u0, a0 = _problem(900, S, n_c, n_u, 40, 0, 601)
    with Problem(ctx, V, D, Rt) as p:
        with Solver(p, u0, a0) as s:
            s.set_purity(purity)
            assert _kinds(s.describe(20)) == expect
            s.step(3, 20, 0.0)
            want = s.get()
        with Solver(p, u0, a0) as s:
            s.set_purity(purity)
            assert s.step(2, 20, 0.0)[0] == 2
            assert s.step(1, 20, 0.0)[0] == 3
            got = s.get()
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
