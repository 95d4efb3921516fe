"""Every template instance of k_rowpass_v2 against the oracle (oracle/solver.py), on both of its forms.

k_rowpass_v2<NKC, NU, MAXW, XS, PAIR> has 100 instances: known-type chunks NKC = 0..4 (n_c = 4 NKC - 3 .. 4 NKC; none in
unsupervised mode) x unknowns NU = 1..4 x five variants:

    V form (reads f64 V), MAXW 4        2..256 samples, when V is not an exact x / d or the X16 switch is off
    V form, MAXW 8                      257..512 samples
    X16 form, one block per cycle       2..64 samples; two waves with four unknowns; or the pair switch off
    X16 form, pair schedule             65..256 samples, except two waves with four unknowns
    X16 form, MAXW 8                    257..512 samples (no pair schedule)

For every (NKC, NU) a four-wave problem (2..4 waves) runs the V, X16 one-block and X16 pair legs, and an eight-wave problem
(5..8 waves) the V and X16 legs, each leg against one oracle run of its problem.  Both have a few more 16-row blocks than
the row pass's grid has workgroups, so that some workgroups loop (and pair, on the pair leg): 1.1e6 to 2.1e6 elements.  The
pair leg must agree with the one-block
leg bit for bit and the X16 legs with the V leg to 1e-12.  Cycles of different lengths spread the kinds of input over the
table, so that every variant meets each somewhere: unsupervised mode and padded R_trunc copies, full / one-short /
two-short / one-sample last column groups, all sixteen row tails, one and two count digits, zero-coverage stripes (with
V != 0 where d = 0 in some), 1 to 50 inner steps.  One more problem per NKC runs one wave at 2..64 samples.
test_every_instance_is_in_the_matrix (no GPU) holds the legs to the 100 instances through the selection table.

Further cases: workgroups that loop over several blocks on the V form and the eight-wave forms, inputs at the edges of the
integer encodings (count digits, exact 0 and 1 in alpha, u and R_trunc, constant rows), and inputs that the X16 acceptance
test takes with a small deviation or turns away."""
import ctypes as C
import itertools
from collections import namedtuple
from fractions import Fraction

import numpy as np
import pytest

from oracle import solver as osol

import rowpass_schedule_model as model
from conftest import rel_err
from test_gpu_rowpass_pair import _run

T1 = 3
TIGHT = 1e-8   # oracle parity, as in tests/test_gpu_bench_paths.py
PATHS = 1e-12  # the X16 form against the V form, as in tests/test_gpu_x16.py

# a leg: (name, the context's X16 switch, its pair switch).  The eight- and one-wave X16 legs keep the pair switch on: those
# shapes must not pair.
V_LEG, ONE_LEG, PAIR_LEG, X16_LEG = ("v", False, False), ("one", True, False), ("pair", True, True), ("x16", True, True)
FOUR_LEGS, OTHER_LEGS = (V_LEG, ONE_LEG, PAIR_LEG), (V_LEG, X16_LEG)

# zero: 0 no zero coverage, 1 zero-coverage stripes with V = 0 there, 2 the same with V != 0 there (must be ignored)
Case = namedtuple("Case", "N S n_c n_u n_iter2 depth zero seed")


def _nw(S):
    return (S + 63) // 64


def _grid(nw):
    """The row pass's workgroups for rows enough to fill it (tests/rowpass_schedule_model.py: the launch plan's rule)."""
    return model.plan(10 ** 7, 64 * nw, 0, 1)["grid"]


def _legs(S):
    return FOUR_LEGS if 2 <= _nw(S) <= 4 else OTHER_LEGS


def _instance(S, n_c, n_u, leg, x16=None, n_iter2=50):
    """(NKC, NU, MAXW, form, schedule) of the k_rowpass_v2 instance a leg runs, by the launch plan's rule; x16: whether the
    problem takes X16 (by default: with the leg's switch).  Schedule: "pair" for the pair schedule and the forms built on it
    (the 100 instances of this file are told apart by PAIR, and the launch counter these legs read counts them all)."""
    x16 = leg[1] if x16 is None else x16
    g = model.plan(16, S, n_c, n_u, n_iter2, x16=x16, pair=leg[2])
    return (g["nkc"], n_u, g["maxw"], "x16" if x16 else "v", "one" if g["schedule"] == "one" else "pair")


def _matrix():
    """(id, Case): for every (NKC, NU) a four-wave and an eight-wave problem, and one one-wave problem per NKC."""
    out = []
    for nkc, n_u in itertools.product(range(5), range(1, 5)):
        i = 4 * nkc + n_u - 1
        for w8 in (0, 1):
            nw = 5 + i % 4 if w8 else (2, 3, 4)[i % 3]
            if nw == 2 and n_u == 4:
                nw = 4  # (the pair schedule does not apply at two waves with four unknowns)
            S = (64 * nw, 64 * nw - 1, 64 * nw - 2, 64 * (nw - 1) + 1)[(i + i // 4 + w8) % 4]
            n_c = 4 * nkc - (3 * i + 2 * w8) % 4 if nkc else 0
            # a few more blocks than the grid has workgroups: one to seven workgroups run two blocks (a pair cycle on
            # the pair leg), the others one
            N = 16 * (_grid(nw) + 1 + 2 * (i % 4)) + (5 * i + 8 * w8) % 16
            n_iter2 = (20, 1, 7, 50)[(i // 3 + w8) % 4]
            depth = 400 if (i // 2 + w8) % 2 else 40
            out.append((f"w{8 if w8 else 4}-{nkc}-{n_u}",
                        Case(N, S, n_c, n_u, n_iter2, depth, (i + w8) % 3, 1000 * (w8 + 1) + i)))
    for nkc in range(5):
        S, n_u = (2, 3, 17, 63, 64)[nkc], (3, 1, 4, 2, 4)[nkc]
        N = 16 * max(1, 200_000 // (16 * S)) + (3 + 7 * nkc) % 16  # (2 and 3 samples: several blocks per workgroup)
        out.append((f"w1-{nkc}-{n_u}", Case(N, S, 4 * nkc - nkc % 4, n_u, (50, 7, 20, 1, 20)[nkc], (40, 400)[nkc % 2],
                                            nkc % 3, 3000 + nkc)))
    return out


MATRIX = _matrix()

# workgroups that run several blocks (grid: 2048 workgroups at one wave, 1024 at two, 512 at three or four, 256 at five to
# eight): 2..5 blocks each, an odd number of blocks, a ragged last block, on the V form at every wave class and both
# eight-wave forms (the X16 four-wave forms: tests/test_gpu_rowpass_pair.py)
LOOPS = [
    ("w1", Case(16 * 4398 + 3, 40, 5, 2, 20, 40, 1, 11)),     # 4399 blocks: 2 or 3 per workgroup
    ("w2", Case(16 * 2404 + 9, 66, 0, 3, 7, 40, 0, 12)),      # 2405 blocks: 2 or 3, one-sample last column group
    ("w3", Case(16 * 2124 + 11, 130, 9, 4, 7, 400, 2, 13)),   # 2125 blocks: 4 or 5, two count digits
    ("w4", Case(16 * 1124 + 13, 255, 16, 1, 20, 40, 0, 14)),  # 1125 blocks: 2 or 3
    ("w5", Case(16 * 600 + 7, 320, 12, 4, 20, 40, 1, 15)),    # 601 blocks: 2 or 3
    ("w8", Case(16 * 1100 + 3, 512, 3, 2, 7, 40, 0, 16)),     # 1101 blocks: 4 or 5
    ("w7", Case(16 * 1200 + 1, 449, 0, 4, 7, 400, 2, 17)),    # 1201 blocks: 4 or 5, one-sample last column group
]


def _data(c):
    """(V, D, Rt or None, u0, alpha0) of a Case."""
    V, D, Rt = osol.synthetic_problem(c.N, c.S, max(c.n_c, 1), c.n_u, seed=c.seed, depth=c.depth)
    if c.zero:
        rs = np.random.RandomState(c.seed + 7)
        D[rs.randint(0, 5)::rs.randint(3, 9), rs.randint(0, 2)::rs.randint(2, 5)] = 0
        V = np.where(D == 0, rs.uniform(0.05, 1.0, V.shape) if c.zero == 2 else 0.0, V)
    if c.n_c:
        Rt = np.ascontiguousarray(Rt[:, :c.n_c])
        u0, _, a0 = osol.init_partial("uniform_", V, D, Rt, c.n_u, seed=c.seed + 1)
    else:
        Rt = None
        u0, a0 = osol.init_unsupervised("uniform_", V, c.n_u, seed=c.seed + 1)
    return V, D, Rt, u0, a0


def _oracle(V, D, Rt, u0, a0, n_u, n_iter2):
    """(u, alpha, cost) after T1 outer iterations of the reference loop."""
    if Rt is not None:
        wu, wa = osol.solve_partial(u0.copy(), np.c_[Rt, u0], a0.copy(), V, D, Rt, n_u, T1, n_iter2, 0.0,
                                    project=osol.simplex_project_columns_fast)
        return wu, wa, osol.weighted_cost(V, np.c_[Rt, wu], wa, D)
    wu, wa = osol.solve_unsupervised(V, n_u, D, "uniform_", T1, n_iter2, 0.0, init=(u0.copy(), a0.copy()),
                                     project=osol.simplex_project_columns_fast)
    return wu, wa, osol.weighted_cost(V, wu, wa, D)


def _legs_against_oracle(ctx, record_property, data, n_iter2, legs, x16=None):
    """Runs every leg on one problem against one oracle run: path, launches, oracle parity; then the legs against each
    other.  x16=False: the problem must not take X16 whatever the switch says."""
    V, D, Rt, u0, a0 = data
    N, S = V.shape
    n_c, n_u = (0 if Rt is None else Rt.shape[1]), u0.shape[1]
    nd = 1 if D.max() <= 127 else 2
    wu, wa, want = _oracle(V, D, Rt, u0, a0, n_u, n_iter2)
    runs = {}
    for leg in legs:
        name = leg[0]
        desc, trail, direct, launches = _run(ctx, V, D, Rt, u0, a0, n_iter2, T1, leg[2], x16=leg[1])
        nkc, _, _, form, sched = _instance(S, n_c, n_u, leg, x16=None if x16 is None else leg[1] and x16, n_iter2=n_iter2)
        assert f"rowpass=k_rowpass_v2<{nkc},{n_u}> nw={_nw(S)} " in desc, (name, desc)
        assert f" tail={N % 16} " in desc and f"gram=k_gram_i8<nd={nd}>" in desc, (name, desc)
        assert (" x16 " in desc) if form == "x16" else ("x16" not in desc), (name, desc)
        assert launches == (T1, T1 if sched == "pair" else 0), (name, launches)
        u, alpha, cost, it = trail[-1]
        assert it == T1, (name, it)
        du, da = float(np.abs(u - wu).max()), float(np.abs(alpha - wa).max())
        record_property(f"{name}_oracle_du", du)
        record_property(f"{name}_oracle_da", da)
        assert du < TIGHT and da < TIGHT, (name, du, da)
        assert cost == pytest.approx(want, rel=1e-9) and direct == pytest.approx(want, rel=1e-11), (name, cost, direct, want)
        runs[name] = (trail, direct)
    for name in ("one", "x16"):  # the X16 form against the V form
        if name in runs and "v" in runs:
            for k, (a, b) in enumerate(zip(runs[name][0], runs["v"][0])):
                eu, ea = rel_err(a[0], b[0]), rel_err(a[1], b[1])
                record_property(f"{name}_vs_v_rel_{k}", max(eu, ea))
                assert eu <= PATHS and ea <= PATHS, (name, k, eu, ea)
    if "pair" in runs:  # the pair schedule against the one-block loop: the same sums in the same order
        for k, (a, b) in enumerate(zip(runs["one"][0], runs["pair"][0])):
            for what, x, y in zip(("u", "alpha", "cost", "iterations"), a, b):
                assert np.array_equal(x, y), (k, what)
        assert runs["one"][1] == runs["pair"][1]
    return runs


# ----------------------------------------------------------------------------------------- no GPU
def test_every_instance_is_in_the_matrix():
    """Every leg of MATRIX describes (dmf_select_describe, level 0) as the instance, wave count and form it claims, and the
    legs cover all 100 instances: a selection change that moves a case off its instance fails here first."""
    from demethify_amd import _lib as L

    lib = L.load()
    seen = set()
    for cid, c in MATRIX:
        nd = 2 if c.depth > 127 else 1
        for leg in _legs(c.S):
            nkc, nu, maxw, form, sched = inst = _instance(c.S, c.n_c, c.n_u, leg, n_iter2=c.n_iter2)
            flags = L.DMF_SELECT_COUNTS_F32_EXACT | (L.DMF_SELECT_X16 if form == "x16" else 0)
            buf = C.create_string_buffer(512)
            assert lib.dmf_select_describe(c.N, c.S, c.n_c, c.n_u, nd, 0, c.n_iter2, flags, buf, len(buf)) == L.DMF_OK
            got = buf.value.decode()
            want = f"rowpass=k_rowpass_v2<{nkc},{nu}> nw={_nw(c.S)} grid="
            assert got.startswith(want), (cid, leg, got)
            assert f" tail={c.N % 16}{' x16' if form == 'x16' else ''} gram=k_gram_i8<nd={nd}>" in got, (cid, leg, got)
            assert (maxw == 8) == (c.S > 256) and (sched == "pair") == (leg is PAIR_LEG), (cid, leg)
            assert f" grid={min(_grid(_nw(c.S)), (c.N + 15) // 16)} " in got, (cid, got)
            assert c.N * c.S <= 2_200_000 and 1 <= c.n_iter2 <= 50, cid
            assert (c.N + 15) // 16 > _grid(_nw(c.S)) or cid.startswith("w1"), cid  # some workgroups run two blocks
            seen.add(inst)
    want = {(nkc, nu, maxw, form, sched) for nkc, nu in itertools.product(range(5), range(1, 5))
            for maxw, form, sched in ((4, "v", "one"), (8, "v", "one"), (4, "x16", "one"), (4, "x16", "pair"),
                                      (8, "x16", "one"))}
    assert len(want) == 100 and seen == want, sorted(want - seen)


# ----------------------------------------------------------------------------------------- instance matrix
@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for _, c in MATRIX], ids=[cid for cid, _ in MATRIX])
def test_instance_matrix_against_oracle(ctx, record_property, case):
    data = _data(case)
    assert (data[1].max() > 127) == (case.depth > 127)
    _legs_against_oracle(ctx, record_property, data, case.n_iter2, _legs(case.S))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for _, c in LOOPS], ids=[cid for cid, _ in LOOPS])
def test_several_blocks_per_workgroup_against_oracle(ctx, record_property, case):
    legs = (V_LEG, X16_LEG)  # (at two to four waves the X16 leg pairs: that loop is covered bit for bit elsewhere)
    _legs_against_oracle(ctx, record_property, _data(case), case.n_iter2, legs)


# ----------------------------------------------------------------------------------------- edges of the integer encodings
EDGE_SHAPES = [Case(3000 + 5, 192, 12, 4, 20, 40, 0, 21), Case(1500 + 9, 129, 0, 2, 7, 40, 1, 22),
               Case(1200 + 3, 384, 7, 3, 20, 40, 0, 23), Case(900 + 14, 449, 16, 1, 50, 40, 2, 24)]


def _with_count(data, count, seed):
    """The largest count made exactly `count`: a few cells hold it, one with x = 0 and one with x = d."""
    V, D, Rt, u0, a0 = data
    V, D = V.copy(), D.copy()
    rs = np.random.RandomState(seed)
    cells = [tuple(rs.randint(0, n) for n in D.shape) for _ in range(6)]
    for k, (r, c) in enumerate(cells):
        x = 0 if k == 0 else count if k == 1 else int(rs.randint(0, count + 1))
        D[r, c] = count
        V[r, c] = x / count
    assert D.max() == count
    return V, D, Rt, u0, a0


def _simplex_and_box_edges(data):
    """alpha0 with simplex-vertex columns and exact zeros (and unknown mass left: else the reference's own l_w is 0),
    u0 and R_trunc with exact 0 and 1 entries: fixed-point features at exactly 0 and 2^52."""
    V, D, Rt, u0, a0 = data
    u0, a0 = u0.copy(), a0.copy()
    K, S = a0.shape
    for j in range(0, S, 5):
        a0[:, j] = 0.0
        a0[(j // 5) % K, j] = 1.0
    for j in (j for j in range(2, S, 7) if j % 5):
        a0[j % K, j] = 0.0
        a0[:, j] /= a0[:, j].sum()
    assert np.linalg.norm(a0[K - u0.shape[1]:]) > 0.1
    u0[::7] = 0.0
    u0[3::11] = 1.0
    if Rt is not None:
        Rt = Rt.copy()
        Rt[::5] = 0.0
        Rt[2::9, ::2] = 1.0
    return V, D, Rt, u0, a0


def _constant_rows(data):
    """Fully methylated (V = 1) and unmethylated (V = 0) rows."""
    V, D, Rt, u0, a0 = data
    V = V.copy()
    V[::13] = 1.0
    V[5::17] = 0.0
    return V, D, Rt, u0, a0


EDGES = {"count_127": lambda d, s: _with_count(d, 127, s), "count_128": lambda d, s: _with_count(d, 128, s),
         "count_32639": lambda d, s: _with_count(d, 32639, s), "simplex_box": lambda d, s: _simplex_and_box_edges(d),
         "constant_rows": lambda d, s: _constant_rows(d)}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", range(len(EDGE_SHAPES)))
@pytest.mark.parametrize("edge", list(EDGES))
def test_encoding_edges_against_oracle(ctx, record_property, edge, shape):
    c = EDGE_SHAPES[shape]
    data = EDGES[edge](_data(c), c.seed + 5)
    if edge.startswith("count_"):
        assert data[1].max() == int(edge[6:])  # 127: nd=1; 128 and 32639: nd=2 (_legs_against_oracle checks it)
    _legs_against_oracle(ctx, record_property, data, c.n_iter2, _legs(c.S))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [0, 2])
def test_counts_beyond_two_digits_leave_the_row_pass(ctx, shape):
    """32640: no integer copies of the counts (two balanced 8-bit digits end at 32639), no X16: another row pass, the
    same results."""
    c = EDGE_SHAPES[shape]
    V, D, Rt, u0, a0 = _with_count(_data(c), 32640, c.seed + 5)
    wu, wa, want = _oracle(V, D, Rt, u0, a0, c.n_u, c.n_iter2)
    desc, trail, direct, launches = _run(ctx, V, D, Rt, u0, a0, c.n_iter2, T1, True)
    assert "k_rowpass_v2" not in desc and "x16" not in desc and "k_gram_i8" not in desc, desc
    assert launches == (0, 0)
    u, alpha, cost, _ = trail[-1]
    assert np.abs(u - wu).max() < TIGHT and np.abs(alpha - wa).max() < TIGHT
    assert cost == pytest.approx(want, rel=1e-9) and direct == pytest.approx(want, rel=1e-11)


# ----------------------------------------------------------------------------------------- X16 acceptance, inexact inputs
UNIT = Fraction(1, 2 ** 53)  # kX16MaxDev = 8 UNIT of max(x, 1)


def _dev(v, d):
    """|v d - x| / max(x, 1) in UNITs, exactly (x = rint(v d))."""
    p = Fraction(float(v)) * int(d)
    x = round(p)
    return abs(p - x) / max(x, 1) / UNIT


def _nudged(V, D, cells, lo, hi, limit=None):
    """V with each cell moved up by whole ulps until its deviation reaches lo UNITs; cells that overshoot hi stay as
    they were.  At most `limit` cells move.  Returns (V, deviations of the moved cells)."""
    V = V.copy()
    devs = []
    for r, c in cells:
        if len(devs) == limit:
            break
        d = int(D[r, c])
        x = round(Fraction(float(V[r, c])) * d)
        w = V[r, c]
        for _ in range(64):
            w = np.nextafter(w, 2.0)
            dev = _dev(w, d)
            if dev >= lo:
                break
        if lo <= dev <= hi and round(Fraction(float(w)) * d) == x:
            V[r, c] = w
            devs.append(dev)
    return V, devs


def _inner_cells(V, D, n, seed):
    """n cells with 0 < x < d, in random order."""
    rs = np.random.RandomState(seed)
    X = np.rint(V * D)
    r, c = np.nonzero((X > 0) & (X < D))
    pick = rs.choice(len(r), size=n, replace=False)
    return list(zip(r[pick], c[pick]))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [0, 2])
def test_small_deviations_take_x16(ctx, record_property, shape):
    """Deviations of 2..4 UNITs (half the acceptance bound or less, clear of its edge) on a few hundred cells: the
    problem takes X16 and computes what the oracle computes on that same V."""
    c = EDGE_SHAPES[shape]
    V, D, Rt, u0, a0 = _data(c)
    V, devs = _nudged(V, D, _inner_cells(V, D, 600, c.seed), 2, 4)
    assert len(devs) >= 200 and 2 <= min(devs) and max(devs) <= 4, (len(devs), float(min(devs)), float(max(devs)))
    # (every other cell is x / d rounded once: within 1 UNIT)
    _legs_against_oracle(ctx, record_property, (V, D, Rt, u0, a0), c.n_iter2, _legs(c.S))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [0, 2])
def test_one_large_deviation_falls_back_to_v(ctx, record_property, shape):
    """One cell 16 UNITs or more off (twice the bound): the whole problem keeps V, on every leg."""
    c = EDGE_SHAPES[shape]
    V0, D, Rt, u0, a0 = _data(c)
    V, devs = _nudged(V0, D, _inner_cells(V0, D, 40, c.seed + 1), 16, 64, limit=1)
    assert len(devs) == 1 and np.count_nonzero(V != V0) == 1
    _legs_against_oracle(ctx, record_property, (V, D, Rt, u0, a0), c.n_iter2, _legs(c.S), x16=False)
