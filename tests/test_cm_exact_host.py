"""The model of k_cm_i8's per-row moments (tests/cm_exact.py) against scalar rational arithmetic, its launch plan against
the library's own (dmf_u_phase_describe: pure, no GPU), and the proof that the case table of tests/test_gpu_cm_exact.py
reaches every template instance and every launch-time split it claims.  No GPU."""
import math
import os
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import cm_exact as cm
import gram_exact as ge

from demethify_amd.device import u_phase_describe

CASES = cm.all_cases()


# ------------------------------------------------------------------------------------------------ the model
def _scalar_M(alpha_unk, Di):
    """model_M entry by entry: Fractions for the products and the sums, float() of an int / a Fraction for the one rounding
    (both round half to even), math.frexp for the exponents."""
    n_u, S = alpha_unk.shape
    N = Di.shape[0]
    out = np.zeros((N, n_u * (n_u + 1) // 2))
    for ip, (col0, sp) in enumerate(cm.panels(S)):
        a = alpha_unk[:, col0:col0 + sp].tolist()
        esc = []
        for j in range(n_u):
            mx = max(a[j])
            e = math.frexp(mx)[1]
            esc.append(0 if mx == 0 or mx >= 0.5 else min(-e, 200))
        for l in range(n_u):
            for j in range(l + 1):
                Z = [round(Fraction(math.ldexp(a[j][s], esc[j])) * Fraction(math.ldexp(a[l][s], esc[l])) * ge.TWO52) for s in range(sp)]
                for i in range(N):
                    total = sum(z * int(d) for z, d in zip(Z, Di[i, col0:col0 + sp].tolist()))
                    val = math.ldexp(float(total), -52 - esc[j] - esc[l])
                    p = l * (l + 1) // 2 + j
                    out[i, p] = val if ip == 0 else out[i, p] + val
    return out


def _edge_alpha(rs, n_u, S):
    """Unknown rows with the edge entries of the GPU cases: exactly 1.0, 0, rows at 2^-30 and 2^-250, a row that is zero in
    the first panel, entries on a rounding tie ((2 m + 1) 2^-53 against 1/2)."""
    a = rs.rand(n_u, S) * (2.0 ** -(np.arange(n_u) * 3 % 7))[:, None]
    a[0, ::5] = 1.0
    a[0, 1::5] = 0.0
    a[1] = (0.5 + 0.5 * rs.rand(S)) * 2.0 ** -250
    a[2] = (0.5 + 0.5 * rs.rand(S)) * 2.0 ** -30
    a[2, :cm.PANEL] = 0.0
    a[3, ::2] = 0.5
    a[4, ::2] = (2 * rs.randint(1, 1 << 40, size=len(a[4, ::2])) + 1) / float(1 << 53)
    return a


@pytest.mark.parametrize("N,S,nd", [(3, 7, 1), (2, 7, 2), (2, 258, 2), (1, 260, 1), (1, 513, 2)])
def test_panel_sums_against_fractions(N, S, nd):
    """A few hundred to a few thousand (pair, sample) entries per shape, edge entries included, one to three panels, a last
    panel of 1, 2 and 4 samples: the vectorised model equals scalar rational arithmetic bit for bit."""
    rs = np.random.RandomState(S + nd)
    a = _edge_alpha(rs, 5, S)
    top = 127 if nd == 1 else 32639
    Di = rs.randint(0, top + 1, size=(N, S)).astype(np.int64)
    Di[0, :5] = cm.PLANTED[nd][:5] if nd == 2 else (127, 0, 1, 64, 127)
    got = cm.model_M(a, Di)
    want = _scalar_M(a, Di)
    assert got.tobytes() == want.tobytes()
    # the row at 2^-250: esc stops at 200, its own pair rounds to nothing and its cross terms to a few units
    Z, esc = cm.panel_Z(a[:, :min(S, cm.PANEL)])
    assert esc[1] == 200 and not Z[2].any() and Z[1].max() <= 8        # pairs (1, 1) and (0, 1)
    if S > cm.PANEL:   # zero in the first panel, 2^-30 in the next: a different exponent per panel
        assert esc[2] == 0 and cm.esc_of(a[:, cm.PANEL:])[2] == 30


def test_esc_rule():
    a = np.array([[0.0, 0.0], [1.0, 0.2], [0.5, 0.1], [0.49, 0.3], [2.0 ** -30, 0.0], [2.0 ** -31 * 1.5, 0.0], [2.0 ** -250, 0.0],
                  [2.0 ** -200, 0.0], [2.0 ** -201, 0.0], [2.0 ** -199, 0.0]])
    assert cm.esc_of(a).tolist() == [0, 0, 0, 1, 29, 30, 200, 199, 200, 198]
    # ... and every scaled row has its largest entry in [1/2, 1) unless it is zero, at least 1/2, or beyond the cap
    sc = np.ldexp(a, cm.esc_of(a)[:, None].astype(np.int32)).max(axis=1)
    assert all(0.5 <= x < 1.0 for x in sc[[3, 4, 5, 7, 9]])


@pytest.mark.parametrize("nd", [1, 2])
@pytest.mark.parametrize("edge", ["", "headroom", "headroom_alt"])
def test_digit_accumulators_are_exact_and_in_range(nd, edge):
    """What the integer matrix cores hold: sum_w 256^w acc[w] IS the plain sum, every accumulator stays inside the bound the
    kernel's exactness argument names (256 samples x 128 x 128 per plane), and both halves of the epilogue fit a double."""
    c = cm.Case(33, 256 if edge != "headroom_alt" else 260, 0, 5, nd, edge, "")
    d = cm.make(c, "full")
    Z, _ = cm.panel_Z(d.alpha[:, :cm.PANEL])
    Dp = d.Di[:, :cm.PANEL]
    acc = cm.digit_accumulators(Z, Dp, nd)
    bound = cm.PANEL * 128 * 128 * nd
    assert len(acc) == 6 + nd and max(int(np.abs(a).max()) for a in acc) <= bound < (1 << 31)
    lo = sum(a.astype(object) * 256 ** w for w, a in enumerate(acc[:4]))
    hi = sum(a.astype(object) * 256 ** w for w, a in enumerate(acc[4:]))
    assert max(abs(int(x)) for x in lo.ravel()) < (1 << 53) and max(abs(int(x)) for x in hi.ravel()) < (1 << 53)
    plo, phi = cm.panel_sums(Z, Dp)
    assert ((hi << 32) + lo == (phi.astype(object) << 32) + plo.astype(object)).all()
    assert ((phi.astype(object) << 32) + plo.astype(object) == ge.exact(Z.T, Dp.T).T).all()
    if edge:
        z = cm.HEADROOM_Z if edge == "headroom" else cm.HEADROOM_ALT_Z
        want_digits = [-128] * 6 + [16] if edge == "headroom" else [127, -128, 127, -128, 127, -128, 16]
        assert [int(a[0]) for a in ge.balanced_digits(np.array([z]))] == want_digits
        p = 3 * 4 // 2 + 0   # the pair (0, 3): alpha_0 = 1, alpha_3 = z 2^-52
        assert (Z[p] == z).all() and (Dp[5] == cm.HEADROOM_COUNT[nd]).all()
        planes = [int(x[0]) for x in ge.count_digits(np.array([cm.HEADROOM_COUNT[nd]]), nd)]
        assert planes == ([127] if nd == 1 else [-128, 127])
        peak = max(abs(int(a[5, p])) for a in acc)
        # all digits at -128, planes (-128, 127): the two planes of a weight cancel but for weight 0 (256 x 128 x 128) and
        # weight 6 (digit 6 = 16 against plane 0, digit 5 against plane 1); alternating digits: both planes of a weight add
        # up, 256 x (128 x 128 + 127 x 127) -- the largest sum the data format can produce
        if nd == 1:
            assert peak == cm.PANEL * 128 * 127
        elif edge == "headroom":
            assert peak == cm.PANEL * (128 * 127 + 16 * 128) and int(acc[0][5, p]) == cm.PANEL * 128 * 128
        else:
            assert peak == cm.PANEL * (128 * 128 + 127 * 127)


def test_dyadic_family_has_one_right_answer():
    """From the magnitudes alone: every partial sum of c and M stays below 2^53 units at multiples of 2^-6 on every case --
    and would not at 2^-8 on the widest; the model of M then IS the plain sum."""
    for c in CASES:
        c_units, m_units = cm.dyadic_headroom(c)
        assert c_units < (1 << 53) and m_units < (1 << 53), c
    widest = max(CASES, key=lambda c: (1 + c.n_c) * c.S)
    assert widest.S == 2048 and widest.n_c == 48
    assert cm.dyadic_headroom(widest)[0] * 4 ** 3 >= (1 << 53)   # (alpha, R_trunc and V at 2^-8: 2^6 times the units)
    for c in CASES[::7]:
        d = cm.make(c, "dyadic")
        assert cm.model_M(d.alpha[c.n_c:], d.Di).tobytes() == cm.dyadic_M(c, d).tobytes(), c
        assert d.alpha.min() >= 0.0 and d.alpha.max() <= 1.0


def test_c_bound_counts_operations():
    c = cm.Case(33, 260, 5, 5, 1, "", "")
    # 8 chain links, one product, (4 + 1) column groups x 4 strips x 4 MFMAs, one panel addition
    assert cm.c_operations(c) == 8 + 1 + 4 * 4 * 5 + 1
    assert cm.c_operations(cm.Case(1, 2, 0, 5, 1, "", "")) == 0 + 1 + 16 + 0
    d = cm.make(c, "full")
    ref, A = cm.c_reference(c, d)
    # (the reference against a plain float64 evaluation: the same number to float64 accuracy, and the bound is not vacuous)
    plain = (d.D * (d.V - d.Rt @ d.alpha[:c.n_c])) @ d.alpha[c.n_c:].T
    assert np.allclose(plain, ref.astype(np.float64), rtol=1e-12, atol=0)
    assert cm.c_ratio(c, d, plain) < 1.0 and cm.c_ratio(c, d, plain * (1 + 1e-13)) > 1.0


# ------------------------------------------------------------------------------------------------ the plan
def test_plan_text_equals_the_library():
    """The plan re-derived in Python equals dmf_u_phase_describe for the stand-alone u phase of every case (whole string)."""
    for c in CASES:
        got = u_phase_describe(c.N, c.S, c.n_c, c.n_u, c.nd, 0, 20, 0, "update_u")
        assert got == cm.u_phase_text(c.N, c.S, c.n_c, c.n_u, c.nd), c
    # in the solver's loop the same producer runs in front of k_inner_bu where the integer Gram follows: the same plan
    got = u_phase_describe(1000, 128, 0, 12, 1, 0, 20, 0, "solver")
    assert got == "k_cm_i8<nd=1>+k_inner_bu " + cm.plan_text(1000, 128, 0, 12, 1)
    assert got == ("k_cm_i8<nd=1>+k_inner_bu panels=1 tiles=5 | col0=0 sp=128 k_cm_i8<0,1,2,s4> tpl=5 launches=1 ctiles=1 "
                   "lds=84480 grid=4 blocks/wave=1")   # 2 x 5 x 7 x 1024 + 12 rows x 132 doubles + 128


def test_every_launch_holds_a_tile():
    """(n_launch - 1) tpl < n_tiles on every shape the producer takes: a launch without tiles would size its LDS for ALL
    tiles (cm_layout reads 0 as "all").  The LDS bytes depend on the panel through its column-group count only, so one
    width per count (and the widths next to the seams) over every (n_c, n_u) is every supported shape; the library's text
    agrees with the re-derived plan wherever the selection sends the shape to the producer."""
    n_seen = n_lib = 0
    for S in (2, 64, 65, 128, 129, 192, 193, 256, 257, 320):
        for n_c in range(0, 49):
            for n_u in range(1, 33):
                if not cm.takes(S, n_c, n_u):
                    continue
                nmt = cm.n_tiles(n_u)
                for p in cm.plan(100, S, n_c, n_u, 1):
                    n_seen += 1
                    assert (p.launches - 1) * p.tpl < nmt and p.first.tiles >= 1 and p.last.tiles >= 1, (S, n_c, n_u, p)
                    assert p.first.lds <= cm.LDS_MAX and (p.launches - 1) * p.tpl + p.last.tiles == nmt
                if (n_c + n_u) % 3 == 0:   # a third of them through the library too
                    text = u_phase_describe(100, S, n_c, n_u, 1, 0, 20, 0, "update_u")
                    if text is not None and text.startswith("k_cm_i8<"):
                        n_lib += 1
                        assert text == cm.u_phase_text(100, S, n_c, n_u, 1), (S, n_c, n_u)
    assert n_seen > 10000 and n_lib > 2000


# ------------------------------------------------------------------------------------------------ coverage of the table
def test_every_instance_and_every_launch_class_is_in_the_table():
    inst, classes = set(), set()
    for c in CASES:
        assert cm.takes(c.S, c.n_c, c.n_u), c
        assert c.N * (c.n_u * (c.n_u + 1) // 2) * c.S <= cm.MODEL_WORK, c
        inst |= {p.inst for p in cm.plan(c.N, c.S, c.n_c, c.n_u, c.nd)}
        classes |= cm.classes_of(c)
    assert inst == set(cm.INSTANCES) and len(inst) == 48       # NKC {0,1,2,3,4,12} x ND {1,2} x NCGX {2,4} x S4
    assert classes == cm.LAUNCH_CLASSES, cm.LAUNCH_CLASSES - classes
    # ... the instances also at their smallest shapes, one case each, as the library names them
    named = set()
    for c in cm.instance_cases():
        text = u_phase_describe(c.N, c.S, c.n_c, c.n_u, c.nd, 0, 20, 0, "update_u")
        named.add(text.split(" k_cm_i8<")[1].split(">")[0])
    assert len(named) == 48


def test_shapes_and_edges_of_the_table():
    assert {c.S for c in CASES} >= set(cm.S_ALL) and {c.n_c for c in CASES} >= set(cm.NC_ALL)
    assert {c.n_u for c in CASES} == {1, 5, 16, 17, 25, 32}
    assert {c.N for c in CASES} >= {1, 31, 32, 33, 289, cm.BIG_N} and cm.BIG_N == 32 * 8 * 512 + 163
    assert all(c.n_c > 16 or c.S > 512 for c in CASES if c.n_u == 1)
    assert all(c.N <= 33 for c in CASES if c.S >= 2047)
    big = [c for c in CASES if c.N == cm.BIG_N][0]
    assert (big.S, big.n_u) == (8, 5) and "blocks/wave>1" in cm.classes_of(big)
    for nd in (1, 2):
        edges = set()
        for c in CASES:
            if c.nd == nd:
                edges |= cm.auto_edges(c)
        assert edges == {"vertex", "zerocov", "tiny", "zero30", "planted", "headroom", "headroom_alt"}, (nd, edges)
        for S in cm.S_ALL:   # every sample count under both digit-plane counts
            assert any(c.S == S and c.nd == nd for c in CASES), (S, nd)
    # the data delivers what the names say
    for c in (c for c in CASES if c.S in (260, 513) and c.n_u >= 5 and c.N >= 3 and not c.edge):
        for family in ("dyadic", "full"):
            d = cm.make(c, family)
            au = d.alpha[c.n_c:]
            assert au[c.n_u - 1, 0] == 1.0 and au[0, c.S - 1] == 1.0 and (au[:c.n_u - 1, 0] == 0).all()
            assert not d.Di[c.N // 2].any() and d.alpha.min() >= 0.0 and d.alpha.max() <= 1.0
            assert set(cm.PLANTED[c.nd]) <= set(np.unique(d.Di).tolist())
            e0, e1 = cm.esc_of(au[:, :cm.PANEL]), cm.esc_of(au[:, cm.PANEL:])
            assert e0[2] == 0 and e1[2] in (30, 31, 32, 33, 34, 35, 36) and not au[2, :cm.PANEL].any()
            assert e0[1] == (200 if family == "full" else e0[1]) and e0[1] >= 150
            assert len(set(e0.tolist())) >= 3                  # rows at different scales


def test_no_test_sets_the_producers_knobs():
    """DMF_CM_PER_CU (workgroups per CU) and DMF_CM_I8_MIN_NU (the selection threshold) change the plan: the expected texts
    hold only while nothing sets them."""
    here = Path(__file__).resolve()
    for name in ("DMF_CM_PER_CU", "DMF_CM_I8_MIN_NU"):
        assert name not in os.environ
        users = [p.name for p in here.parent.glob("*.py") if p != here and name in p.read_text()]
        assert users == [], (name, users)
