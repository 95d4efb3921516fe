"""The per-row moments of the split u phase as k_cm_i8 (csrc/dmf_kernels_cm_i8.hip) must deliver them -- M_i predicted bit
for bit, c_i exactly on dyadic data and inside a derived bound otherwise -- the launch plan of the producer written down
independently of the library, and the case table that reaches every template instance and every launch-time split.  A plain
helper module like tests/gram_exact.py: tests/test_cm_exact_host.py checks it without a GPU, tests/test_gpu_cm_exact.py runs
it through Solver.row_moments().

The model of M.  The kernel walks the samples in PANELS of 256.  Per panel and unknown type j it takes mx = the largest entry
of alpha's row j over the panel's columns and esc[j] = 0 when mx = 0 or mx >= 1/2, else min(-frexp(mx).exp, 200): the power
of two that puts the row's largest entry into [1/2, 1).  A pair p = l (l + 1) / 2 + j (j <= l) and a sample s give
    Z[p][s] = z_int(ldexp(alpha_js, esc_j), ldexp(alpha_ls, esc_l)) = rint(product 2^52), rounded once (gram_exact.z_int),
seven balanced base-256 digits; the counts are one or two balanced digits (gram_exact.count_digits); the integer matrix
cores sum every digit product exactly in i32 (|sum| <= 256 x 128 x 128 x 2 = 2^23), digit t and plane c at weight 256^(t + c).
The epilogue joins weights 0..3 into lo and 4..7 into hi by FMAs that are exact (|lo|, |hi| < 2^49) and returns
ldexp(fma(hi, 2^32, lo), -52 - esc_j - esc_l): lo + 2^32 hi IS sum_s Z[p][s] d[i][s], so the panel's contribution is that
exact integer rounded ONCE to double, half to even, and scaled by a power of two (no result is subnormal: esc <= 200).  Any
split of the integer into two halves that a double holds exactly gives the same rounding: `panel_sums` splits Z at bit 32,
sums in int64 and carries lo's overflow into hi, and gram_exact.finish does the rounding.  The first panel stores, every
later one adds with one float64 addition, in panel order (a wave owns its rows; the panels follow each other on the stream).

c_i[j] = sum_s alpha_js d_is (v_is - sum_k Rt_ik alpha_ks) runs on the FP64 matrix cores and has no bit-exact model; two data
families pin it.

  dyadic: V, R_trunc and alpha are multiples of 2^-6 (an alpha row of the edge data: of 2^-36 or 2^-156 throughout the row
  -- the row at 2^-250 exists in the full family only: there esc stops at its cap of 200, the scaled entries are about
  2^-50 and their digits ROUND, so M is the model's and not the plain sum),
  the counts integers.  e = v - sum Rt alpha is a multiple of 2^-12 below 49, d e below 2^15 x 49, a term alpha d e a multiple
  of the row's unit 2^-6 x 2^-12 and any partial sum of at most 2048 of them below 2^6 x 2^15 x 49 x 2^12 x 2^11 < 2^50 units:
  every product and every partial sum, in any order, is representable (`dyadic_headroom` asserts it from the magnitudes; with
  multiples of 2^-8 the same count gives 2^56 and fails).  So c has ONE right answer, `dyadic_c`, and M, a sum of multiples of
  2^-12 below 2^38 units, equals the plain sum_s alpha_j alpha_l d (`dyadic_M`) -- which ties the digit model to the
  mathematics, since the model must give the same.

  full: uniform doubles.  c is held to  |c - exact| <= n u A,  u = 2^-53,  A = sum_s alpha_js d_is (|v_is| + sum_k |Rt_ik
  alpha_ks|)  (the sum of the absolute values of all terms), n = the operations one result passes through:
      4 ceil(n_c / 4)   FMAs of the chain e = v - sum_k Rt_k alpha_k (the padded links multiply by zero but are issued),
      1                 product w = d e,
      4 per strip       v_mfma_f64_16x16x4 instructions that add a strip's 16 samples into the accumulator, one accumulation
                        each (four strips per 64-sample column group of every panel, the padded ones included),
      1 per panel after the first: the addition into cm.
  Each operation commits at most one relative error u on a quantity that A bounds, and later operations carry it on
  unamplified to first order: n u A.  (Counting an MFMA as ONE rounded accumulation of its four products is the tighter
  reading; an implementation that rounds after each product stays within four times the accumulation term.  The measured
  ratio is printed per case -- "DEV c ..." -- and is far below either.)  The reference is an x87 extended-precision sum
  whose own error, at most (n_c + S + 8) 2^-64 A, is taken OFF the limit (`c_ratio`).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import gram_exact as ge

PANEL = 256             # samples per launch
WAVES = 8               # waves per workgroup, 32 rows each at a time
LDS_MAX = 160 * 1024    # dynamic LDS a launch may take
LDS_TWO_PER_CU = 76 * 1024
NKC_WIDE = 12           # the instance for more than 16 known types
ESC_MAX = 200
NKC_ALL = (0, 1, 2, 3, 4, NKC_WIDE)
INSTANCES = tuple((nkc, nd, ncgx, s4) for nkc in NKC_ALL for nd in (1, 2) for ncgx in (2, 4) for s4 in (True, False))


# ------------------------------------------------------------------------------------------------ the plan, from Python
def layout_bytes(Sp, n_c, n_u, tiles):
    """Dynamic LDS of a launch over a panel of Sp samples that holds `tiles` 16-pair tiles: the P digit table
    [column group][tile][7 digits][64 lanes] x 16 bytes, the alpha copy (4 ceil(n_c / 4) + n_u rows of 64 ncg + 4 doubles)
    and 32 exponents."""
    ncg = (Sp + 63) // 64
    return ncg * tiles * 7 * 64 * 16 + ((n_c + 3) // 4 * 4 + n_u) * (64 * ncg + 4) * 8 + 32 * 4


def panels(S):
    return [(c0, min(PANEL, S - c0)) for c0 in range(0, S, PANEL)]


def n_tiles(n_u):
    return (n_u * (n_u + 1) // 2 + 15) // 16


def takes(S, n_c, n_u):
    """The producer's own limits (cm_i8_supported), alignment aside -- and the solver's: a shape needs a fall-back u phase
    to exist at all, and beyond 1792 samples (k_u_step_direct's LDS) that is k_u_phase_gram, up to 16 unknowns."""
    return (1 <= n_u <= 32 and 0 <= n_c <= 48 and n_c + n_u <= 64 and 2 <= S <= 2048 and (S <= 1792 or n_u <= 16)
            and layout_bytes(min(S, PANEL), n_c, n_u, 1) <= LDS_MAX)


Launch = namedtuple("Launch", "tiles lds grid blocks_per_wave")
Panel = namedtuple("Panel", "col0 sp inst tpl launches fit first last")


def plan(N, S, n_c, n_u, nd):
    """cm_i8_plan written down independently: one Panel per 256 samples.  fit: the tiles the LDS would hold at once."""
    nmt, n_ct = n_tiles(n_u), (n_u + 15) // 16
    nkc = (n_c + 3) // 4 if n_c <= 16 else NKC_WIDE
    nblk = (N + 31) // 32
    out = []
    for col0, sp in panels(S):
        fit = max([t for t in range(1, nmt + 1) if layout_bytes(sp, n_c, n_u, t) <= LDS_MAX] or [1])
        launches = max(-(-nmt // fit), n_ct)
        tpl = -(-nmt // launches)

        def launch(li):
            mt0 = min(li * tpl, nmt)
            tiles = min(mt0 + tpl, nmt) - mt0
            lds = layout_bytes(sp, n_c, n_u, tiles)
            grid = min(-(-nblk // WAVES), 256 * (2 if lds <= LDS_TWO_PER_CU else 1))
            return Launch(tiles, lds, grid, -(-nblk // (grid * WAVES)))

        inst = (nkc, nd, 4 if sp > 128 else 2, sp % 4 == 0 and S % 2 == 0)
        out.append(Panel(col0, sp, inst, tpl, launches, fit, launch(0), launch(launches - 1)))
    return out


def _launch_text(l):
    return f"lds={l.lds} grid={l.grid} blocks/wave={l.blocks_per_wave}"


def plan_text(N, S, n_c, n_u, nd):
    """What dmf_solver_row_moments answers, and what dmf_u_phase_describe appends to the rowpass= text."""
    pl = plan(N, S, n_c, n_u, nd)
    out = [f"panels={len(pl)} tiles={n_tiles(n_u)}"]
    for p in pl:
        nkc, ndp, ncgx, s4 = p.inst
        t = (f"col0={p.col0} sp={p.sp} k_cm_i8<{nkc},{ndp},{ncgx},{'s4' if s4 else 'pairs'}> tpl={p.tpl} launches={p.launches} "
             f"ctiles={(n_u + 15) // 16} {_launch_text(p.first)}")
        if p.last.tiles != p.first.tiles:
            t += f" last: tiles={p.last.tiles} {_launch_text(p.last)}"
        out.append(t)
    return " | ".join(out)


def u_phase_text(N, S, n_c, n_u, nd):
    """dmf_u_phase_describe of the stand-alone u phase (route update_u) on the integer producer."""
    return f"k_cm_i8<nd={nd}>+k_u_inner_rows " + plan_text(N, S, n_c, n_u, nd)


def classes_of(c):
    """The launch-time classes a case reaches, as strings (the coverage list of tests/test_cm_exact_host.py)."""
    pl = plan(c.N, c.S, c.n_c, c.n_u, c.nd)
    out = {"panels=1" if len(pl) == 1 else "panels=2" if len(pl) == 2 else "panels>=3"}
    if len(pl) > 1 and pl[-1].sp <= 4:
        out.add(f"last-panel={pl[-1].sp}")
    out.add(f"ctiles={(c.n_u + 15) // 16}")
    nmt, n_ct = n_tiles(c.n_u), (c.n_u + 15) // 16
    for p in pl:
        if p.launches == 1:
            out.add("launches=1")
        elif -(-nmt // p.fit) >= n_ct and p.fit < nmt:
            out.add("launches>1:lds")
        if p.launches == n_ct > -(-nmt // p.fit):
            out.add("launches>1:ctile")
        for l in (p.first, p.last):
            out.add("lds<=76K" if l.lds <= LDS_TWO_PER_CU else "lds>76K")
            if l.blocks_per_wave > 1:
                out.add("blocks/wave>1")
    return out


LAUNCH_CLASSES = {"panels=1", "panels=2", "panels>=3", "last-panel=1", "last-panel=2", "last-panel=3", "last-panel=4", "ctiles=1",
                  "ctiles=2", "launches=1", "launches>1:lds", "launches>1:ctile", "lds<=76K", "lds>76K", "blocks/wave>1"}


# ------------------------------------------------------------------------------------------------ the model of M
def pair_index(n_u):
    """(j, l) of pair p = l (l + 1) / 2 + j, j <= l, as two index arrays."""
    J = np.array([j for l in range(n_u) for j in range(l + 1)])
    Lq = np.array([l for l in range(n_u) for j in range(l + 1)])
    return J, Lq


def esc_of(a):
    """a: the unknown rows of alpha over ONE panel (n_u x Sp) -> the scaling exponents of the rows (int64)."""
    mx = a.max(axis=1)
    _, e = np.frexp(mx)
    return np.where((mx > 0.0) & (e < 0), np.minimum(-e.astype(np.int64), ESC_MAX), 0).astype(np.int64)


def panel_Z(a):
    """-> (Z, esc): Z[p][s] of one panel (NP x Sp int64)."""
    esc = esc_of(a)
    sc = np.ldexp(a, esc[:, None].astype(np.int32))
    J, Lq = pair_index(a.shape[0])
    return ge.z_int(sc[J], sc[Lq]), esc


def panel_sums(Z, d):
    """sum_s Z[p][s] d[i][s] as (lo, hi) with lo in [0, 2^32) and the sum = hi 2^32 + lo exactly: N x NP int64 each (both
    exact in a double)."""
    Z, d = np.asarray(Z, dtype=np.int64), np.asarray(d, dtype=np.int64)
    assert d.shape[1] <= PANEL and (d.size == 0 or (int(d.min()) >= 0 and int(d.max()) <= 32639))
    m32 = (1 << 32) - 1
    lo_raw = d @ (Z & m32).T      # < 2^32 x 2^15 x 2^8 = 2^55
    hi_raw = d @ (Z >> 32).T      # < 2^21 x 2^15 x 2^8
    hi = hi_raw + (lo_raw >> 32)
    assert hi.size == 0 or int(hi.max()) < (1 << 53)
    return lo_raw & m32, hi


def model_M(alpha_unk, Di):
    """What k_cm_i8 must leave in the M part of cm: N x NP float64, bit for bit."""
    n_u, S = alpha_unk.shape
    J, Lq = pair_index(n_u)
    M = None
    for col0, sp in panels(S):
        Z, esc = panel_Z(alpha_unk[:, col0:col0 + sp])
        lo, hi = panel_sums(Z, Di[:, col0:col0 + sp])
        val = np.ldexp(ge.finish(lo, hi), -(esc[J] + esc[Lq])[None, :].astype(np.int32))
        M = val if M is None else M + val   # the first panel stores, the later ones add
    return M


def digit_accumulators(Z, d, nd):
    """The eight (seven with one count digit) i32 accumulators of the integer matrix cores per (row, pair), by digit weight:
    list of N x NP int64.  For the host checks of the exactness argument."""
    A, Cd = ge.balanced_digits(Z), ge.count_digits(d, nd)
    acc = [np.zeros((d.shape[0], Z.shape[0]), dtype=np.int64) for _ in range(7 + nd - 1)]
    for t, a in enumerate(A):
        for c, cd in enumerate(Cd):
            acc[t + c] += cd @ a.T
    return acc


# ------------------------------------------------------------------------------------------------ cases
# edge: "" | "headroom" | "headroom_alt" (see make); every case carries the automatic edges of `auto_edges`
Case = namedtuple("Case", "N S n_c n_u nd edge why")

S_ALL = (2, 3, 4, 5, 6, 7, 64, 65, 127, 128, 129, 130, 131, 132, 255, 256, 257, 258, 259, 260, 513, 2047, 2048)
NC_ALL = (0, 1, 4, 5, 8, 12, 16, 17, 48)
NU_ALL = (5, 16, 17, 25, 32, 1)
N_ALL = (1, 31, 32, 33, 289)   # 289: a full workgroup of eight 32-row blocks and one row of a second
MODEL_WORK = 2.2e7             # N x pairs x S the host model is asked for at most


def cid(c):
    return f"N{c.N}-S{c.S}-{c.n_c}+{c.n_u}-nd{c.nd}{'-' + c.edge if c.edge else ''}"


def _fit(N, S, n_c, n_u):
    """The nearest shape the producer takes and the model affords: one unknown only behind many known types or samples."""
    if n_u == 1 and not (n_c > 16 or S > 512):
        n_c = 17
    order = [n_u] + [x for x in (25, 17, 16, 5, 1) if x < n_u]
    for nu in order:
        if nu == 1 and not (n_c > 16 or S > 512):
            continue
        if takes(S, n_c, nu):
            for n in (N, 33):
                if n * (nu * (nu + 1) // 2) * S <= MODEL_WORK:
                    return n, n_c, nu
    raise AssertionError((N, S, n_c, n_u))


def sample_cases():
    """Every S of the list under both digit-plane counts; n_c, n_u and N rotate through their lists."""
    out = []
    for i, S in enumerate(S_ALL):
        for nd in (1, 2):
            k = 2 * i + nd - 1
            N, n_c, n_u = _fit(N_ALL[k % 5], S, NC_ALL[(k * 2 + i) % 9], NU_ALL[(k + i // 3) % 6])
            out.append(Case(N, S, n_c, n_u, nd, "", "sample edge"))
    return out


INSTANCE_S = {(2, True): 4, (2, False): 6, (4, True): 132, (4, False): 130}   # (NCGX, S4) -> the smallest S of the issue's list
INSTANCE_NC = {0: 0, 1: 1, 2: 5, 3: 12, 4: 16, NKC_WIDE: 17}


def instance_cases():
    """All 48 instances <NKC, ND, NCGX, S4> at their smallest sample count; n_u and N rotate."""
    out = []
    for a, nkc in enumerate(NKC_ALL):
        for nd in (1, 2):
            for b, (key, S) in enumerate(sorted(INSTANCE_S.items())):
                k = 8 * a + 4 * (nd - 1) + b
                out.append(Case((31, 32, 33, 1)[k % 4], S, INSTANCE_NC[nkc], (5, 16, 17)[k % 3], nd, "", f"instance {nkc},{nd},{key}"))
    return out


BIG_N = 32 * 8 * 512 + 163


def special_cases():
    out = [Case(BIG_N, 8, 0, 5, 1, "", "two blocks per wave: persistent loop, next-block prefetch, R_trunc hand-over (NKC = 0)"),
           Case(32 * 8 * 512 + 33, 4, 5, 5, 2, "", "two blocks per wave with known types: the R_trunc rows handed over")]
    for nd in (1, 2):
        out += [
            Case(33, 256, 0, 5, nd, "headroom", "every balanced digit of Z at -128 on a full panel of the largest planes"),
            Case(33, 260, 4, 5, nd, "headroom_alt", "digits alternating 127 / -128: both planes add up in every accumulator"),
            Case(289, 128, 12, 16, nd, "", "a full workgroup and one row of a second"),
            Case(33, 256, 0, 32, nd, "", "33 tiles in 11 launches: the LDS bound"),
            Case(33, 260, 3, 25, nd, "", "21 tiles: LDS bound in the full panel, c-tile minimum in the 4-sample one"),
            Case(31, 64, 8, 17, nd, "", "10 tiles fit one launch: two launches for the two c tiles"),
            Case(32, 2048, 48, 1, nd, "", "the widest: eight panels, twelve chain links"),
            Case(33, 2047, 17, 5, nd, "", "eight panels, the last one 255 samples, rows 8 bytes off"),
            Case(33, 513, 0, 32, nd, "", "three panels, the last one sample wide, both c tiles full"),
        ]
    return out


def all_cases():
    seen, out = set(), []
    for c in instance_cases() + sample_cases() + special_cases():
        if c[:6] not in seen:
            seen.add(c[:6])
            out.append(c)
    return out


def auto_edges(c):
    """The edge data every case carries where its shape has room: alpha columns on a vertex (always), a zero-coverage row
    (N >= 3), an alpha row at 2^-250 (n_u >= 3), an alpha row that is zero in the first panel and about 2^-30 in the later
    ones (n_u >= 4, two panels or more), the planted counts (8 cells or more)."""
    out = {"vertex"}
    if c.N >= 3:
        out.add("zerocov")
    if c.n_u >= 3:
        out.add("tiny")
    if c.n_u >= 4 and c.S > PANEL:
        out.add("zero30")
    if c.N * c.S >= 8:
        out.add("planted")
    if c.edge:
        out.add(c.edge)
    return out


# ------------------------------------------------------------------------------------------------ data
HEADROOM_Z = (1 << 52) - 0x808080808080                     # digits -128 x 6, 16
HEADROOM_ALT_Z = (16 << 48) + sum((127 if t % 2 == 0 else -128) << (8 * t) for t in range(6))   # 127, -128, 127, ...
PLANTED = {1: (127, 0, 1, 64), 2: (32639, 128, 32384, 127, 0)}
HEADROOM_COUNT = {1: 127, 2: 32384}                         # planes (127) and (-128, 127)

Data = namedtuple("Data", "family V D Di Rt alpha Vi Ri Ai rexp")


def counts(rs, c):
    """Integer counts of a case: nd = 1 uniform in [0, 127]; nd = 2 a mixture of small counts and, in a third of the cells,
    counts from 128 up to 32639; a tenth zeros; the planted values; a zero-coverage row."""
    N, S, nd = c.N, c.S, c.nd
    if nd == 1:
        Di = rs.randint(0, 128, size=(N, S)).astype(np.int64)
    else:
        Di = rs.randint(0, 300, size=(N, S)).astype(np.int64)
        big = rs.rand(N, S) < 0.33
        Di[big] = rs.randint(128, 32640, size=int(big.sum()))
    Di[rs.rand(N, S) < 0.1] = 0
    if c.edge in ("headroom", "headroom_alt"):
        Di[:N - 1, :PANEL] = HEADROOM_COUNT[nd]
    if N >= 3:
        Di[N // 2, :] = 0
    flat = Di.reshape(-1)
    vals = PLANTED[nd]
    for k, v in enumerate(vals):      # spread over the array, first and last cell included, the zero-coverage row left alone
        at = (k * (flat.size - 1)) // (len(vals) - 1)
        flat[at + S if N >= 3 and at // S == N // 2 else at] = v
    if N * S >= 8:
        assert set(vals) <= set(np.unique(Di).tolist()), (c, vals)
    elif nd == 2:
        flat[0] = 32639               # (a handful of cells: the second plane is still not empty)
    return Di


def _apply_vertices(A, n_c, n_u, S, one):
    """Columns on a vertex of the simplex: column 0 on the last unknown type, column S - 1 (S >= 4) on the first, column 1
    (with known types, S >= 5) on a known type -- zero unknown mass.  (The narrowest shapes keep a column of full digits.)"""
    A[:, 0] = 0
    A[n_c + n_u - 1, 0] = one
    if S >= 4:
        A[:, S - 1] = 0
        A[n_c, S - 1] = one
    if n_c and S >= 5:
        A[:, 1] = 0
        A[0, 1] = one


def make(c, family):
    """The data of a case: family "dyadic" (integers Vi, Ri, Ai with V = Vi / 64, Rt = Ri / 64, alpha row k = Ai[k] 2^rexp[k])
    or "full" (uniform doubles), with the edges of auto_edges(c)."""
    rs = np.random.RandomState(1000 * c.S + 37 * c.n_c + c.n_u + c.nd + c.N % 97 + (7 if family == "full" else 0))
    N, S, n_c, n_u, K = c.N, c.S, c.n_c, c.n_u, c.n_c + c.n_u
    Di = counts(rs, c)
    edges = auto_edges(c)
    rexp = np.full(K, -6, dtype=np.int64)
    if family == "dyadic":
        Vi = rs.randint(0, 65, size=(N, S)).astype(np.int64)
        Ri = rs.randint(0, 65, size=(N, n_c)).astype(np.int64)
        Ai = rs.randint(0, 65, size=(K, S)).astype(np.int64)
        Ai[n_c:] >>= (np.arange(n_u) * 3 % 7)[:, None]      # rows whose largest entry lies below 1/2: esc 0 .. 6
        if "tiny" in edges:
            Ai[n_c + 1] = rs.randint(1, 65, size=S)
            rexp[n_c + 1] = -156      # (not 2^-250: beyond the cap of 200 the kernel's digits round, see the docstring)
        if "zero30" in edges:
            Ai[n_c + 2] = rs.randint(1, 65, size=S)
            Ai[n_c + 2, :PANEL] = 0
            rexp[n_c + 2] = -36
        _apply_vertices(Ai, n_c, n_u, S, 64)
        if c.edge in ("headroom", "headroom_alt"):            # (alpha_j = alpha_l = 1: digit 6 at 16 throughout the panel)
            Ai[n_c, :PANEL] = 64
            Ai[n_c + 3, :PANEL] = 64
        for k in range(n_c, K):                               # an entry of exactly 1.0 needs the row's unit at 2^-6
            if rexp[k] != -6:
                Ai[k][Ai[k] == 64] = 63
        alpha = np.ldexp(Ai.astype(np.float64), rexp[:, None].astype(np.int32))
        return Data(family, Vi / 64.0, Di.astype(np.float64), Di, (Ri / 64.0) if n_c else None, alpha, Vi, Ri, Ai, rexp)
    V = rs.rand(N, S)
    Rt = rs.rand(N, n_c)
    alpha = rs.rand(K, S)
    alpha[n_c:] *= (2.0 ** -(np.arange(n_u) * 3 % 7))[:, None]
    if "tiny" in edges:
        alpha[n_c + 1] = (0.5 + 0.5 * rs.rand(S)) * 2.0 ** -250
    if "zero30" in edges:
        alpha[n_c + 2] = (0.5 + 0.5 * rs.rand(S)) * 2.0 ** -30
        alpha[n_c + 2, :PANEL] = 0.0
    _apply_vertices(alpha, n_c, n_u, S, 1.0)
    if c.edge in ("headroom", "headroom_alt"):
        z = HEADROOM_Z if c.edge == "headroom" else HEADROOM_ALT_Z
        alpha[n_c, :PANEL] = 1.0
        alpha[n_c + 3, :PANEL] = z / float(ge.TWO52)          # (exact: z < 2^53)
    return Data(family, V, Di.astype(np.float64), Di, Rt if n_c else None, alpha, None, None, None, None)


# ------------------------------------------------------------------------------------------------ dyadic: the one right answer
def dyadic_headroom(c):
    """The largest number of units any partial sum of c (unit 2^-18 of the row's scale) and of M (2^-12) can reach on the
    dyadic family, from the magnitudes alone: must stay below 2^53."""
    e_max = 64 * 64 * (1 + c.n_c)                 # |v - sum Rt alpha| in units of 2^-12
    return 64 * 32639 * e_max * c.S, 64 * 64 * 32639 * c.S


def dyadic_c(c, d):
    """c exactly: (sum_s Ai_js d_is (64 Vi_is - sum_k Ri_ik Ai_ks)) 2^(rexp_j - 12)."""
    n_c = c.n_c
    E = 64 * d.Vi - (d.Ri @ d.Ai[:n_c] if n_c else 0)
    ci = (d.Di * E) @ d.Ai[n_c:].T
    assert ci.size == 0 or int(np.abs(ci).max()) < (1 << 53)
    return np.ldexp(ci.astype(np.float64), (d.rexp[n_c:] - 12)[None, :].astype(np.int32))


def dyadic_M(c, d):
    """M exactly: (sum_s Ai_js Ai_ls d_is) 2^(rexp_j + rexp_l)."""
    J, Lq = pair_index(c.n_u)
    Au = d.Ai[c.n_c:]
    mi = d.Di @ (Au[J] * Au[Lq]).T
    assert mi.size == 0 or int(mi.max()) < (1 << 53)
    r = d.rexp[c.n_c:]
    return np.ldexp(mi.astype(np.float64), (r[J] + r[Lq])[None, :].astype(np.int32))


# ------------------------------------------------------------------------------------------------ full: the bound on c
def c_operations(c):
    """n of the module docstring."""
    strips = sum(4 * ((sp + 63) // 64) for _, sp in panels(c.S))
    return 4 * ((c.n_c + 3) // 4) + 1 + 4 * strips + len(panels(c.S)) - 1


def c_reference(c, d):
    """(ref, A) in extended precision: c and the sum of the absolute values of its terms (N x n_u longdouble each)."""
    ld = np.longdouble
    assert np.finfo(ld).nmant >= 63, "this platform's long double is no wider than double: no cheap accurate reference"
    n_c = c.n_c
    V, D, al = d.V.astype(ld), d.D.astype(ld), d.alpha.astype(ld)
    if n_c:
        Rt = d.Rt.astype(ld)
        known = Rt @ al[:n_c]            # every term non-negative: also the sum of the |terms|
    else:
        known = np.zeros_like(V)
    ref = (D * (V - known)) @ al[n_c:].T
    A = (D * (V + known)) @ al[n_c:].T
    return ref, A


def c_ratio(c, d, got):
    """max over the entries of |got - ref| / (n 2^-53 A - the reference's own error); 0 where A = 0 requires got = 0.  <= 1
    is the bound of the module docstring."""
    ld = np.longdouble
    ref, A = c_reference(c, d)
    lim = (ld(c_operations(c)) * ld(2.0) ** -53 - ld(c.n_c + c.S + 8) * ld(2.0) ** -64) * A
    err = np.abs(np.asarray(got, dtype=np.float64).astype(ld) - ref)
    zero = A == 0
    if zero.any() and (err[zero] != 0).any():
        return float("inf")
    if zero.all():
        return 0.0
    return float((err[~zero] / lim[~zero]).max())
