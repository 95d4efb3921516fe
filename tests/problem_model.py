"""What the three problem builders must leave on the device -- dmf_problem_create, dmf_problem_gather / _gather_device and
dmf_problem_mask (csrc/dmf_api_problem.hip) -- written down from host arrays in numpy, Python integers and Fraction, and the
case table of tests/test_gpu_problem_copies.py.  A plain helper module like tests/gram_exact.py: it imports nothing from
the library; tests/test_problem_model_host.py checks it without a GPU, tests/test_gpu_problem_copies.py holds
Problem.report() / Problem.copy_out() to it.

The model states the builders' CONTRACT, not a re-creation: a gather of a problem with integer count copies keeps the
source's digit count ND and its exactness flags (max |D - f32(D)|, R_trunc outside [0, 1], x16_dev) and takes max(D) and
the sum of x from the gathered rows; a mask does the same with the kept elements.  Padding is part of the contract: rows
N .. N16 and samples S .. SD of D16 / X16 / W16, the digits of rows >= N in Dt8 and the columns n_c .. 4 ceil(n_c / 4) of the
padded R_trunc copy are ZERO, because the row pass, k_cm_i8 and the integer Gram read them without guards.

Every comparison is equality, with one exception: ||R_trunc||_F^2 is a floating-point sum in an order the launch geometry
decides, so off a grid where every partial sum is representable it is held to |got - exact| <= (n + 4) 2^-53 exact, n = N n_c
(the bound derived in the docstring of tests/test_gpu_gram_exact.py: non-negative terms, one rounding per square, n additions
in any order)."""
from __future__ import annotations

from collections import namedtuple
from fractions import Fraction

import numpy as np

CONSTS = ("kDsq", "kRtSumsq", "kDmax", "kF32ResidualMax", "kIntCountMax", "kRtOutsideUnit")   # order of the device array
ARRAYS = ("V", "D", "Rt", "Rtp", "D16", "X16", "W16", "Dt8", "mask_bits")
X16_MAX_DEV = 8.0 * 2.0 ** -53   # kX16MaxDev
COUNT_MAX = 32639                # two balanced digits: (d + 128) >> 8 <= 127
ONE_DIGIT_MAX = 127
RT_GRID = 1 << 10                # R_trunc on multiples of 2^-10: squares on 2^-20, sums exact while n 2^20 < 2^53


class Model:
    """One resident problem: shapes, arrays (None = the problem has no such array), constants."""

    def __init__(self):
        self.N = self.S = self.n_c = 0
        self.ND = self.SD = self.N16 = self.plane_stride = 0
        self.V = self.D = self.Rt = self.Rtp = self.D16 = self.X16 = self.W16 = self.Dt8 = self.mask_bits = None
        self.rtp_width = 0
        self.rtp_borrows_rt = False
        self.consts = {}                  # name -> float; kRtSumsq is not in it
        self.rt_sumsq = Fraction(0)       # the exact sum
        self.rt_on_grid = True            # every partial sum representable: the device's sum must EQUAL float(rt_sumsq)
        self.x16_dev = 0.0
        self.x16_sum = 0
        self.n_test = 0
        self.d_f32_exact = False

    def copy(self):
        m = Model()
        m.__dict__.update(self.__dict__)
        m.consts = dict(self.consts)
        return m


# ------------------------------------------------------------------------------------------------ pieces
def count_shapes(N, S):
    """alloc_count_copies: -> (SD, N16, plane_stride)."""
    SD = (S + 63) // 64 * 64
    return SD, (N + 15) // 16 * 16, ((N + 31) // 32) * (SD // 32) * 1024


def pad_u16(A, N16, SD):
    """An N x S integer array as u16 [N16][SD], zero padded."""
    out = np.zeros((N16, SD), dtype=np.uint16)
    out[:A.shape[0], :A.shape[1]] = A
    return out


def dt8_of(D16, N, nd):
    """The digit planes of the first N rows of D16 ([N16][SD] u16) in the MFMA B layout: int8 [nd][ceil(N / 32)][SD / 32][32][32],
    Dt8[plane, rb, sb, n, k] = digit of D16[32 rb + k, 32 sb + n]; rows >= N: digit 0 in every plane."""
    SD = D16.shape[1]
    RB, SB = (N + 31) // 32, SD // 32
    d = np.zeros((RB * 32, SD), dtype=np.int16)   # (d + 128 <= 32767: 16 bits hold every step below)
    assert D16.size == 0 or int(D16.max()) <= COUNT_MAX
    d[:N] = D16[:N]
    if nd == 1:
        planes = [d]
    else:
        assert nd == 2
        planes = [((d + 128) % 256) - 128, (d + 128) >> 8]   # (a padding row's d = 0 gives digits 0 and 0)
    out = np.empty((nd, RB, SB, 32, 32), dtype=np.int8)
    for c, pl in enumerate(planes):
        assert pl.size == 0 or (int(pl.min()) >= -128 and int(pl.max()) <= 127)
        out[c] = pl.reshape(RB, 32, SB, 32).transpose(0, 2, 3, 1)   # [rb, k, sb, n] -> [rb, sb, n, k]
    return out


def dt8_decode(Dt8):
    """Back to counts: plane0 + 256 plane1 with the tile transpose undone -> int64 [32 RB][SD]."""
    nd, RB, SB = Dt8.shape[:3]
    d = Dt8[0].astype(np.int64)
    if nd == 2:
        d = d + 256 * Dt8[1].astype(np.int64)
    return d.transpose(0, 3, 1, 2).reshape(RB * 32, SB * 32)


def _exact_dev(v, d, x):
    """fma(v, d, -x) as the hardware returns it: the exact v d - x, rounded once."""
    return float(Fraction(v) * int(d) - int(x))


def x16_of(V, D):
    """The methylated read counts of k_build_d16: per element with d > 0, x = rint(v d), accepted iff 0 <= x <= d and
    |v d - x| <= 8 2^-53 max(x, 1) with v d - x the exact difference rounded once (Fraction, then float()); d = 0: x = 0
    whatever v is.  -> (X int64 N x S or None if any element is rejected, largest |v d - x| / max(x, 1) as a double, sum of
    x as a Python int, number of rejected elements).  Where V lies on the grid of 2^-20 inside [0, 2] every v d (below 2^36
    units of 2^-20) and every v d - x is a double, so float arithmetic IS the exact arithmetic and no Fraction is needed."""
    V = np.asarray(V, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)
    live = D > 0.0
    P = np.where(live, V * D, 0.0)
    X = np.rint(P)
    err = np.zeros(V.shape)
    on_grid = bool(np.all((V >= 0.0) & (V <= 2.0) & (V * 1048576.0 == np.rint(V * 1048576.0))))
    if on_grid:
        err = np.abs(P - X)
    else:
        for i, j in zip(*np.nonzero(live)):
            err[i, j] = abs(_exact_dev(float(V[i, j]), D[i, j], X[i, j]))
    xm = np.maximum(X, 1.0)
    ok = ~live | ((X >= 0.0) & (X <= D) & (err <= X16_MAX_DEV * xm))
    n_bad = int((~ok).sum())
    if n_bad:
        return None, 0.0, 0, n_bad
    Xi = X.astype(np.int64)
    dev = float((err / xm)[live].max()) if live.any() else 0.0
    return Xi, dev, int(Xi.sum()), 0


def rt_sumsq_of(Rt):
    """-> (exact sum of squares as a Fraction, whether every square and partial sum is a double)."""
    if Rt is None or Rt.size == 0:
        return Fraction(0), True
    R = np.asarray(Rt, dtype=np.float64)
    G = R * RT_GRID
    if np.all(G == np.rint(G)) and float(np.abs(G).max()) <= 4 * RT_GRID and R.size * 16 * RT_GRID * RT_GRID < (1 << 53):
        Gi = G.astype(np.int64)
        return Fraction(int((Gi * Gi).sum()), RT_GRID * RT_GRID), True
    return sum((Fraction(float(x)) ** 2 for x in R.ravel().tolist()), Fraction(0)), False


def rtp_of(m):
    """The padded R_trunc copy: width 4 ceil(n_c / 4), zero padded; R_trunc itself when n_c % 4 == 0; none for n_c = 0 or
    n_c > 48."""
    if not 0 < m.n_c <= 48:
        m.Rtp, m.rtp_width, m.rtp_borrows_rt = None, 0, False
        return
    w = (m.n_c + 3) // 4 * 4
    m.Rtp = np.zeros((m.N, w))
    m.Rtp[:, :m.n_c] = m.Rt
    m.rtp_width, m.rtp_borrows_rt = w, w == m.n_c


def _rt_consts(m):
    m.rt_sumsq, m.rt_on_grid = rt_sumsq_of(m.Rt)
    m.consts["kDsq"] = m.consts["kDmax"] * m.consts["kDmax"]
    m.d_f32_exact = m.consts["kF32ResidualMax"] == 0.0


def _no_count_copies(m):
    m.ND = m.SD = m.N16 = m.plane_stride = 0
    m.D16 = m.X16 = m.W16 = m.Dt8 = None
    m.x16_dev, m.x16_sum = 0.0, 0


# ------------------------------------------------------------------------------------------------ the three builders
def created(V, D, Rt, x16=True, level=0):
    """dmf_problem_create on host arrays (D: counts as doubles or integers; Rt: N x n_c or None); x16: the context's
    X16 switch; level: its kernel-selection level when the problem is created."""
    m = Model()
    m.V = np.array(V, dtype=np.float64)
    m.D = np.array(D, dtype=np.float64)
    m.N, m.S = m.V.shape
    m.Rt = np.array(Rt, dtype=np.float64) if Rt is not None and np.asarray(Rt).shape[1] > 0 else None
    m.n_c = 0 if m.Rt is None else m.Rt.shape[1]
    integral = bool(np.all((m.D >= 0.0) & (m.D == np.rint(m.D))))
    m.consts = {
        "kDmax": float(m.D.max()),
        "kF32ResidualMax": float(np.abs(m.D - m.D.astype(np.float32).astype(np.float64)).max()),
        "kIntCountMax": float(m.D.max()) if integral else float("inf"),
        "kRtOutsideUnit": 0.0 if m.Rt is None or bool(np.all((m.Rt >= 0.0) & (m.Rt <= 1.0))) else 1.0,
    }
    _rt_consts(m)
    _no_count_copies(m)
    if (level == 0 and m.consts["kIntCountMax"] <= COUNT_MAX and m.consts["kRtOutsideUnit"] == 0.0 and 2 <= m.S <= 2048
            and m.n_c <= 48):
        m.ND = 1 if m.consts["kIntCountMax"] <= ONE_DIGIT_MAX else 2
        m.SD, m.N16, m.plane_stride = count_shapes(m.N, m.S)
        m.D16 = pad_u16(m.D.astype(np.int64), m.N16, m.SD)
        m.Dt8 = dt8_of(m.D16, m.N, m.ND)
        if x16:
            X, dev, xsum, _ = x16_of(m.V, m.D)
            if X is not None:
                m.X16, m.x16_dev, m.x16_sum = pad_u16(X, m.N16, m.SD), dev, xsum
    rtp_of(m)
    return m


def gathered(src, idx, x16=True, level=0):
    """dmf_problem_gather(_device) of rows idx (any length >= 1, repeats allowed) of the problem `src` models."""
    idx = np.asarray(idx, dtype=np.int64).ravel()
    Rt = src.Rt[idx] if src.Rt is not None else None
    if not (src.ND > 0 and level == 0):
        return created(src.V[idx], src.D[idx], Rt, x16=x16, level=level)
    m = Model()
    m.N, m.S, m.n_c = int(idx.size), src.S, src.n_c
    m.V, m.D, m.Rt = src.V[idx].copy(), src.D[idx].copy(), (Rt.copy() if Rt is not None else None)
    m.ND = src.ND
    m.SD, m.N16, m.plane_stride = count_shapes(m.N, m.S)
    assert m.SD == src.SD
    m.D16 = np.zeros((m.N16, m.SD), dtype=np.uint16)
    m.D16[:m.N] = src.D16[idx]
    m.Dt8 = dt8_of(m.D16, m.N, m.ND)
    dmax = float(m.D16.max())
    m.consts = {"kDmax": dmax, "kIntCountMax": dmax, "kF32ResidualMax": src.consts["kF32ResidualMax"],
                "kRtOutsideUnit": src.consts["kRtOutsideUnit"]}
    if src.X16 is not None and x16:
        m.X16 = np.zeros((m.N16, m.SD), dtype=np.uint16)
        m.X16[:m.N] = src.X16[idx]
        m.x16_dev, m.x16_sum = src.x16_dev, int(m.X16.sum(dtype=np.int64))
    _rt_consts(m)
    rtp_of(m)
    return m


def pack_bits(mask):
    """N x S bool -> the bit-packed train mask (sample s = bit s & 7 of byte s >> 3 of its row, padding bits 0)."""
    return np.packbits(np.asarray(mask, dtype=bool), axis=1, bitorder="little")


def masked(src, mask, x16=True, level=0, bits=None):
    """dmf_problem_mask of the problem `src` models: mask N x S bool, True = kept.  bits: the packed mask as it was handed
    over, where it differs from pack_bits(mask) in its padding bits (they are kept as they came)."""
    mask = np.asarray(mask, dtype=bool)
    assert mask.shape == (src.N, src.S)
    m = Model()
    m.N, m.S, m.n_c = src.N, src.S, src.n_c
    m.V, m.D = np.where(mask, src.V, 0.0), np.where(mask, src.D, 0.0)
    m.Rt = src.Rt.copy() if src.Rt is not None else None
    m.mask_bits = pack_bits(mask) if bits is None else np.array(bits, dtype=np.uint8)
    m.n_test = int((~mask).sum())
    ints = src.ND > 0 and level == 0
    _no_count_copies(m)
    if ints:
        m.ND, m.SD, m.N16, m.plane_stride = src.ND, src.SD, src.N16, src.plane_stride
        keep = pad_u16(mask, m.N16, m.SD).astype(bool)
        m.D16 = np.where(keep, src.D16, 0).astype(np.uint16)
        m.W16 = pad_u16(~mask, m.N16, m.SD)
        m.Dt8 = dt8_of(m.D16, m.N, m.ND)
        if src.X16 is not None and x16:
            m.X16 = np.where(keep, src.X16, 0).astype(np.uint16)
            m.x16_dev, m.x16_sum = src.x16_dev, int(m.X16.sum(dtype=np.int64))
    dmax = max(float(m.D.max()), 0.0)
    m.consts = {"kDmax": dmax, "kF32ResidualMax": src.consts["kF32ResidualMax"],
                "kIntCountMax": dmax if np.isfinite(src.consts["kIntCountMax"]) else src.consts["kIntCountMax"],
                "kRtOutsideUnit": src.consts["kRtOutsideUnit"]}
    _rt_consts(m)
    rtp_of(m)
    return m


# ------------------------------------------------------------------------------------------------ comparison
REPORT_INTS = ("N", "S", "n_c", "ND", "SD", "N16", "plane_stride", "has_D16", "has_X16", "has_W16", "has_Dt8", "has_mask_bits",
               "rtp_width", "rtp_borrows_rt", "n_test", "d_f32_exact")


def as_readback(m):
    """What Problem.report() and Problem.copy_out() answer for a problem that is exactly the model: (report dict, arrays
    dict with None for the arrays the problem does not have, "consts" included)."""
    rep = {"N": m.N, "S": m.S, "n_c": m.n_c, "ND": m.ND, "SD": m.SD, "N16": m.N16, "plane_stride": m.plane_stride,
           "has_D16": int(m.D16 is not None), "has_X16": int(m.X16 is not None), "has_W16": int(m.W16 is not None),
           "has_Dt8": int(m.Dt8 is not None), "has_mask_bits": int(m.mask_bits is not None), "rtp_width": m.rtp_width,
           "rtp_borrows_rt": int(m.rtp_borrows_rt), "n_test": m.n_test, "d_f32_exact": int(m.d_f32_exact)}
    rep.update(m.consts)
    rep["kRtSumsq"] = float(m.rt_sumsq)
    rep["x16_dev"], rep["x16_sum"] = m.x16_dev, float(m.x16_sum)
    arrays = {k: (None if getattr(m, k) is None else np.array(getattr(m, k))) for k in ARRAYS}
    arrays["consts"] = np.array([rep[k] for k in CONSTS])
    return rep, arrays


def rt_sumsq_ok(got, m):
    """Equality on the grid; elsewhere |got - exact| <= (n + 4) 2^-53 exact with n = N n_c, in rational arithmetic."""
    if m.rt_on_grid:
        return got == float(m.rt_sumsq)
    n = m.N * m.n_c
    return abs(Fraction(float(got)) - m.rt_sumsq) <= Fraction(n + 4, 1 << 53) * m.rt_sumsq


def compare(name, report, arrays, m, say=print):
    """Holds one read-back problem (report: Problem.report(); arrays: name -> what Problem.copy_out gave, None where the
    call answered that the problem has no such array; "consts": the device copy of the constants) to the model.  Says, per
    scalar class and per array, how many elements differ and where the first one is, then asserts that nothing does."""
    want, want_arrays = as_readback(m)
    failures = []
    bad = [k for k in REPORT_INTS if int(report[k]) != int(want[k])]
    say(f"{name}: report integers: {len(bad)} of {len(REPORT_INTS)} differ" +
        "".join(f"; {k} = {report[k]} want {want[k]}" for k in bad))
    failures += bad
    dbl = [k for k in CONSTS if k != "kRtSumsq"] + ["x16_dev", "x16_sum"]
    bad = [k for k in dbl if not float(report[k]) == float(want[k])]
    say(f"{name}: constants, x16_dev, x16_sum: {len(bad)} of {len(dbl)} differ" +
        "".join(f"; {k} = {report[k]!r} want {want[k]!r}" for k in bad))
    failures += bad
    ok = rt_sumsq_ok(report["kRtSumsq"], m)
    rel = abs(Fraction(float(report["kRtSumsq"])) - m.rt_sumsq) / m.rt_sumsq if m.rt_sumsq else Fraction(0)
    say(f"{name}: kRtSumsq = {report['kRtSumsq']!r}, exact {float(m.rt_sumsq)!r}, off by {float(rel) * 2.0 ** 53:.3f} x 2^-53 "
        f"relative; held to {'equality' if m.rt_on_grid else f'{m.N * m.n_c + 4} x 2^-53'}")
    if not ok:
        failures.append("kRtSumsq")
    for k in list(ARRAYS) + ["consts"]:
        got, exp = arrays.get(k), want_arrays[k]
        if k == "consts" and got is not None:
            # the device copy is the host copy, bit for bit (kRtSumsq included: whatever the sum came to, both hold it)
            exp = np.array([float(report[c]) for c in CONSTS])
        if got is None or exp is None:
            if (got is None) != (exp is None):
                say(f"{name}: {k}: {'absent' if got is None else 'present'}, want {'absent' if exp is None else 'present'}")
                failures.append(k)
            else:
                say(f"{name}: {k}: absent, as it must be")
            continue
        got = np.asarray(got)
        if got.shape != exp.shape or got.dtype != exp.dtype:
            say(f"{name}: {k}: shape {got.shape} {got.dtype}, want {exp.shape} {exp.dtype}")
            failures.append(k)
            continue
        diff = got != exp
        n_bad = int(np.count_nonzero(diff))
        where = ""
        if n_bad:
            first = np.unravel_index(int(diff.argmax()), diff.shape)
            where = f", first at {tuple(int(i) for i in first)}: {got[first]!r} want {exp[first]!r}"
            failures.append(k)
        say(f"{name}: {k}: {n_bad} of {got.size} elements differ{where}")
    assert not failures, (name, failures)


# ------------------------------------------------------------------------------------------------ data
def true_data(N, S, n_c, seed, max_count, rt_grid=True, zero_fraction=0.1, max_at=(0, 0)):
    """Read counts as a sequencer gives them: integer depths d in [0, max_count] (about `zero_fraction` zeros, the maximum
    planted at max_at), methylated reads x <= d, v = fl(x / d) (0.5 where d = 0), and R_trunc in [0, 1] -- on the grid of
    2^-10 (its sum of squares has one right answer) or full-mantissa doubles.  -> (V, D int64, Rt or None)."""
    rs = np.random.RandomState(seed)
    D = rs.randint(0, max(min(max_count, 60), 1) + 1, size=(N, S)).astype(np.int64)
    if max_count > 127:   # a few cells per row block above one digit, spread wide
        big = rs.rand(N, S) < 0.05
        D[big] = rs.randint(128, max_count + 1, size=int(big.sum()))
    D[rs.rand(N, S) < zero_fraction] = 0
    D[max_at] = max_count
    X = np.floor(rs.rand(N, S) * (D + 1)).astype(np.int64)
    X = np.minimum(X, D)
    with np.errstate(invalid="ignore", divide="ignore"):
        V = np.where(D > 0, X / np.where(D > 0, D, 1), 0.5)
    Rt = None
    if n_c:
        Rt = rs.randint(0, RT_GRID + 1, size=(N, n_c)) / float(RT_GRID) if rt_grid else rs.rand(N, n_c)
        Rt[N - 1] = 1.0   # (the last row, last padded column's neighbour: a padding write one short would lose it)
    return np.ascontiguousarray(V), D, Rt


def grid_data(N, S, n_c, seed, max_count=100):
    """The same with v on {0, 1/4, 1/2, 3/4, 1} wherever d allows an exact integer v d, so that x16_of needs no Fraction:
    for shapes of a million rows."""
    rs = np.random.RandomState(seed)
    D = rs.randint(0, max_count + 1, size=(N, S)).astype(np.int64)
    D[0, 0] = max_count
    q = rs.randint(0, 5, size=(N, S))              # quarters
    q = np.where(D % 4 == 0, q, np.where(D % 2 == 0, q // 2 * 2, q // 4 * 4))
    V = q / 4.0
    Rt = rs.randint(0, RT_GRID + 1, size=(N, n_c)) / float(RT_GRID) if n_c else None
    return V, D, Rt


# ------------------------------------------------------------------------------------------------ the case table
Case = namedtuple("Case", "N S n_c why")

TAILS = [
    Case(77, 13, 3, "row tails of 16 (N16 = 80) and of 32 (3 row blocks, 13 rows in the last), one sample block pair, n_c % 4 = 3"),
    Case(33, 2, 0, "N = 1 mod 32, the smallest S with integer copies, no known types: no Rt, no Rtp"),
    Case(1, 2, 1, "one row: 15 padding rows in D16, 31 zero rows in the only Dt8 tile, n_c % 4 = 1"),
    Case(257, 130, 2, "N = 1 mod 256, three column blocks of 64 (SD = 192, 62 padding samples), n_c % 4 = 2"),
    Case(96, 300, 1, "N a multiple of 32, ten sample blocks of 32 (SD = 320)"),
    Case(50, 1, 2, "S = 1: no integer copies at all"),
    Case(64, 64, 4, "nothing to pad anywhere, Rtp is R_trunc itself"),
]

# the grid-stride tails: one long thin problem that exceeds every clamp of the builders' launches
BIG = Case(1_048_613, 2, 1, "every clamped launch runs its grid-stride loop at least twice in some workgroup")

# the pool's keep threshold (csrc/dmf_api_context.hip: kKeepMinBytes, kKeepPerSize)
KEEP_MIN_BYTES, KEEP_PER_SIZE = 1 << 20, 3
RECYCLED = Case(8197, 127, 13, "D16 / X16 / W16, one plane of Dt8 and Rtp each reach the keep threshold of the pool")

GATHER_SOURCE_N = 1000
GATHER_LENGTHS = (1, 15, 16, 17, 31, 33, 1000, 2500)


def clamps(N, S, n_c, n_idx=None):
    """Per clamped launch of the builders: (workgroups the unclamped formula asks for, the clamp), from the shapes alone --
    the arithmetic of launch_gather_rows, launch_gather_counts_int, launch_mask_problem, launch_build_counts_int,
    launch_build_dt8, launch_pad_rows, reduce_blocks, launch_convert_counts and launch_index_range_check."""
    n_idx = N if n_idx is None else n_idx
    SD, N16, _ = count_shapes(N, S)
    SDg, N16g, _ = count_shapes(n_idx, S)
    nct = (n_c + 3) // 4 * 4
    cdiv = lambda a, b: (a + b - 1) // b
    return {
        "k_gather_rows": (cdiv(n_idx, 4), 65536),
        "k_gather_rows_u16": (cdiv(N16g, 4), 2048),
        "k_mask_rows": (cdiv(N16, 4), 4096),
        "k_build_d16": (cdiv(N16 * (SD // 8), 256), 8192),
        "k_build_dt8": (cdiv(cdiv(N, 32) * (SD // 32), 4), 16384),
        "k_pad_rows": (cdiv(N * nct, 256), 8192),
        "k_reduce_partial": (min(cdiv(N * S, 256), cdiv(N * n_c, 256)), 1024),   # both the scans of D and those of Rt
        "k_convert_counts": (cdiv(N * S, 256), 8192),
        "k_index_range_check": (cdiv(n_idx, 256), 1024),
    }


def pool_sizes(N, S, n_c, nd):
    """Bytes of the allocations whose padding the recycled-memory case is about."""
    SD, N16, plane_stride = count_shapes(N, S)
    return {"D16 / X16 / W16": N16 * SD * 2, "Dt8": plane_stride * nd, "Rtp": N * ((n_c + 3) // 4 * 4) * 8}


def planted_source(N, S, n_c, seed, row, top, base_max=60, rt_grid=True):
    """true_data with every count at most base_max, except in ONE row: `row` holds `top` (its first sample) and, where top
    exceeds one digit, further counts in [128, top] -- so that a gather that avoids the row, or a mask that holds the row's
    large elements out, loses the maximum (and every second digit).  -> (V, D, Rt, row)."""
    V, D, Rt = true_data(N, S, n_c, seed, base_max, rt_grid=rt_grid)
    D[row] = np.minimum(D[row], base_max)
    cols = np.arange(0, S, 3)
    D[row, cols] = top if top <= ONE_DIGIT_MAX else 128 + (cols * 977) % (top - 127)
    D[row, 0] = top
    X = D[row] // 3
    V[row] = np.where(D[row] > 0, X / np.where(D[row] > 0, D[row], 1), 0.5)
    assert D.max() == top and np.delete(D, row, axis=0).max() <= base_max < top
    return V, D, Rt, row


def avoiding(N, row, n_idx, seed):
    """A resample of n_idx rows of N that never draws `row`."""
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, N - 1, size=n_idx)
    return np.where(idx >= row, idx + 1, idx).astype(np.int64)


# (max count, what the created problem must be)
THRESHOLDS = [(127, 1), (128, 2), (32639, 2), (32640, 0)]
LOSE_MAX = [
    # name, top count of the planted row, X16 accepted?, digit count of the source, of a re-creation of the gathered rows
    ("one_digit_x16", 120, True, 1, 1), ("one_digit_v", 120, False, 1, 1), ("digit_lost_x16", 300, True, 2, 1),
]
