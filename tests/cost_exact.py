"""Exact fixtures for the streaming cost cost_f_w = sum d (v - R alpha)^2 (deconvolution.py:15-17), and the case table that
reaches every instance of its kernel family (csrc/dmf_kernels_stream.hip).  A plain helper module: tests/test_cost_plan_host.py
checks it without a GPU, tests/test_gpu_cost_exact.py runs it.

Why the kernels must reproduce the integer bit for bit.  ``exact_case`` draws dyadic data: R = Ri / 16 (Ri in 0..16),
alpha = Ai / 64 (every column a composition of 64, so it lies on the simplex), V = Vi / 1024 (Vi in 0..1024), and integer
counts Di in 0..dmax (optionally divided by count_scale = 4).  Then, in float64, whatever the kernel and its order of sums:

  - every partial sum of fma(r, a, pred) is a multiple of 2^-10 and at most 1 (sum_k Ri Ai <= 16 * 64 = 1024), hence exact;
  - e = v - pred is a multiple of 2^-10 with |e| <= 1, hence exact;
  - d * e has at most 17 + 11 significant bits, hence exact;
  - fma(d * e, e, acc) and every later addition -- lanes, waves, workgroups, the final reduction -- add non-negative
    multiples of 2^-20 / count_scale whose total stays below 2^53 such units, hence exact.

So cost * 2^20 * count_scale = sum(Di * Ei^2) with Ei = Vi - Ri @ Ai, an integer that depends on the data alone.  A dropped,
duplicated or mis-weighted element changes bits where a tolerance would only lose digits.  The helper asserts the bound on
the total; it holds whenever N * S * dmax <= 2^33.

(oracle.solver.weighted_cost goes through sqrt(d) and does not always hit the integer: the exact tests compare with the
integer, never with that function.)
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import numpy as np

UNITS = 1 << 20          # 1 / (2^-10)^2
BOUND = 1 << 53
U16_MAX_COUNT = 32639    # largest count of the u16 / digit-plane copies (dmf_problem_create)

ExactCase = namedtuple("ExactCase", "V D Rt u alpha want Vi Di Ri Ai count_scale")


def _compositions(rs, K, S):
    """K x S integers >= 0, every column summing to 64."""
    cuts = np.sort(rs.randint(0, 65, size=(K - 1, S)), axis=0)
    edges = np.vstack([np.zeros((1, S), dtype=np.int64), cuts, np.full((1, S), 64, dtype=np.int64)])
    return np.diff(edges, axis=0).astype(np.int64)


def exact_sum(Di, Vi, Ri, Ai, weights=None):
    """sum(Di * Ei^2) (weights: an integer / bool array multiplied in) as a Python int; asserts the 2^53 bound."""
    Ei = Vi.astype(np.int64) - Ri.astype(np.int64) @ Ai.astype(np.int64)
    w = Di.astype(np.int64) if weights is None else Di.astype(np.int64) * np.asarray(weights).astype(np.int64)
    assert int(np.abs(Ei).max()) <= 1024 and int(w.min()) >= 0
    # (each term is below 2^36 and N * S below 2^27 in every case here: the int64 sum cannot wrap before the bound is checked)
    assert int(w.max()) * UNITS * Ei.size < (1 << 63)
    total = int(np.sum(w * Ei * Ei, dtype=np.int64))
    assert total == sum(int(x) for x in np.sum(w * Ei * Ei, axis=1, dtype=np.int64))
    assert total < BOUND, f"sum of {total} units does not stay below 2^53: float64 would round"
    return total


def exact_case(N, S, n_c, n_u, dmax, seed, count_scale=1):
    """-> ExactCase: float64 V, D (counts / count_scale), Rt (None without known types), u (None without unknown ones), alpha;
    `want` = cost * 2^20 * count_scale as a Python int; and the integer arrays behind them (Ri = [Rt | u] * 16)."""
    K = n_c + n_u
    assert K >= 1 and dmax >= 2 and count_scale in (1, 4)
    rs = np.random.RandomState(seed)
    Ri = rs.randint(0, 17, size=(N, K)).astype(np.int64)
    Ai = _compositions(rs, K, S)
    Vi = rs.randint(0, 1025, size=(N, S)).astype(np.int64)
    Di = rs.randint(1, dmax + 1, size=(N, S)).astype(np.int64)
    Di[rs.rand(N, S) < 0.1] = 0                      # about 10 % zeros
    Di[rs.randint(0, N), rs.randint(0, max(S - 1, 1))] = dmax  # dmax at least once (not in the last sample where S > 1)
    # the edges weigh something: the last row and the last sample are non-zero, and on odd S the last sample differs from
    # its neighbour (the lone lane of k_cost_cols2 fetches both)
    Di[N - 1][Di[N - 1] == 0] = 1 + (seed % dmax)
    Di[:, S - 1][Di[:, S - 1] == 0] = dmax - (seed % dmax)
    if S > 1:
        same = Di[:, S - 1] == Di[:, S - 2]
        Di[same, S - 1] = Di[same, S - 1] % dmax + 1
    assert Di.max() == dmax and Di.min() >= 0 and (Di[N - 1] > 0).all() and (Di[:, S - 1] > 0).all()
    assert S == 1 or (Di[:, S - 1] != Di[:, S - 2]).all()
    want = exact_sum(Di, Vi, Ri, Ai)
    R = Ri / 16.0
    Rt = np.ascontiguousarray(R[:, :n_c]) if n_c else None
    u = np.ascontiguousarray(R[:, n_c:]) if n_u else None
    D = Di if count_scale == 1 else Di / float(count_scale)
    return ExactCase(Vi / 1024.0, D, Rt, u, Ai / 64.0, want, Vi, Di, Ri, Ai, count_scale)


# ------------------------------------------------------------------------------------------------ the plan, from Python
CostCase = namedtuple("CostCase", "N S n_c n_u dmax count_scale level seed expect")


def has_u16(case):
    """dmf_problem_create builds the u16 copy of the counts at level 0, for integer counts up to 32639, 2 <= S <= 2048 and
    n_c <= 48 (R_trunc of exact_case lies inside [0, 1])."""
    return (case.level == 0 and case.count_scale == 1 and case.dmax <= U16_MAX_COUNT and 2 <= case.S <= 2048
            and case.n_c <= 48)


def pure_describe(lib, S, n_c, n_u, u16, level, v_align=0, SD=None, rtp=None):
    """dmf_cost_describe for a key; SD and rtp_present default to what dmf_problem_create makes of the shape."""
    buf = ctypes.create_string_buffer(128)
    if SD is None:
        SD = (S + 63) // 64 * 64 if u16 else 0
    if rtp is None:
        rtp = 1 <= n_c <= 48
    st = lib.dmf_cost_describe(S, n_c, n_u, int(u16), SD, v_align, int(rtp), level, buf, len(buf))
    assert st == 0, (st, S, n_c, n_u, u16, level)
    return buf.value.decode()


def describe_case(lib, case, level=None):
    """The pure describe function on the key a problem of this case has (at `level` instead of the level it was created at)."""
    return pure_describe(lib, case.S, case.n_c, case.n_u, has_u16(case), case.level if level is None else level)


def expected_describe(S, n_c, n_u, u16, level, SD=None, v_align=0, rtp=None):
    """The rules of the cost plan (csrc/dmf_kernels_stream.hip: cost_plan), written down independently."""
    K = n_c + n_u
    if SD is None:
        SD = (S + 63) // 64 * 64 if u16 else 0
    if rtp is None:
        rtp = 1 <= n_c <= 48
    nkc = (n_c + 3) // 4
    rtp_ok = n_c == 0 or rtp
    pair_ok = u16 and SD % 2 == 0 and v_align % 8 == 0 and (S + 127) // 128 <= 1024
    parity = "odd" if S % 2 else "even"
    if level in (0, 3, 4) and rtp_ok and n_c <= 16 and n_u <= 4:
        if pair_ok and S >= 128:
            return f"cost=k_cost_cols2<{nkc},{n_u},{parity}>"
        if (S + 63) // 64 <= 1024:
            return f"cost=k_cost_cols<{nkc},{n_u},{'u16' if u16 else 'f64'}>"
    elif level == 0 and rtp_ok and n_c <= 16 and 5 <= n_u <= 16 and pair_ok and S >= 32:
        return f"cost=k_cost_cols2<{nkc},{n_u},{parity}>"
    return "cost=k_cost alpha=" + ("lds" if K * S * 8 <= 48 * 1024 else "global")


def all_column_instances():
    """The describe strings of the 48 + 48 + 120 column-resident instances."""
    cols = {f"cost=k_cost_cols<{a},{b},{t}>" for a in range(5) for b in range(5) if a + b for t in ("u16", "f64")}
    narrow = {f"cost=k_cost_cols2<{a},{b},{p}>" for a in range(5) for b in range(5) if a + b for p in ("odd", "even")}
    wide = {f"cost=k_cost_cols2<{a},{b},{p}>" for a in range(5) for b in range(5, 17) for p in ("odd", "even")}
    assert len(cols) == 48 and len(narrow) == 48 and len(wide) == 120
    return cols | narrow | wide


ROWS = (1, 3, 31, 33, 67)  # fewer rows than waves, fewer than one 8-row sweep, a clamped tail
S_COLS_U16 = (2, 7, 63, 64, 65, 127)
S_COLS_F64 = (1, 5, 64, 65, 129, 200)
S_NARROW = {"even": (128, 130, 256), "odd": (129, 191, 255, 257)}  # (257: the third block's lone lane is alone in it)
S_WIDE = {"even": (32, 64, 128, 130, 256), "odd": (33, 127, 129, 191, 255, 257)}


def instance_cases():
    """One CostCase per instance of the column-resident kernels -- every (NKC, NU) of k_cost_cols on u16 and on f64 counts,
    every (NKC, NU) of k_cost_cols2 with both parities of S -- at the smallest shapes that reach the edges: n_c alternates
    between 4 NKC (borrowed R_trunc) and 4 NKC - 1 (padded copy), N and S rotate through ROWS and the S_* lists, u16 cases
    alternate one and two digit planes, f64 cases alternate among a count of 40000, fractional counts and level 4."""
    cases, used = [], {}

    def add(nkc, nu, S_list, expect, f64=False):
        i = len(cases)
        j = used[S_list] = used.get(S_list, -1) + 1     # the j-th case of this list: S walks it, the rest shifts per lap
        a, lap = j % len(S_list), j // len(S_list)
        n_c = 0 if nkc == 0 else 4 * nkc - (a + lap) % 2
        N, S = ROWS[i % len(ROWS)], S_list[a]
        if f64:
            dmax, scale, level = ((40000, 1, 0), (127, 4, 0), (127, 1, 4))[(a + lap) % 3]
        else:
            dmax, scale, level = (127, 32639)[(j // 2 + lap) % 2], 1, 0
        cases.append(CostCase(N, S, n_c, nu, dmax, scale, level, 1000 + i, expect))

    for nkc in range(5):
        for nu in range(5):
            if nkc + nu == 0:
                continue
            add(nkc, nu, S_COLS_U16, f"cost=k_cost_cols<{nkc},{nu},u16>")
            add(nkc, nu, S_COLS_F64, f"cost=k_cost_cols<{nkc},{nu},f64>", f64=True)
            for parity in ("even", "odd"):
                add(nkc, nu, S_NARROW[parity], f"cost=k_cost_cols2<{nkc},{nu},{parity}>")
        for nu in range(5, 17):
            for parity in ("even", "odd"):
                add(nkc, nu, S_WIDE[parity], f"cost=k_cost_cols2<{nkc},{nu},{parity}>")
    return cases


LDS, GLOBAL = "cost=k_cost alpha=lds", "cost=k_cost alpha=global"


def generic_cases():
    """k_cost: alpha in LDS with S below a wave and S = 1, S > 256 (threads loop over samples), alpha from global memory
    (K S 8 > 48 KiB), and n_u beyond the wide form.  All at level 0 but (50, 1, 2, 1): a problem of one sample with two known
    types and one unknown belongs to k_cost_cols<1,1,f64> there, so that shape reaches k_cost at level 1."""
    shapes = [(40, 20, 1, 5, 0, LDS), (50, 1, 2, 1, 1, LDS), (33, 300, 17, 1, 0, LDS), (20, 260, 26, 4, 0, GLOBAL),
              (64, 40, 0, 17, 0, LDS)]
    return [CostCase(N, S, n_c, n_u, (127, 32639)[i % 2], 1, level, 2000 + i, e)
            for i, (N, S, n_c, n_u, level, e) in enumerate(shapes)]


def grid_cap_cases():
    """The row loop takes a second trip: more than 1024 / ny row blocks of 32 rows."""
    shapes = [(32805, 3, 2, 1, "cost=k_cost_cols<1,1,u16>"), (32805, 128, 0, 2, "cost=k_cost_cols2<0,2,even>"),
              (2100, 2047, 12, 4, "cost=k_cost_cols2<3,4,odd>")]
    return [CostCase(N, S, n_c, n_u, 127, 1, 0, 3000 + i, e) for i, (N, S, n_c, n_u, e) in enumerate(shapes)]


WIDE_S_CASE = CostCase(3, 65600, 1, 1, 127, 1, 0, 4000, GLOBAL)  # ceil(S / 64) partial columns do not fit the scratch
