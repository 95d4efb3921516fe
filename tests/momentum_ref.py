"""The momentum coefficient beta = min((a_prev - 1) / a_next, 0.9999 sqrt(l_prev / l_cur)) (deconvolution.py:83-85, :95-97)
and the alpha phase, case by case: the tables of tests/test_gpu_momentum.py, the data they run on and plain numpy references
in any precision.  A helper module like tests/fp64_rowpass.py and tests/gram_exact.py: tests/test_momentum_host.py proves
without a GPU that the tables reach every alpha kernel instance and branch and that the cap really decides the result of
every case that claims it; the GPU file runs them.

Scalar states (a, l_prev / l) for either phase:
  QUIET  3.1, 1.1   the ratio stays below the cap (the state of tests/test_gpu_kat.py)
  SQRT   40,  0.5   0.9999 sqrt(0.5) = 0.707 < 39 / 40.5: the cap decides the first step only (l_prev = l behind it)
  FLAT   3e4, 1.0   0.9999 < (3e4 - 1) / (3e4 + 0.5) = 0.99995: the cap decides every step
The ratio is below 1 and the flat cap is 0.9999, so under FLAT the two are never more than 1e-4 apart: FLAT_GAP below is what
a = 3e4 leaves, eleven orders above the rounding of either side.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from oracle import solver as osol

LD = np.longdouble
EPS = 2.0 ** -53
STATES = {"QUIET": (3.1, 1.1), "SQRT": (40.0, 0.5), "FLAT": (3e4, 1.0)}
STATE_NAMES = ("QUIET", "SQRT", "FLAT")
CAP_EFFECT = 1e-6   # what dropping the cap must change in the extended-precision reference of a case that claims it
CAP_GAP = 1e-3      # relative distance between the two arguments of the min wherever the cap decides ...
FLAT_GAP = 4e-5     # ... and under FLAT, where 1e-4 is the most there can be (see above): 5e-5 at a = 3e4, less 20 %
MARGIN = 16.0       # bar = MARGIN * max(noise of the float64 references, steps * 2^-53)
KAT, TIGHT = 1e-11, 1e-8


def tri(k, l):
    return l * (l + 1) // 2 + k


# ------------------------------------------------------------------------------------------------ references
def momentum(a, l_prev, l_cur, cap=True):
    """(a_next, beta, ratio, cap value) in the precision of the arguments (numpy scalars of one dtype)."""
    t = type(a)
    a_next = (1 + np.sqrt(1 + 4 * a * a)) / 2
    ratio = (a - 1) / a_next
    capv = t(0.9999) * np.sqrt(l_prev / l_cur)
    return a_next, (min(ratio, capv) if cap else ratio), ratio, capv


def all_steps(a, l_prev, l_cur, n_iter2):
    """[(step, ratio, cap value)] of the inner steps of one phase (float64 scalars)."""
    out = []
    a, l_prev, l_cur = np.float64(a), np.float64(l_prev), np.float64(l_cur)
    for t in range(n_iter2):
        a, _, ratio, capv = momentum(a, l_prev, l_cur)
        out.append((t, float(ratio), float(capv)))
        l_prev = l_cur
    return out


def cap_steps(a, l_prev, l_cur, n_iter2):
    """all_steps at which the cap decides beta."""
    return [(t, ratio, capv) for t, ratio, capv in all_steps(a, l_prev, l_cur, n_iter2) if ratio > capv]


def project(X):
    """deconvolution.py:25-35, sort-based, every column at once, in X's dtype."""
    p, n = X.shape
    srt = -np.sort(-X, axis=0)
    shifted = np.cumsum(srt, axis=0) - 1
    ranks = np.arange(1, p + 1).astype(X.dtype)[:, None]
    ok = (srt - shifted / ranks) > 0
    rho = np.where(ok.any(axis=0), p - 1 - np.argmax(ok[::-1], axis=0), -1)
    theta = shifted[rho, np.arange(n)] / (rho + 1).astype(X.dtype)
    return np.maximum(X - theta[None, :], 0)


def unpack(gb, K, dtype):
    """(G (K, K, S) symmetric, b (K, S), vDv (S)) of a packed Gram buffer."""
    gb = np.asarray(gb).astype(dtype)
    G = np.empty((K, K, gb.shape[1]), dtype=dtype)
    for l in range(K):
        for k in range(l + 1):
            G[k, l] = G[l, k] = gb[tri(k, l)]
    return G, gb[[tri(k, K) for k in range(K)]], gb[tri(K, K)]


def alpha_phase_ref(gb, alpha, alpha_prev, a2, l_h_prev, l_h, n_iter2, dtype, cap=True):
    """deconvolution.py:93-102 from the packed Gram, x = at + (b - G at) / l_h, everything -- the momentum recurrence
    too -- in `dtype` -> (alpha, alpha_prev).  cap=False drops the min: for preconditions only."""
    K = alpha.shape[0]
    G, b, _ = unpack(gb, K, dtype)
    a, ap = np.asarray(alpha).astype(dtype), np.asarray(alpha_prev).astype(dtype)
    a2, lp, l = dtype(a2), dtype(l_h_prev), dtype(l_h)
    for _ in range(n_iter2):
        a2, beta, _, _ = momentum(a2, lp, l, cap)
        at = a + beta * (a - ap)
        ap = a
        a = project(at + (b - (G * at[None, :, :]).sum(axis=1)) / l)
        lp = l
    return a, ap


def gram_ref(V, D, Rt, u, dtype):
    """The packed Gram ((K + 1)(K + 2) / 2, S) of X = [R_trunc | u | v_s] with weights d_s, from the data, in `dtype`."""
    V, D = np.asarray(V).astype(dtype), np.asarray(D).astype(dtype)
    R = np.c_[Rt, u].astype(dtype) if Rt is not None else np.asarray(u).astype(dtype)
    K, S = R.shape[1], V.shape[1]
    gb = np.empty(((K + 1) * (K + 2) // 2, S), dtype=dtype)
    for l in range(K):
        blk = R[:, :l + 1].T @ (D * R[:, l:l + 1])
        for k in range(l + 1):
            gb[tri(k, l)] = blk[k]
    DV = D * V
    blk = R.T @ DV
    for k in range(K):
        gb[tri(k, K)] = blk[k]
    gb[tri(K, K)] = (DV * V).sum(axis=0)
    return gb


def cost_ref(gb, alpha):
    """(cost, magnitude): the Gram-form cost sum_s vDv - 2 a.b + a^T G a in np.longdouble, and the sum of the absolute
    values of its terms, sum_s vDv + 2 sum_k a_k |b_k| + sum_kl a_k a_l |G_kl|, that the error bound is a multiple of."""
    K = alpha.shape[0]
    G, b, vdv = unpack(gb, K, LD)
    a = np.asarray(alpha).astype(LD)
    lin, quad = (a * b).sum(axis=0), (a[:, None, :] * a[None, :, :] * G).sum(axis=(0, 1))
    mag = vdv + 2 * (a * np.abs(b)).sum(axis=0) + (a[:, None, :] * a[None, :, :] * np.abs(G)).sum(axis=(0, 1))
    return float((vdv - 2 * lin + quad).sum()), float(mag.sum())


def cost_factor(K, S):
    """The multiple of 2^-53 x magnitude that bounds |cf - cost_ref|.  Per sample the kernels form G a and a.b as fma
    chains of K terms (error at most K units each, relative to the absolute sum), the quadratic form adds one product and
    the 16-lane sum (1 + 4), cost - 2 lin + quad three more roundings: K + 8 covers the sample.  The samples are then
    summed over the wave (6 steps), the workgroup partials in a strided loop (ceil(nb / 64) <= 2 terms here) and a last wave
    sum (6): 14.  The Gram entries themselves are the GPU's own (read back), so they contribute nothing."""
    return K + 8 + 14


# ------------------------------------------------------------------------------------------------ Leg A: one alpha phase
# kernel: the instance, level: kernel selection level; edges: the edge data set
ACase = namedtuple("ACase", "kernel level N S n_c n_u n_iter2 state edges")
ROW16_K = (1, 2, 3, 4, 5, 8, 9, 12, 13, 16)
ROW16_S = (1, 2, 3, 5, 300)   # every S % 4 (one to three live columns of four), 75 workgroups
LANES_K = {"k_alpha_phase_lanes<32>": (17, 24, 32), "k_alpha_phase_lanes<64>": (33, 48, 64)}
LANES_S = {"k_alpha_phase_lanes<32>": (1, 5), "k_alpha_phase_lanes<64>": (1, 3)}
PHASE_K = (1, 2, 4, 5, 8, 9, 12, 13, 16)
PHASE_S = (3, 64, 65, 130)
DYN_K = (17, 33, 64)
DYN_S = (3, 66)
STEPS = (1, 4, 20)
KERNEL_STEPS = (0, 2, 64, 65, 500)
KERNELS = ("k_alpha_phase_row16", "k_alpha_phase_lanes<32>", "k_alpha_phase_lanes<64>", "k_alpha_phase<4>", "k_alpha_phase<8>",
           "k_alpha_phase<16>", "k_alpha_phase_dyn")


def kernel_of(K, level):
    """The alpha kernel instance of K types at a level (dmf_select.hip; launch_alpha picks the template argument)."""
    if level in (1, 2):
        return "k_alpha_phase_dyn" if K > 16 else f"k_alpha_phase<{4 if K <= 4 else 8 if K <= 8 else 16}>"
    return "k_alpha_phase_row16" if K <= 16 else f"k_alpha_phase_lanes<{32 if K <= 32 else 64}>"


def described_as(kernel):
    """What dmf_select_describe prints behind alpha= for an instance: the kernel's name without template arguments."""
    return kernel.split("<")[0]


def branch_of(K):
    """The side of every K > 2 / 4 / 8 / 12 branch (sort, scan, product of k_alpha_phase_row16) that K is on."""
    return (K > 2) + (K > 4) + (K > 8) + (K > 12)


def _rows(K):
    return 120 if K <= 16 else 64


def _grid(level, Ks, Ss):
    """Every K with every (n_c, S), the scalar states and the step counts cycled so that each K sees all of both."""
    out = []
    for K in Ks:
        combos = [(n_c, S) for n_c in sorted({0, K // 2}) for S in Ss]
        if len(combos) < 3:
            combos = combos * 2
        for i, (n_c, S) in enumerate(combos):
            out.append(ACase(kernel_of(K, level), level, _rows(K), S, n_c, K - n_c, STEPS[(i + i // 3) % 3],
                             STATE_NAMES[i % 3], False))
    return out


def _smallest(kernel):
    """(level, K, S) of the extra cases of a kernel: its largest K, a sample count of at most 5."""
    return {"k_alpha_phase_row16": (0, 16, 5), "k_alpha_phase_lanes<32>": (0, 32, 5), "k_alpha_phase_lanes<64>": (0, 64, 3),
            "k_alpha_phase<4>": (1, 3, 5), "k_alpha_phase<8>": (1, 7, 5), "k_alpha_phase<16>": (1, 13, 5),
            "k_alpha_phase_dyn": (1, 33, 3)}[kernel]


def grid_cases():
    out = _grid(0, ROW16_K, ROW16_S)
    for name in LANES_K:
        out += _grid(0, LANES_K[name], LANES_S[name])
    return out + _grid(1, PHASE_K, PHASE_S) + _grid(1, DYN_K, DYN_S)


def step_cases():
    out = []
    for j, kernel in enumerate(KERNELS):
        level, K, S = _smallest(kernel)
        for i, n in enumerate(KERNEL_STEPS):
            out.append(ACase(kernel, level, _rows(K), S, K // 2 if i % 2 else 0, K - (K // 2 if i % 2 else 0), n,
                             STATE_NAMES[(i + j) % 3], False))
    return out


def edge_cases():
    out = []
    for j, kernel in enumerate(KERNELS):
        level, K, S = _smallest(kernel)
        out.append(ACase(kernel, level, _rows(K), 5 if level == 0 else 65, K // 2, K - K // 2, 4, STATE_NAMES[1 + j % 2], True))
    return out


def alpha_cases():
    return grid_cases() + step_cases() + edge_cases()


def aid(c):
    return (f"{c.kernel}-L{c.level}-N{c.N}-S{c.S}-{c.n_c}+{c.n_u}-t{c.n_iter2}-{c.state}{'-edges' if c.edges else ''}")


def select_describe(N, S, n_c, n_u, level, n_iter2, nd=1, x16=True):
    """dmf_select_describe of a shape on integer counts below 128 that are exact x / d (None: unsupported)."""
    import ctypes as C

    from demethify_amd import _lib as L

    buf = C.create_string_buffer(512)
    flags = L.DMF_SELECT_COUNTS_F32_EXACT | (L.DMF_SELECT_X16 if x16 and nd else 0)
    st = L.load().dmf_select_describe(N, S, n_c, n_u, nd if (level == 0 and 2 <= S <= 2048) else 0, level, n_iter2, flags, buf,
                                      len(buf))
    if st == L.DMF_ERR_UNSUPPORTED:
        return None
    L.check(st, "dmf_select_describe")
    return buf.value.decode()


@functools.lru_cache(maxsize=8)
def alpha_inputs(c):
    """(V, D, Rt or None, u, alpha, alpha_prev, a2, l_h_prev, l_h) of a Leg A case, read-only."""
    K = c.n_c + c.n_u
    V, D, Rt = osol.synthetic_problem(c.N, c.S, max(c.n_c, 1), c.n_u, seed=7 + K + 3 * c.S, depth=20)
    rs = np.random.RandomState(200 + K + 5 * c.S)
    u = rs.uniform(size=(c.N, c.n_u))
    alpha = rs.dirichlet(np.ones(K), c.S).T.copy()
    # (half way to another point of the simplex: the extrapolated point then mostly stays inside it, where beta matters)
    alpha_prev = 0.5 * alpha + 0.5 * rs.dirichlet(np.ones(K), c.S).T
    if c.edges:
        D = D.copy()
        D[:, 0] = 0                              # a zero-coverage sample: G = 0 and b = 0
        V = np.where(D == 0, 0.0, V)
        alpha[:, 1] = 0.0
        alpha[K - 1, 1] = 1.0                    # a column on a vertex
        alpha[:, 2] = 1.0 / K
        alpha_prev[:, 2] = 1.0 / K               # a column at 1 / K throughout, alpha_prev equal to it
        alpha_prev[:, 3::2] = alpha[:, 3::2]     # alpha_prev == alpha in half the columns
    R = np.c_[Rt, u] if c.n_c else u
    l_h = np.linalg.norm(R) ** 2 * float(D.max()) ** 2
    a2, f = STATES[c.state]
    out = (V, D, (Rt if c.n_c else None), u, alpha, alpha_prev, a2, f * l_h, l_h)
    for x in out:
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=8)
def alpha_refs(c):
    """(ref alpha, ref alpha_prev, bar, noise, gb in longdouble): the np.longdouble reference of a Leg A case and its bar,
    MARGIN * max(noise, steps * 2^-53), noise = the larger deviation from it of the same phase in float64 on the float64
    Gram and of oracle.solver.alpha_phase -- measured on the references alone."""
    V, D, Rt, u, alpha, alpha_prev, a2, lhp, lh = alpha_inputs(c)
    gb = gram_ref(V, D, Rt, u, LD)
    ref = alpha_phase_ref(gb, alpha, alpha_prev, a2, lhp, lh, c.n_iter2, LD)
    f64 = alpha_phase_ref(gram_ref(V, D, Rt, u, np.float64), alpha, alpha_prev, a2, lhp, lh, c.n_iter2, np.float64)
    R = np.c_[Rt, u] if Rt is not None else u
    orc = osol.alpha_phase(c.n_iter2, alpha, a2, lhp, lh, alpha_prev, R, D, V, project=osol.simplex_project_columns_fast)
    noise = max(float(np.abs(x - r).max()) for x, r in ((f64[0], ref[0]), (f64[1], ref[1]), (orc[0], ref[0]), (orc[1], ref[1])))
    return ref[0], ref[1], alpha_bar(noise, c.n_iter2), noise, gb


def alpha_bar(noise, n_iter2):
    return MARGIN * max(noise, max(1, n_iter2) * EPS)


def phase_noise(gb, alpha, alpha_prev, a2, lhp, lh, n_iter2, ref):
    """The noise of one alpha phase from a given Gram: the float64 run against the longdouble `ref` (Leg C)."""
    f64 = alpha_phase_ref(np.asarray(gb, dtype=np.float64), alpha, alpha_prev, a2, lhp, lh, n_iter2, np.float64)
    return max(float(np.abs(f64[0] - ref[0]).max()), float(np.abs(f64[1] - ref[1]).max()))


# ------------------------------------------------------------------------------------------------ Leg B: one u phase
UCAP_STEPS = 5


def u_cases():
    """(name, fp64_rowpass.UCase) per stand-alone route, the smallest shapes of tests/fp64_rowpass.py and
    tests/test_gpu_u_inner.py at 5 inner steps; `name` is what the u phase must describe as."""
    import fp64_rowpass as fr

    n = UCAP_STEPS
    return [
        ("k_u_phase_mfma<1,3,vec> one-launch", fr.ucase("mfma", fr.ROWS, 8, 2, 3, n, 3)),
        ("k_u_phase_mfma<0,7,vec> split", fr.ucase("mfma", fr.ROWS, 8, 0, 7, n, 0, ints=False)),
        ("k_u_phase_mfma<1,3,vec,d16> one-launch", fr.ucase("mfma", fr.ROWS, 8, 2, 3, n, 0)),
        ("k_u_phase_big<1,16>", fr.ucase("big", fr.ROWS, 8, 3, 9, n, 3)),
        ("k_u_phase_gram<3>", fr.ucase("gram", fr.GRAM_ROWS, 7, 2, 3, n, 1)),
        ("k_u_step_direct", fr.ucase("direct", 15, 7, 2, 3, n, 2)),
        ("k_cm_i8<nd=1>+k_u_inner_rows", fr.ucase("cm", 2 * 16 + 9, 8, 2, 5, n, 0)),
        ("k_cm_i8<nd=1>+k_u_inner_rows", fr.ucase("cm", 2 * 16 + 9, 8, 0, 12, n, 0)),
        ("k_cm_i8<nd=1>+k_u_inner_rows", fr.ucase("cm", 2 * 8 + 5, 8, 2, 20, n, 0)),
    ]


def u_state(l_w, state):
    a1, f = STATES[state]
    return a1, f * l_w, l_w


def u_phase_nocap(c, unsup, V, D, Rt, u, u_prev, alpha, a1, l_w_prev, l_w, cap=True):
    """fp64_rowpass.update_u_oracle's loops with the cap optional (float64): for the cap-effect precondition."""
    Rt = Rt if Rt is not None else np.zeros((c.N, 0))
    A_known, A_unk = alpha[:c.n_c], alpha[c.n_c:]
    base = V - Rt @ A_known
    a1, l_w_prev, l_w = np.float64(a1), np.float64(l_w_prev), np.float64(l_w)
    for _ in range(c.n_iter2):
        a1, beta, _, _ = momentum(a1, l_w_prev, l_w, cap)
        ut = u + beta * (u - u_prev)
        u_prev = u
        u = np.clip(ut + (D * (base - (u_prev if unsup else ut) @ A_unk)) @ A_unk.T / l_w, 0, 1)
        l_w_prev = l_w
    return u, u_prev


# ------------------------------------------------------------------------------------------------ Legs C, D: cold start
A1_MASS = 1e-4   # one inner step per iteration: the ratio stays below 0.53 for four iterations, l_w has to grow faster
# row / alpha: what the path must describe as; x16: problems carry the u16 read counts; mass: what the unknown block of
# alpha0 is rescaled to (None: alpha0 as drawn -- "the u0 scaling alone"); u_cap / alpha_cap: the caps the case claims
CCase = namedtuple("CCase", "name level N S n_c n_u n_iter2 x16 row alpha mass u_cap alpha_cap")
T1 = 4
ROW16 = "k_alpha_phase_row16"


def _cold(name, level, N, S, n_c, n_u, n_iter2, row, alpha, x16=True, mass=0.02):
    """A case with the unknown block at `mass` (claims the u cap; without known types alpha0 stays as drawn and only the
    alpha cap engages)."""
    return CCase(name, level, N, S, n_c, n_u, n_iter2, x16, row, alpha, mass if n_c else None, n_c > 0, n_c == 0)


def _alpha_start(c):
    """The same path from alpha0 as drawn: claims the alpha cap."""
    return c._replace(name=c.name + "-alpha", mass=None, u_cap=False, alpha_cap=True)


COLD = [
    _cold("a1", 0, 200, 8, 2, 4, 1, "k_rowpass_v2<1,4>", ROW16, mass=A1_MASS),
    _cold("a20", 0, 200, 8, 2, 4, 20, "k_rowpass_v2<1,4>", ROW16),
    _cold("a50", 0, 200, 8, 2, 4, 50, "k_rowpass_v2<1,4>", ROW16),
    _cold("b", 0, 300, 70, 6, 2, 7, "k_rowpass_v2<2,2>", ROW16, x16=False),
    _cold("c", 0, 120, 8, 16, 2, 20, "k_rowpass_v2<4,2>", "k_alpha_phase_lanes"),
    _cold("d", 0, 200, 8, 2, 4, 51, "k_u_phase_mfma(split)+k_u_inner_rows", ROW16),
    _cold("e", 0, 150, 8, 2, 6, 20, "k_cm_i8<nd=1>+k_inner_bu", ROW16),
    _cold("f", 0, 200, 8, 0, 4, 20, "k_rowpass_v2<0,4>", ROW16),
    _cold("g", 4, 200, 8, 2, 4, 20, "k_rowpass_fused<1,4>", ROW16),
    _cold("h", 3, 200, 8, 2, 4, 20, "k_u_phase_mfma", ROW16),
    _cold("i", 1, 200, 8, 2, 4, 20, "k_u_phase_gram", "k_alpha_phase"),
    _cold("j", 2, 100, 6, 14, 3, 7, "k_u_step_direct", "k_alpha_phase_dyn"),
]
# known types dominate l_h where they outnumber the unknown ones (b, c, j): those paths claim the u cap alone, and their
# alpha kernels see the cap in Leg A
COLD += [_alpha_start(c) for c in COLD if c.name in ("a20", "e", "g", "h", "i")]
LEG_D = COLD[1]._replace(name="rows")   # the smallest shape of case (a)
LEG_D_TRAIL = (20, 20, 51, 20, 20)      # step(2, 20), step(1, 51), step(2, 20): the momentum rows on, off and on again


def uses_rows(c, n_iter2):
    """Whether dmf_solver_step uploads momentum rows for the case: k_rowpass_v2 (which takes 1..50 inner steps) together
    with k_alpha_phase_row16."""
    return c.row.startswith("k_rowpass_v2") and c.alpha == ROW16 and 1 <= n_iter2 <= 50


def cid(c):
    return f"{c.name}-L{c.level}-N{c.N}-S{c.S}-{c.n_c}+{c.n_u}-t{c.n_iter2}"


@functools.lru_cache(maxsize=4)
def cold_inputs(c):
    """(V, D, Rt or None, u0, alpha0): u0 = 0.05 uniform, alpha0 = Dirichlet columns rescaled so that the unknown block
    carries mass c.mass (None: unchanged)."""
    V, D, Rt = osol.synthetic_problem(c.N, c.S, max(c.n_c, 1), c.n_u, seed=17 + c.n_u, depth=20)
    rs = np.random.RandomState(23)
    u0 = 0.05 * rs.uniform(size=(c.N, c.n_u))
    a0 = rs.dirichlet(np.ones(c.n_c + c.n_u), c.S).T.copy()
    if c.mass is not None:
        a0[:c.n_c] *= (1.0 - c.mass) / a0[:c.n_c].sum(axis=0)
        a0[c.n_c:] *= c.mass / a0[c.n_c:].sum(axis=0)
    out = (V, D, (Rt if c.n_c else None), u0, a0)
    for x in out:
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return out


def u_phase_oracle(c, u, u_prev, alpha, a1, l_w_prev, l_w, V, D, Rt, n_iter2=None, cap=True):
    """One u phase of a cold-start case in float64: oracle.solver.u_phase with known types, else the unsupervised inline
    loop (gradient at the previous iterate, deconvolution.py:163).  cap=False: preconditions only."""
    import fp64_rowpass as fr

    n = c.n_iter2 if n_iter2 is None else n_iter2
    k = fr.ucase("cold", c.N, c.S, c.n_c, c.n_u, n, c.level)
    if cap and c.n_c:
        return osol.u_phase(u, alpha, n, a1, l_w_prev, l_w, u_prev, V, Rt, c.n_u, D)[:2]
    return u_phase_nocap(k, c.n_c == 0, V, D, Rt, u, u_prev, alpha, a1, l_w_prev, l_w, cap)


@functools.lru_cache(maxsize=4)
def cold_trajectory(c, n_steps=None):
    """The oracle's trajectory from the cold start, T1 outer iterations (or the inner-step counts `n_steps`, one per
    iteration) -> (list of per-iteration dicts, u, alpha).  Each dict: u_cap / alpha_cap = cap_steps of the phase, u_all /
    alpha_all = all_steps of it,
    u_effect / alpha_effect = what dropping the cap from that phase alone changes in its result."""
    V, D, Rt, u, alpha = cold_inputs(c)
    Rt0 = Rt if Rt is not None else np.zeros((c.N, 0))
    d = float(D.max()) ** 2
    a1 = a2 = 1.0
    u_prev, alpha_prev = u, alpha
    l_w = np.linalg.norm(alpha[-c.n_u:]) ** 2 * d
    l_h = np.linalg.norm(np.c_[Rt0, u]) ** 2 * d
    l_w_prev, l_h_prev = l_w, l_h
    out = []
    for n in (n_steps or (c.n_iter2,) * T1):
        rec = {"u_cap": cap_steps(a1, l_w_prev, l_w, n), "u_all": all_steps(a1, l_w_prev, l_w, n)}
        nu, nup = u_phase_oracle(c, u, u_prev, alpha, a1, l_w_prev, l_w, V, D, Rt, n)
        if rec["u_cap"]:
            rec["u_effect"] = float(np.abs(u_phase_oracle(c, u, u_prev, alpha, a1, l_w_prev, l_w, V, D, Rt, n, cap=False)[0] - nu).max())
        u, u_prev = nu, nup
        for _ in range(n):
            a1 = (1 + np.sqrt(1 + 4 * a1 * a1)) / 2
        if n:
            l_w_prev = l_w
        R = np.c_[Rt0, u]
        l_h = np.linalg.norm(R) ** 2 * d
        rec["alpha_cap"], rec["alpha_all"] = cap_steps(a2, l_h_prev, l_h, n), all_steps(a2, l_h_prev, l_h, n)
        if rec["alpha_cap"]:
            gb = gram_ref(V, D, Rt, u, LD)
            w = alpha_phase_ref(gb, alpha, alpha_prev, a2, l_h_prev, l_h, n, LD)[0]
            wo = alpha_phase_ref(gb, alpha, alpha_prev, a2, l_h_prev, l_h, n, LD, cap=False)[0]
            rec["alpha_effect"] = float(np.abs(w - wo).max())
        alpha, alpha_prev, a2, _ = osol.alpha_phase(n, alpha, a2, l_h_prev, l_h, alpha_prev, R, D, V,
                                                    project=osol.simplex_project_columns_fast)
        if n:
            l_h_prev = l_h
        l_w = np.linalg.norm(alpha[-c.n_u:]) ** 2 * d
        out.append(rec)
    return out, u, alpha


def cap_iterations(c, n_steps=None):
    """(iterations whose u phase runs under the cap, iterations whose alpha phase does), counted from 1, on the oracle's
    trajectory: what tests/test_gpu_momentum.py asserts of the scalars it reads back."""
    traj = cold_trajectory(c, n_steps)[0]
    return ([i + 1 for i, r in enumerate(traj) if r["u_cap"]], [i + 1 for i, r in enumerate(traj) if r["alpha_cap"]])
