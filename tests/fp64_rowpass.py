"""The first-generation FP64 row kernels -- k_u_phase_mfma, k_rowpass_fused, k_u_phase_big, k_u_phase_gram, k_u_step_direct --
case by case: the tables of tests/test_gpu_fp64_rowpass.py, the launch plan of every case written down independently of the
library (expected_text: what dmf_u_phase_describe must answer), and the data and plain numpy references the cases run on.
A helper module like tests/gram_exact.py and tests/cost_exact.py: tests/test_fp64_rowpass_host.py proves without a GPU that
the tables reach every reachable template instance; the GPU file runs them.

Routes (dmf_select.hip).  The stand-alone u phase (Problem.update_u) never takes the one-launch row passes, so it lands on
  k_u_phase_mfma   levels 0, 3, 4, S <= 512, n_c <= 16, n_u <= 8 -- unless the integer producer k_cm_i8 takes the shape
                   (level 0, integer counts, n_u >= 5, alpha inside [0, 1]).  d16 instances: level 0 with integer counts
                   (n_u >= 5: a starting alpha with an entry above 1); the others: fractional counts, or level 3.
                   split mode: n_u >= 7, n_u >= 5 with known types, or more than 50 inner steps.
  k_u_phase_big    the same levels without integer copies, 9 <= n_u <= 26
  k_u_phase_gram   level 1, n_u <= 16
  k_u_step_direct  level 2
and the solver's loop takes k_rowpass_fused at level 4 (level 0 when the counts exceed 32639) up to 50 inner steps.
"""
from __future__ import annotations

import re
from collections import namedtuple

import numpy as np

from oracle import solver as osol

KAT = 1e-11      # one u phase of up to KAT_STEPS inner steps against the oracle's (tests/test_gpu_u_inner.py)
KAT_STEPS = 5
TIGHT = 1e-8     # the project's bar for longer runs (51 inner steps, whole outer iterations)
DEPTH = 40       # Poisson depth of the synthetic counts: below 128
SPLIT_STEPS = 51  # the first count past kSplitInnerSteps
LDS_STEPS = 6200  # a momentum table that pushes the dynamic LDS of k_u_phase_big past 48 KB

FORMS = ("scalar", "vec", "vec,d16")
MODES = ("one-launch", "split")

# kernel: mfma | big | gram | direct.  level: kernel selection level the problem and the solver are created at.
# ints: integer counts (level 0 then builds the u16 copy); False: counts + 0.5.  alpha_out: one alpha entry above 1.
# edges: zero-coverage rows / samples / stripes, alpha columns on vertices, u entries at 0 and 1, u_prev == u in half the rows.
UCase = namedtuple("UCase", "kernel N S n_c n_u n_iter2 level ints alpha_out edges why")


def ucase(kernel, N, S, n_c, n_u, n_iter2, level, ints=True, alpha_out=False, edges=False, why=""):
    return UCase(kernel, N, S, n_c, n_u, n_iter2, level, ints, alpha_out, edges, why)


def uid(c):
    return (f"{c.kernel}-N{c.N}-S{c.S}-{c.n_c}+{c.n_u}-t{c.n_iter2}-L{c.level}{'' if c.ints else '-frac'}"
            f"{'-aout' if c.alpha_out else ''}{'-edges' if c.edges else ''}")


def nd_of(c):
    """Count digit planes of the case's problem: integer counts below 128 at level 0 with 2..2048 samples."""
    return 1 if (c.ints and c.level == 0 and 2 <= c.S <= 2048) else 0


# ------------------------------------------------------------------------------------------------ plans, independently
def _tail(nw, grid, lds, blocks):
    return f"nw={nw} grid={grid} lds={lds} raise={int(lds > 48 * 1024)} blocks/wg={blocks}"


def mfma_natural_split(n_c, n_u, n_iter2):
    return n_iter2 > 50 or n_u >= 7 or (n_c > 0 and n_u >= 5)


def mfma_text(N, S, n_c, n_u, n_iter2, d16, split):
    nw = ((S + 15) // 16 + 3) // 4
    form = "scalar" if S % 4 else ("vec,d16" if d16 else "vec")
    grid = min((N + 15) // 16, 256 * (1 if nw >= 8 else 8 // nw))
    nv = n_u + n_u * (n_u + 1) // 2
    lds = ((0 if split else (n_iter2 + 1) & ~1) + 2 * nw * nv * 16) * 8
    return (f"k_u_phase_mfma<{(n_c + 3) // 4},{n_u},{form}> {'split' if split else 'one-launch'} "
            + _tail(nw, grid, lds, -(-((N + 15) // 16) // grid)))


def big_lds(S, n_c, n_u, n_iter2):
    gs = 16 if n_u <= 16 else 32
    np_ = n_u * (n_u + 1) // 2
    AS = (S + 15) // 16 * 16 + 2
    return 8 * (((n_iter2 + 1) & ~1) + (n_c + n_u) * AS + 16 * (gs + 1) + 16 * (np_ | 1) + 16 * gs)


def big_text(N, S, n_c, n_u, n_iter2):
    gs = 16 if n_u <= 16 else 32
    lds = big_lds(S, n_c, n_u, n_iter2)
    nblk = (N + 15) // 16
    grid = min(nblk, 256 * (2 if lds <= 78 * 1024 else 1))
    return f"k_u_phase_big<{(n_c + 3) // 4},{gs}> n_u={n_u} " + _tail(4 if gs == 16 else 8, grid, lds, -(-nblk // grid))


def gram_text(N, S, n_c, n_u):
    in_lds = (n_c + n_u) * S * 8 <= 36 * 1024
    return (f"k_u_phase_gram<{n_u}> alpha={'lds' if in_lds else 'global'} "
            + _tail(4, (N + 63) // 64, (n_c + n_u) * S * 8 if in_lds else 0, 1))


def direct_text(N, S, n_u, n_iter2):
    nb = (N + 3) // 4
    grid = min(nb, 4096)
    return f"k_u_step_direct n_u={n_u} nw=4 grid={grid} lds={4 * (S + 128) * 8} raise=0 blocks/wg={-(-nb // grid)} launches={n_iter2}"


TILE_BYTES = 16 * 66 * 8 + 16 * 68 * 4


def fused_grid(n_full, S):
    return min(n_full // 16, 256 * (2 if (S + 63) // 64 <= 2 else 1))


def fused_text(N, S, n_c, n_u, n_iter2):
    nw, nct = (S + 63) // 64, (n_c + 3) // 4 * 4
    nv = n_u + n_u * (n_u + 1) // 2
    doubles = ((n_iter2 + 1) & ~1) + 64 * n_u + 32 * max(nct, 1) + nw * nv * 16 + (nct + n_u + 1) * (nw * 64 + 2)
    lds = doubles * 8 + 2 * nw * TILE_BYTES
    n_full = N - N % 16
    grid = fused_grid(n_full, S)
    return f"k_rowpass_fused<{nct // 4},{n_u}> " + _tail(nw, grid, lds, -(-(n_full // 16) // grid)) + f" tail={N % 16}"


def expected_text(c):
    """What dmf_u_phase_describe must answer for the stand-alone u phase of a case."""
    if c.kernel == "mfma":
        return mfma_text(c.N, c.S, c.n_c, c.n_u, c.n_iter2, nd_of(c) > 0, mfma_natural_split(c.n_c, c.n_u, c.n_iter2))
    if c.kernel == "big":
        return big_text(c.N, c.S, c.n_c, c.n_u, c.n_iter2)
    if c.kernel == "gram":
        return gram_text(c.N, c.S, c.n_c, c.n_u)
    return direct_text(c.N, c.S, c.n_u, c.n_iter2)


INSTANCE_RE = [
    (re.compile(r"^k_u_phase_mfma<(\d),(\d),(scalar|vec|vec,d16)> (one-launch|split) "),
     lambda m: ("mfma", int(m[1]), int(m[2]), m[3], m[4])),
    (re.compile(r"^k_rowpass_fused<(\d),(\d)> nw=(\d) "), lambda m: ("fused", int(m[1]), int(m[2]), int(m[3]))),
    (re.compile(r"^k_u_phase_big<(\d),(\d+)> "), lambda m: ("big", int(m[1]), int(m[2]))),
    (re.compile(r"^k_u_phase_gram<(\d+)> alpha=(lds|global) "), lambda m: ("gram", int(m[1]), m[2])),
    (re.compile(r"^k_u_step_direct "), lambda m: ("direct",)),
]


def instance_of(text):
    """The template instance (with the run-time mode where the kernel has one) that a describe text names, or None for the
    second-generation kernels."""
    for rx, make in INSTANCE_RE:
        m = rx.match(text)
        if m:
            return make(m)
    return None


def field(text, name):
    return int(re.search(rf"(?:^| ){re.escape(name)}=(\d+)", text)[1])


def describe_flags(c):
    from demethify_amd import _lib as L

    return L.DMF_SELECT_ALPHA_OUTSIDE_UNIT if c.alpha_out else 0


def describe(c):
    """dmf_u_phase_describe for the stand-alone u phase of a case (None: DMF_ERR_UNSUPPORTED)."""
    from demethify_amd.device import u_phase_describe

    return u_phase_describe(c.N, c.S, c.n_c, c.n_u, nd_of(c), c.level, c.n_iter2, describe_flags(c), "update_u")


# ------------------------------------------------------------------------------------------------ stand-alone u phase: tables
ROWS = 2 * 16 + 16 + 5   # two full workgroups of one 16-row block, one more block, a ragged tail of 5


def _n_c_for(nkc, n_u):
    """A known-type count with ceil(n_c / 4) = nkc: 4 nkc, 4 nkc - 1, - 2, - 3 by n_u (1, 13 and 16 among them)."""
    return 0 if nkc == 0 else 4 * nkc - n_u % 4


def mfma_case(nkc, n_u, form, mode):
    """The smallest stand-alone case on k_u_phase_mfma<nkc, n_u, form> in `mode`, or None where no key reaches it."""
    n_c = _n_c_for(nkc, n_u)
    natural = mfma_natural_split(n_c, n_u, 3)
    if mode == "one-launch":
        if natural:
            return None
        n_iter2 = (1, 2, 5)[(nkc + n_u) % 3]
    else:
        n_iter2 = 3 if natural else SPLIT_STEPS
    if form == "vec,d16":  # level 0 on integer counts; from five unknowns on only a starting alpha outside [0, 1] leads here
        return ucase("mfma", ROWS, 8, n_c, n_u, n_iter2, 0, ints=True, alpha_out=n_u >= 5)
    S = 6 if form == "scalar" else 8
    if n_u % 2 == 0:
        return ucase("mfma", ROWS, S, n_c, n_u, n_iter2, 0, ints=False)   # fractional counts at level 0
    return ucase("mfma", ROWS, S, n_c, n_u, n_iter2, 3)                   # level 3: no integer copies


def mfma_instance_cases():
    return [c for nkc in range(5) for n_u in range(1, 9) for form in FORMS for mode in MODES
            for c in [mfma_case(nkc, n_u, form, mode)] if c is not None]


def mfma_unreachable():
    """(instance, rule) of every k_u_phase_mfma instance x mode that no key reaches: plan_iteration sends 7 and 8 unknowns,
    and 5 and 6 with known types, to the split form at every inner-step count."""
    out = []
    for nkc in range(5):
        for n_u in range(5, 9):
            if n_u >= 7 or nkc > 0:
                rule = "n_u >= kSplitMinNu: always split" if n_u >= 7 else "n_c > 0 and n_u >= 5: always split"
                out += [(("mfma", nkc, n_u, form, "one-launch"), rule) for form in FORMS]
    return out


def big_instance_cases():
    """k_u_phase_big<NKC 0..4, GS 16|32>: n_u at both ends of each group size under every NKC, every other n_u once."""
    out = []
    for n_u in range(9, 27):
        for nkc in range(5):
            if n_u in (9, 16, 17, 26) or nkc == n_u % 5:
                S = 6 if n_u % 3 == 0 else 8   # the kernel's scalar and vector loads
                if n_u % 2 == 0:
                    out.append(ucase("big", ROWS, S, _n_c_for(nkc, n_u), n_u, 3, 0, ints=False))
                else:
                    out.append(ucase("big", ROWS, S, _n_c_for(nkc, n_u), n_u, 3, 3))
    return out


GRAM_ROWS = 2 * 64 + 64 + 5   # k_u_phase_gram: 64 rows per workgroup


def gram_instance_cases():
    """k_u_phase_gram<NU 1..16>, alpha in LDS and -- beyond 36 KB of alpha -- read from global memory."""
    out = []
    for n_u in range(1, 17):
        n_c = (3 * n_u) % 5
        out.append(ucase("gram", GRAM_ROWS, 7, n_c, n_u, 3, 1))
        out.append(ucase("gram", 64 + 5, 4608 // (n_c + n_u) + 1, n_c, n_u, 3, 1, why="alpha beyond 36 KB: global"))
    return out


def direct_instance_cases():
    return [ucase("direct", 4 * 3 + 3, 7, n_c, n_u, 3, 2) for n_c, n_u in ((2, 1), (0, 3), (5, 17), (0, 64), (13, 51))]


def _representatives():
    """(kernel, S, n_c, n_u, level, ints, alpha_out, n_iter2 of the natural mode): each kernel, each mode of k_u_phase_mfma,
    NU and NKC at both ends of their ranges."""
    return [
        ("mfma", 6, 0, 1, 3, True, False),      # <0,1,scalar> one-launch
        ("mfma", 8, 16, 4, 0, True, False),     # <4,4,vec,d16> one-launch
        ("mfma", 8, 13, 8, 0, False, False),    # <4,8,vec> split
        ("mfma", 8, 0, 8, 0, True, True),       # <0,8,vec,d16> split (alpha outside [0, 1])
        ("big", 8, 0, 9, 3, True, False),       # <0,16>
        ("big", 6, 16, 26, 0, False, False),    # <4,32>
        ("gram", 7, 0, 1, 1, True, False),
        ("gram", 7, 13, 16, 1, True, False),
        ("direct", 7, 1, 2, 2, True, False),
        ("direct", 7, 0, 64, 2, True, False),
    ]


def row_edge_cases():
    return [ucase(k, N, S, n_c, n_u, 3, level, ints, aout, why="row edge")
            for k, S, n_c, n_u, level, ints, aout in _representatives() for N in (1, 15, 16, 17)]


def wrap_cases():
    """Workgroups that take 1, 2 and 3 row blocks in ONE launch: N = block rows x (2 grid cap + 1) + a ragged tail, the cap
    read off each launcher (256 x 8 / nw workgroups of k_u_phase_mfma, 512 or -- beyond 78 KB of LDS -- 256 of
    k_u_phase_big, 4096 of k_u_step_direct).  Reached by N alone."""
    w = "1, 2 and 3 blocks per workgroup"
    return [
        ucase("mfma", 16 * (2 * 2048 + 1) + 5, 8, 2, 3, 5, 0, ints=False, why=w),                  # nw = 1, one-launch, vec
        ucase("mfma", 16 * (2 * 2048 + 1) + 5, 6, 0, 1, 2, 3, why=w),                              # nw = 1, one-launch, scalar
        ucase("mfma", 16 * (2 * 2048 + 1) + 5, 8, 5, 4, 5, 0, why=w),                              # nw = 1, one-launch, d16
        ucase("mfma", 16 * (2 * 2048 + 1) + 5, 8, 3, 8, 3, 3, why=w),                              # nw = 1, split (level 3)
        ucase("mfma", 16 * (2 * 2048 + 1) + 5, 8, 0, 7, 3, 0, alpha_out=True, why=w),              # nw = 1, split, d16
        ucase("mfma", 16 * (2 * 1024 + 1) + 5, 68, 13, 2, 5, 3, why=w),                            # nw = 2, one-launch
        ucase("mfma", 16 * (2 * 512 + 1) + 5, 132, 4, 5, 3, 0, ints=False, why=w),                 # nw = 3 (grid 512), split
        ucase("mfma", 16 * (2 * 256 + 1) + 5, 452, 1, 3, 5, 0, why=w),                             # nw = 8, one-launch, d16
        ucase("mfma", 16 * (2 * 256 + 1) + 5, 449, 0, 7, 3, 3, why=w),                             # nw = 8, split, scalar
        ucase("big", 16 * (2 * 512 + 1) + 5, 8, 2, 9, 3, 3, why=w),                                # GS 16, two per CU
        ucase("big", 16 * (2 * 512 + 1) + 5, 6, 0, 17, 3, 0, ints=False, why=w),                   # GS 32, two per CU
        ucase("big", 16 * (2 * 256 + 1) + 5, 100, 16, 26, 3, 3, why=w + ", LDS beyond 78 KB: one per CU"),
        ucase("direct", 4 * (2 * 4096 + 1) + 3, 7, 2, 3, 2, 2, why=w),
    ]


SAMPLE_EDGES = (1, 3, 4, 15, 16, 17, 63, 64, 65)


def sample_edge_cases():
    out = []
    for S in SAMPLE_EDGES + (449, 512):
        out.append(ucase("mfma", ROWS, S, 5, 2, 5, 3, why="sample edge"))                        # one-launch
        out.append(ucase("mfma", ROWS, S, 0, 7, 3, 0, ints=False, why="sample edge"))            # split
    for S in (4, 16, 64, 452, 512):
        out.append(ucase("mfma", ROWS, S, 2, 3, 5, 0, why="sample edge, u16 counts"))            # d16 (S % 4 == 0)
    for S in SAMPLE_EDGES:
        out.append(ucase("big", ROWS, S, 3, 9, 3, 3, why="sample edge"))
        out.append(ucase("gram", 64 + 5, S, 2, 3, 3, 1, why="sample edge"))
        out.append(ucase("direct", 15, S, 2, 3, 3, 2, why="sample edge"))
    out.append(ucase("gram", 64 + 5, 1536, 1, 2, 3, 1, why="K S 8 = 36 KB exactly: alpha in LDS"))
    out.append(ucase("gram", 64 + 5, 1537, 1, 2, 3, 1, why="K S 8 just beyond 36 KB: alpha from global memory"))
    out.append(ucase("direct", 15, 1792, 1, 2, 2, 2, why="60 KB of dynamic LDS, the largest S the kernel takes"))
    return out


def inner_step_cases():
    out = []
    for k, S, n_c, n_u, level, ints, aout in _representatives():
        for n_iter2 in (0, 1, 2, 5):
            out.append(ucase(k, ROWS if k != "direct" else 15, S, n_c, n_u, n_iter2, level, ints, aout, why="inner steps"))
    # Dynamic LDS beyond 48 KB: the launcher raises the kernel's limit first.  k_u_phase_big gets there by its momentum
    # table; k_u_phase_mfma cannot (more than 50 inner steps always take the split mode, which keeps no table) and gets
    # there by the partial sums of eight waves, in both modes.
    out.append(ucase("big", ROWS, 8, 2, 9, LDS_STEPS, 3, why="momentum table beyond 48 KB"))
    out.append(ucase("mfma", ROWS, 452, 0, 6, 5, 3, why="one-launch, eight waves x 27 partial sums: 54 KB"))
    out.append(ucase("mfma", ROWS, 452, 2, 8, 3, 0, alpha_out=True, why="split, d16, eight waves x 44 partial sums: 88 KB"))
    return out


def data_edge_cases():
    out = [ucase(k, ROWS if k != "direct" else 15, S, n_c, n_u, 3, level, ints, aout, edges=True, why="data edges")
           for k, S, n_c, n_u, level, ints, aout in _representatives()]
    for n_c in (0, 1, 13, 16):   # (n_c not a multiple of 4: the padded R_trunc copy)
        out.append(ucase("mfma", ROWS, 8, n_c, 2, 3, 0, edges=True, why="data edges, d16"))
        out.append(ucase("big", ROWS, 8, n_c, 12, 3, 3, edges=True, why="data edges"))
    return out


def instance_cases():
    return mfma_instance_cases() + big_instance_cases() + gram_instance_cases() + direct_instance_cases()


def subset_cases():
    seen, out = set(), []
    for c in row_edge_cases() + wrap_cases() + sample_edge_cases() + inner_step_cases() + data_edge_cases():
        if c[:-1] not in seen:
            seen.add(c[:-1])
            out.append(c)
    return out


# ------------------------------------------------------------------------------------------------ stand-alone u phase: data
def update_u_inputs(c):
    """(V, D, Rt or None, u, u_prev, alpha, a1, l_w_prev, l_w): a NON-initial momentum state, alpha columns on the simplex
    (alpha_out: one entry above 1), every input valid and in bounds."""
    V, D, Rt = osol.synthetic_problem(c.N, c.S, max(c.n_c, 1), c.n_u, seed=41 + c.n_u + 3 * c.n_c, depth=DEPTH)
    assert D.max() <= 127
    D = D.astype(np.float64)
    if not c.ints:
        D = D + 0.5
    rs = np.random.RandomState(9)
    u, u_prev = rs.uniform(size=(c.N, c.n_u)), rs.uniform(size=(c.N, c.n_u))
    alpha = rs.dirichlet(np.ones(c.n_c + c.n_u), c.S).T.copy()
    if c.edges:
        D[min(3, c.N - 1), :] = 0.0            # a zero-coverage row,
        D[:, c.S // 2] = 0.0                   # sample
        D[::7, ::3] = 0.0                      # and stripes (what --fillna produces), V = 0 there
        V = np.where(D == 0, 0.0, V)
        alpha[:, 0] = 0.0
        alpha[c.n_c + c.n_u - 1, 0] = 1.0      # a column on a vertex of the simplex (an unknown type)
        if c.n_c and c.S > 1:
            alpha[:, 1] = 0.0
            alpha[0, 1] = 1.0                  # a column with zero unknown mass
        u[0::5, 0] = 0.0                       # entries at exactly 0 and 1
        u[1::5, -1] = 1.0
        u_prev[2::5, 0] = 1.0
        u_prev[3::5, -1] = 0.0
        u_prev[::2] = u[::2]                   # u_prev == u in every other row
    if c.alpha_out:
        alpha[0, 0] = 1.25
    l_w = np.linalg.norm(alpha[-c.n_u:]) ** 2 * float(D.max()) ** 2
    return V, D, (Rt if c.n_c else None), u, u_prev, alpha, 1.7, 0.9 * l_w, l_w


def update_u_oracle(c, unsup, V, D, Rt, u, u_prev, alpha, a1, l_w_prev, l_w):
    """deconvolution.py:81-90 (gradient at the extrapolated point) or, unsup, :157-164 (at the previous iterate), in numpy."""
    Rt = Rt if Rt is not None else np.zeros((c.N, 0))
    if not unsup:
        return osol.u_phase(u, alpha, c.n_iter2, a1, l_w_prev, l_w, u_prev, V, Rt, c.n_u, D)[:2]
    A_known, A_unk = alpha[:c.n_c], alpha[c.n_c:]
    base = V - Rt @ A_known
    for _ in range(c.n_iter2):
        a0 = a1
        a1, beta = osol.momentum_step(a0, l_w_prev, l_w)
        ut = u + beta * (u - u_prev)
        u_prev = u
        u = np.clip(ut + (D * (base - u @ A_unk)) @ A_unk.T / l_w, 0, 1)
        l_w_prev = l_w
    return u, u_prev


def tolerance(c):
    return KAT if c.n_iter2 <= KAT_STEPS else TIGHT


# ------------------------------------------------------------------------------------------------ fused row pass: tables
# level 4 -- or level 0 with every count scaled beyond 32639 (big) -- through the solver; T1 outer iterations
FCase = namedtuple("FCase", "N S n_c n_u n_iter2 T1 big why")


def fid(c):
    return f"N{c.N}-S{c.S}-{c.n_c}+{c.n_u}-t{c.n_iter2}-T{c.T1}{'-big' if c.big else ''}"


def fused_instance_cases():
    """All 20 instances at one column group and the smallest S; n_iter2 and the tail (N % 16 in {0, 5}) rotate."""
    out = []
    for nkc in range(5):
        for n_u in range(1, 5):
            i = nkc * 4 + n_u
            out.append(FCase(48 + (5 if i % 2 else 0), 4, _n_c_for(nkc, n_u), n_u, (1, 20, 50)[i % 3], 2, i % 7 == 0,
                             "instance at nw = 1"))
    return out


FUSED_WIDE = {2: 68, 3: 132, 4: 196}   # the smallest S of 2, 3 and 4 column groups


def fused_wide_cases():
    """nw = 2, 3, 4 on five instances each, NU and NKC at both ends."""
    out = []
    for nw, S in FUSED_WIDE.items():
        for i, (n_c, n_u) in enumerate(((0, 1), (0, 4), (16, 1), (13, 4), (6, 2))):
            out.append(FCase(48 + (5 if (i + nw) % 2 else 0), S, n_c, n_u, (20, 1, 50)[(i + nw) % 3], 2, False, f"nw = {nw}"))
    return out


def fused_wrap_cases():
    """Per nw a launch whose workgroups take 1, 2 and 3 blocks: 2 grid + 1 full blocks (grid = 512 up to two column
    groups, 256 beyond) -- the A team's prefetch, the s & 1 tile buffers, the C team flushing block s - 1 one step late."""
    w = "1, 2 and 3 blocks per workgroup"
    return [FCase(16 * (2 * 512 + 1) + 5, 8, 6, 2, 20, 2, False, w),
            FCase(16 * (2 * 512 + 1), 8, 0, 3, 1, 2, False, w),
            FCase(16 * (2 * 512 + 1) + 5, 68, 13, 4, 20, 2, False, w),
            FCase(16 * (2 * 256 + 1) + 5, 132, 0, 4, 50, 2, False, w),
            FCase(16 * (2 * 256 + 1), 196, 12, 4, 20, 2, False, w)]


def fused_small_cases():
    return [FCase(16, 8, 5, 2, 20, 2, False, "one block"), FCase(32, 8, 0, 2, 20, 2, False, "two blocks"),
            FCase(16, 8, 3, 1, 1, 2, True, "one block, level 0 with counts beyond 32639"),
            FCase(53, 8, 5, 3, 0, 2, False, "no inner step"), FCase(48, 68, 0, 2, 0, 2, False, "no inner step")]


def fused_cases():
    return fused_instance_cases() + fused_wide_cases() + fused_wrap_cases() + fused_small_cases()


def fused_describe(c):
    from demethify_amd import _lib as L
    from demethify_amd.device import u_phase_describe

    return u_phase_describe(c.N, c.S, c.n_c, c.n_u, 0, 0 if c.big else 4, c.n_iter2, L.DMF_SELECT_COUNTS_F32_EXACT, "solver")


def fused_inputs(c, seed=31):
    V, D, Rt = osol.synthetic_problem(c.N, c.S, max(c.n_c, 1), c.n_u, seed=seed, depth=DEPTH)
    D = D.astype(np.float64) * (1000.0 if c.big else 1.0)   # (big: beyond 32639, still exact in f32)
    return V, D, (Rt if c.n_c else None)


def solver_oracle(V, D, Rt, n_u, T1, n_iter2, seed=1):
    """(u0, a0, u, alpha) of T1 outer iterations: partial-reference with known types, else unsupervised."""
    if Rt is not None:
        u0, R, a0 = osol.init_partial("uniform_", V, D, Rt, n_u, seed=seed)
        wu, wa = osol.solve_partial(u0.copy(), R, a0.copy(), V, D, Rt, n_u, T1, n_iter2, 0.0,
                                    project=osol.simplex_project_columns_fast)
    else:
        u0, a0 = osol.init_unsupervised("uniform_", V, n_u, seed=seed)
        wu, wa = osol.solve_unsupervised(V, n_u, D, "uniform_", T1, n_iter2, 0.0, init=(u0.copy(), a0.copy()),
                                         project=osol.simplex_project_columns_fast)
    return u0, a0, wu, wa


# fused Gram: (family, N, S, n_c, n_u, nd, n_iter2) on the data of tests/gram_exact.py, level 4
GCase = namedtuple("GCase", "family N S n_c n_u nd n_iter2 why")
FUSED_GRAM = [
    GCase("dyadic", 48, 8, 6, 2, 1, 0, "whole blocks, one per workgroup, an even number of known types"),
    GCase("dyadic", 16 * 3 + 5, 8, 5, 3, 2, 0, "fused rows + the tail's slab rows, counts up to 8000, padded known types"),
    GCase("dyadic", 16 * (2 * 512 + 1) + 5, 8, 3, 2, 1, 0, "1, 2 and 3 blocks per workgroup + tail"),
    GCase("dyadic", 16 * (2 * 256 + 1), 132, 0, 1, 1, 0, "three column groups, 1, 2 and 3 blocks per workgroup"),
    GCase("full", 48, 8, 6, 2, 1, 2, "whole blocks, one per workgroup, an even number of known types"),
    GCase("full", 16 * 3 + 5, 68, 5, 3, 2, 2, "fused rows + the tail's slab rows, two column groups"),
    GCase("full", 16 * (2 * 512 + 1) + 5, 8, 3, 2, 1, 2, "1, 2 and 3 blocks per workgroup + tail"),
    GCase("full", 16 * 5 + 5, 196, 13, 4, 1, 2, "four column groups, the widest instance, tail"),
]


def gid(c):
    return f"{c.family}-N{c.N}-S{c.S}-{c.n_c}+{c.n_u}-nd{c.nd}-t{c.n_iter2}"
