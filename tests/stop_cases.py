"""The stop test |cf - cf_0| < tol (deconvolution.py:218-220) on every kernel path of the solver's loop: the table of cases
that tests/test_gpu_stop_paths.py runs, with everything they need from the numpy oracle.  A helper module like
tests/fp64_rowpass.py: tests/test_stop_cases_host.py proves without a GPU that the table reaches every RowKind, GramKind and
AlphaKind of dmf_select.h and that every case's stop is a clear one.

The run-ahead contract under test.  dmf_solver_step enqueues 8 outer iterations, then 16, 32, 64, and reads the state back
between the batches only; it is right only if every kernel of an outer iteration does nothing once state->done is set
(1: stopped; 2: paused inside the confirmation band of 10 tol until the host has decided on streaming costs).  Each case
whose solver runs ahead (runs_ahead: all but the two whose fall-back u path is k_u_step_direct, where the loop looks at
the state after every iteration) therefore stops at an iteration k that has at least two enqueued iterations behind it,
and -- with the confirmation forced -- pauses for the first time at an iteration that has launches behind it too.

Per case, from the oracle's cost trace cf_0 (before the loop), cf_1 .. cf_24 at tol = 0, with d_j = |cf_j - cf_{j-1}|:
  k        a stop iteration the trajectory can reach: d_k < min_{j<k} d_j
  tol      sqrt(d_k min_{j<k} d_j), the geometric middle of the gap the threshold has to fall into
  margin   min(|d_k - tol|, |min_{j<k} d_j - tol|) / tol
  pauses   the iterations j <= k with d_j < 10 tol, and which of them dmf_solver_step decides on two streaming costs
           (n_confirmed: the iteration before paused too, or was the starting point, whose cost is a streaming cost) and
           which on the Gram form (n_unconfirmed) -- pause_model, written from the loop of dmf_solver_step.
"""
from __future__ import annotations

import functools
import re
from collections import namedtuple
from pathlib import Path

import numpy as np

from oracle import solver as osol

FAST = osol.simplex_project_columns_fast
TRACE = 24           # outer iterations traced, and what the GPU legs ask step() for: one batch of 8 and one of 16
BAND = 10.0          # kConfirmBand of dmf_api_solver.hip
MARGIN = 1e-2        # smallest stop margin, and smallest relative distance of any d_j from the band's edge
DEPTH = 40           # Poisson depth of the counts: below 128, one count digit
TIGHT = 1e-8         # max-abs bar of u and alpha against the oracle (tests/test_gpu_small_batch.py: hold)
COST_RTOL = 1e-9     # relative bar of the Gram-form cost
GAP = 1e-9           # purity: smallest relative gap of a Frank-Wolfe vertex decision (tests/test_gpu_purity.py)
FIRST_BATCH, SECOND_BATCH = range(2, 7), range(9, 23)   # stops with at least two enqueued iterations behind them

V2, V2X = "k_rowpass_v2", "k_rowpass_v2 x16"
CM_BU, CM_ROWS = "k_cm_i8+k_inner_bu", "k_cm_i8+k_u_inner_rows"
SPLIT, MFMA, BIG, UGRAM, DIRECT, FUSED = ("k_u_phase_mfma(split)+k_u_inner_rows", "k_u_phase_mfma", "k_u_phase_big",
                                          "k_u_phase_gram", "k_u_step_direct", "k_rowpass_fused")
I8, BU_I8, GU, GMFMA, GRAM, INROW = "k_gram_i8", "k_bu_cols+k_gram_i8", "k_gram_u", "k_gram_mfma", "k_gram", "fused"
ROW16, LANES, PHASE, DYN = "k_alpha_phase_row16", "k_alpha_phase_lanes", "k_alpha_phase", "k_alpha_phase_dyn"
FW16, FW = "k_alpha_frank_wolfe_row16", "k_alpha_frank_wolfe"

# what describe prints for each enumerator of dmf_select.h (describe_row / describe_plan)
ROW_TEXT = {"RowpassV2": (V2, V2X), "CmI8InnerBu": (CM_BU,), "CmI8InnerRows": (CM_ROWS,), "RowpassFused": (FUSED,),
            "UPhaseBig": (BIG,), "UPhaseMfmaSplit": (SPLIT,), "UPhaseMfma": (MFMA,), "UPhaseGram": (UGRAM,),
            "UStepDirect": (DIRECT,)}
GRAM_TEXT = {"InRowPass": INROW, "I8": I8, "BuColsI8": BU_I8, "GramU": GU, "GramMfma": GMFMA, "Gram": GRAM}
ALPHA_TEXT = {"FrankWolfeRow16": FW16, "FrankWolfe": FW, "PhaseRow16": ROW16, "PhaseLanes": LANES, "Phase": PHASE,
              "PhaseDyn": DYN}

# level: dmf_context_set_generic.  ints: integer counts (False: counts + 0.5).  purity: the Frank-Wolfe alpha phase.
# x16: the context's X16 switch (matters at level 0).  masked: the solver runs on Problem.masked(mask).
# seed / init: of synthetic_problem and of the starting point.  k: the stop iteration (a reachable one of the trace).
# row, gram, alpha: what Solver.describe(n_iter2) must name (template arguments left out); extra: further tokens.
StopCase = namedtuple("StopCase", "name N S n_c n_u n_iter2 level ints purity x16 masked seed init k row gram alpha extra")


def case(name, N, S, n_c, n_u, n_iter2, level, seed, init, k, row, gram, alpha, ints=True, purity=False, x16=True,
         masked=False, extra=()):
    return StopCase(name, N, S, n_c, n_u, n_iter2, level, ints, purity, x16, masked, seed, init, k, row, gram, alpha, extra)


ROWS = 2 * 16 + 16 + 5   # tests/fp64_rowpass.py: two workgroups of one 16-row block, one more block, a ragged tail of 5

# name, N, S, n_c, n_u, n_iter2, level, seed, init, k, row, gram, alpha.  Seeds and k come from a search over the oracle's
# traces (seeds 3.., starting points 1..4) for a reachable k inside a batch with a margin well above MARGIN; they are not
# tuned on anything a GPU returned.
CASES = [
    case("01-v2-x16", ROWS, 8, 4, 2, 5, 0, 3, 2, 9, V2X, I8, ROW16),                      # the control
    case("02-v2-v", ROWS, 6, 3, 1, 5, 0, 3, 1, 6, V2, I8, ROW16, x16=False),              # the row pass's V form
    case("03-cm-bu-row16", ROWS, 8, 7, 5, 3, 0, 3, 1, 12, CM_BU, I8, ROW16),              # wide row group, K = 12
    case("04-cm-bu-lanes", 200, 64, 12, 6, 20, 0, 3, 1, 3, CM_BU, I8, LANES),             # K = 18
    case("05-cm-rows-wide", 96, 16, 3, 17, 5, 0, 3, 2, 9, CM_ROWS, BU_I8, LANES),         # n_u > 16: no k_inner_bu -- and no
    #                                     run-ahead: the fall-back u path of 17 unknowns is k_u_step_direct (runs_ahead below)
    case("06-fused-tail", ROWS, 8, 4, 2, 5, 4, 4, 3, 6, FUSED, INROW, ROW16, extra=("tail=5",)),  # + k_u_phase_mfma,
    #                                                          launch_sumsq_f64, k_gram_u and k_finish_u_norm on the tail's 5 rows
    case("07-mfma", ROWS, 8, 0, 3, 5, 3, 4, 2, 9, MFMA, GU, ROW16),                       # unsupervised, first pause at 1, next at 6
    case("08-split-51", ROWS, 8, 4, 2, 51, 3, 3, 1, 4, SPLIT, GU, ROW16, ints=False),     # fractional counts
    case("09-split-51-ints", ROWS, 8, 12, 4, 51, 0, 3, 3, 9, SPLIT, BU_I8, ROW16),        # level 0 beyond kSplitInnerSteps
    case("10-big", 96, 16, 3, 12, 5, 3, 3, 4, 9, BIG, GMFMA, ROW16),                      # K = 15
    case("11-gram-phase", 69, 7, 2, 3, 5, 1, 3, 2, 16, UGRAM, GRAM, PHASE),               # pauses at 1, then from 5 on
    case("12-gram-dyn", 128, 100, 12, 6, 20, 1, 3, 1, 3, UGRAM, GRAM, DYN),               # K = 18 at level 1
    case("13-direct", 15, 7, 2, 3, 3, 2, 3, 3, 14, DIRECT, GRAM, PHASE),                  # check_every is 1 here: any k >= 2
    case("14-purity-row16", ROWS, 8, 4, 2, 5, 0, 3, 3, 14, V2X, I8, FW16, purity=True),   # first pause at 6
    case("15-purity-general", ROWS, 8, 16, 1, 5, 3, 3, 2, 6, MFMA, GU, FW, purity=True),  # K = 17
    case("16-masked", ROWS, 8, 4, 2, 5, 0, 4, 3, 6, V2X, I8, ROW16, masked=True),         # the hold-out weights path
    case("17-cm-rows-257", ROWS, 257, 7, 5, 3, 0, 3, 2, 15, CM_ROWS, BU_I8, ROW16),       # beyond k_inner_bu's 256 samples: the
    #                                     k_u_inner_rows route WITH run-ahead; two panels (256 + 1 samples) of k_cm_i8
]

IDS = [c.name for c in CASES]
assert len(set(IDS)) == len(IDS)


def runs_ahead(c):
    """Whether dmf_solver_step enqueues batches of 8, 16, .. iterations for the case, or reads the state after every one.
    It is the solver's FALL-BACK u path that decides (select_path: u_path; check_every is 1 when that is k_u_step_direct),
    also where the loop never launches it: k_u_phase_mfma's shapes at levels 0, 3, 4, else k_u_phase_gram's up to 16
    unknowns below level 2, else k_u_step_direct."""
    if c.level in (0, 3, 4) and c.n_u <= 8 and c.n_c <= 16 and c.S <= 512:
        return True
    return c.level != 2 and c.n_u <= 16


# ------------------------------------------------------------------------------------------------ data and oracle
def nd_of(c):
    """Count digit planes of the case's problem (tests/fp64_rowpass.py): integer counts below 128 at level 0."""
    return 1 if (c.ints and c.level == 0 and 2 <= c.S <= 2048) else 0


def purity_of(c):
    """Per-sample mass of the known block: uniform in (0.05, 0.95) with an exact 0 and an exact 1 planted."""
    p = np.random.RandomState(c.seed + 11).uniform(0.05, 0.95, c.S)
    p[c.S // 2], p[c.S - 1] = 0.0, 1.0
    return p


def mask_of(c):
    """The training mask of a masked case: about one element in eight held out, one row and one sample kept whole."""
    m = np.random.RandomState(c.seed + 5).uniform(size=(c.N, c.S)) >= 0.125
    m[0, :] = True
    m[:, 0] = True
    return m


Inputs = namedtuple("Inputs", "V D Rt purity mask u0 a0 Vo Do")   # Vo, Do: what the oracle solves on (masked: V, D x mask)


@functools.lru_cache(maxsize=None)
def inputs(c):
    V, D, Rt = osol.synthetic_problem(c.N, c.S, max(c.n_c, 1), c.n_u, seed=c.seed, depth=DEPTH)
    assert D.max() <= 127
    D = D.astype(np.float64) + (0.0 if c.ints else 0.5)
    purity = purity_of(c) if c.purity else None
    if c.n_c == 0:
        Rt = None
        u0, a0 = osol.init_unsupervised("uniform_", V, c.n_u, seed=c.init)
    elif c.purity:
        u0, _, a0 = osol.init_partial_purity("uniform_", V, D, Rt, c.n_u, purity, seed=c.init)
    else:
        u0, _, a0 = osol.init_partial("uniform_", V, D, Rt, c.n_u, seed=c.init)
    mask = mask_of(c) if c.masked else None
    Vo, Do = (V * mask, D * mask) if c.masked else (V, D)
    for a in (V, D, Rt, purity, mask, u0, a0, Vo, Do):
        if a is not None:
            a.setflags(write=False)
    return Inputs(V, D, Rt, purity, mask, u0, a0, Vo, Do)


def oracle_run(c, n_iter1, tol):
    """(u, alpha, cost before the loop, cost trace, smallest Frank-Wolfe gap or inf) of the numpy oracle from the case's
    starting point: up to n_iter1 outer iterations, stopping where |cf - cf_0| < tol."""
    i = inputs(c)
    trace, gaps = [], []
    if c.n_c == 0:
        start = osol.weighted_cost(i.Vo, i.u0, i.a0, i.Do)
        u, alpha = osol.solve_unsupervised(i.Vo, c.n_u, i.Do, "uniform_", n_iter1, c.n_iter2, tol,
                                           init=(i.u0.copy(), i.a0.copy()), project=FAST, trace=trace)
        return u, alpha, start, trace, np.inf
    R = np.c_[i.Rt, i.u0]
    start = osol.weighted_cost(i.Vo, R, i.a0, i.Do)
    if c.purity:
        u, alpha = osol.solve_partial_purity(i.u0.copy(), R, i.a0.copy(), i.Vo, i.Do, i.Rt, c.n_u, i.purity, n_iter1, c.n_iter2,
                                             tol, trace=trace, gaps=gaps)
        return u, alpha, start, trace, min(gaps)
    u, alpha = osol.solve_partial(i.u0.copy(), R, i.a0.copy(), i.Vo, i.Do, i.Rt, c.n_u, n_iter1, c.n_iter2, tol, project=FAST,
                                  trace=trace)
    return u, alpha, start, trace, np.inf


def differences(start, trace):
    """d[j] = |cf_j - cf_{j-1}|, j = 1 .. len(trace); d[0] is inf (nothing stops before the loop)."""
    cf = np.r_[start, trace]
    return np.r_[np.inf, np.abs(np.diff(cf))]


def threshold(d, k):
    """(tol, margin) of a stop at iteration k of a trajectory with differences d."""
    lo, hi = d[k], d[1:k].min()
    tol = float(np.sqrt(lo * hi))
    return tol, float(min(abs(lo - tol), abs(hi - tol)) / tol)


def reachable(d):
    """[(k, tol, margin)] of every iteration k >= 2 the stop test can fire at first: d_k < min_{j<k} d_j."""
    return [(k,) + threshold(d, k) for k in range(2, len(d)) if d[k] < d[1:k].min()]


def pause_model(d, k, tol):
    """(pauses, n_confirmed, n_unconfirmed) of step(n, n_iter2, tol) on a fresh solver with the confirmation forced.
    The closing kernel sets done = 2 at every iteration whose difference is inside the band; the host then decides on the
    streaming costs of this and the previous iterate where it holds the previous one (that iteration paused too, or is the
    starting point: its cost, asked for before the loop, is a streaming cost), else on the Gram form -- and the decision
    is to stop exactly when d_j < tol, which first holds at k."""
    pauses = [j for j in range(1, k + 1) if d[j] < BAND * tol]
    known = 0   # the iteration whose streaming cost the host holds (cf_stream_iter): the starting point
    confirmed = unconfirmed = 0
    for j in pauses:
        if known == j - 1:
            confirmed += 1
        else:
            unconfirmed += 1
        known = j
    return pauses, confirmed, unconfirmed


def band_clearance(d, k, tol):
    """Smallest relative distance of d_1 .. d_k from the band's edge 10 tol."""
    return float(np.abs(d[1:k + 1] / (BAND * tol) - 1.0).min())


Analysis = namedtuple("Analysis", "d k tol margin clearance pauses n_confirmed n_unconfirmed u alpha cost stop gap cf_max")


@functools.lru_cache(maxsize=None)
def analyse(c):
    """Everything the tests need from the oracle for one case; the arrays are read-only and shared."""
    _, _, start, trace, gap = oracle_run(c, TRACE, 0.0)
    d = differences(start, trace)
    tol, margin = threshold(d, c.k)
    pauses, confirmed, unconfirmed = pause_model(d, c.k, tol)
    u, alpha, _, stopped, gap_k = oracle_run(c, TRACE, tol)   # the oracle's own stop under this threshold
    u.setflags(write=False)
    alpha.setflags(write=False)
    d.setflags(write=False)
    return Analysis(d, c.k, tol, margin, band_clearance(d, c.k, tol), pauses, confirmed, unconfirmed, u, alpha, stopped[-1],
                    len(stopped), min(gap, gap_k), float(max(start, max(trace))))


# ------------------------------------------------------------------------------------------------ selection, without a GPU
def select_flags(c):
    from demethify_amd import _lib as L

    flags = L.DMF_SELECT_COUNTS_F32_EXACT | L.DMF_SELECT_COUNTS_BYTE   # (counts below 128, fractional ones k + 0.5)
    if c.purity:
        flags |= L.DMF_SELECT_PURITY
    if c.x16 and nd_of(c):
        flags |= L.DMF_SELECT_X16
    return flags


def kinds(desc):
    """(row pass, Gram kernel, alpha kernel) of a describe string, without template arguments; the row pass's X16 form
    keeps its " x16"."""
    row, gram, alpha = re.fullmatch(r"rowpass=(.*) gram=(\S+) alpha=(\S+)", desc).groups()
    kind = re.sub(r"<[^>]*>", "", row).split(" ")[0]
    if kind == V2 and row.endswith(" x16"):
        kind = V2X
    return kind, re.sub(r"<[^>]*>", "", gram).replace("/w8", ""), alpha


def select_describe(c):
    """dmf_select_describe of the case's key: what Solver.describe(n_iter2) will say."""
    import ctypes as C

    from demethify_amd import _lib as L

    buf = C.create_string_buffer(512)
    st = L.load().dmf_select_describe(c.N, c.S, c.n_c, c.n_u, nd_of(c), c.level, c.n_iter2, select_flags(c), buf, len(buf))
    return buf.value.decode() if st == L.DMF_OK else None


def u_phase_text(c):
    """dmf_u_phase_describe of the case's key on the solver's route."""
    from demethify_amd.device import u_phase_describe

    return u_phase_describe(c.N, c.S, c.n_c, c.n_u, nd_of(c), c.level, c.n_iter2, select_flags(c), "solver")


def enumerators(name):
    """The enumerator names of `enum class <name>` as dmf_select.h lists them."""
    text = (Path(__file__).resolve().parent.parent / "demethify_amd" / "csrc" / "dmf_select.h").read_text()
    body = re.search(rf"enum class {name}\s*\{{(.*?)\}};", text, re.S)[1]
    body = re.sub(r"//[^\n]*", "", body)
    return [e.strip() for e in body.split(",") if e.strip()]
