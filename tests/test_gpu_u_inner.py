"""Every instance of the split u phase's consumers against the oracle: k_u_inner_rows at 1..32 unknowns -- one kernel body
with three lane layouts (dmf_ustep.h: row groups of 1..4 lanes, one row per DPP row at 5..16, two DPP rows per row at
17..32) -- and k_inner_bu at 1..16 unknowns x {one, two 128-sample groups} x {even, odd S}.

The shapes are the smallest that fill two workgroups (or chunks), one more wave and one more row, so the whole file takes
seconds.  test_every_instance_is_in_the_matrix (no GPU) holds the case lists to the instances they claim."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

from oracle import solver as osol

from conftest import rel_err

TIGHT = 1e-8
KAT = 1e-11  # one u phase through dmf_update_u against the oracle's (test_update_u_known_answer_on_cm_i8)

SPLIT = "k_u_phase_mfma(split)+k_u_inner_rows"
CM_ROWS, CM_BU = "k_cm_i8<nd=1>+k_u_inner_rows", "k_cm_i8<nd=1>+k_inner_bu"
S_SMALL, DEPTH = 8, 40  # counts stay below 128: one digit plane
SPLIT_STEPS = 51        # the first count past kSplitInnerSteps
BETA_CHUNK = 6144       # kBetaChunk: momentum coefficients held in LDS at a time

Case = namedtuple("Case", "n_u N S n_c n_iter2 unsup")


def _quad_rows(n_u):
    r = 4 * (64 // n_u)  # rows per workgroup: two full workgroups, one full wave and one row of the next
    return 2 * r + 64 // n_u + 1


# row groups (1..4 unknowns), through the solver: partial-reference and unsupervised (gradient at the previous iterate)
QUAD = [Case(n_u, _quad_rows(n_u), S_SMALL, n_c, SPLIT_STEPS, n_c == 0) for n_u in range(1, 5) for n_c in (2, 0)]
# one row per DPP row (5..16) and per two DPP rows (17..32), through the stand-alone u phase
DPP = [Case(n_u, 2 * 16 + 9 if n_u <= 16 else 2 * 8 + 5, S_SMALL, n_c, 3, unsup)
       for n_u in range(5, 33) for n_c, unsup in ((0, False), (2, False), (0, True))]
# the momentum table in two chunks, once per layout, through the solver
CHUNKED = [Case(n_u, 48, 6, 3, BETA_CHUNK + 1, False) for n_u in (2, 5, 17)]
# k_inner_bu: two chunks (16 rows with one 128-sample group, 32 with two) + 3 rows; the second group of S = 130 / 131 holds
# one lane (+ the lone sample).  Up to four unknowns only more than 16 known types lead here.
INNER_BU = [Case(n_u, 2 * (16 if S <= 128 else 32) + 3, S, 17 if n_u <= 4 else 0, 20, n_u > 4)
            for n_u in range(1, 17) for S in (6, 7, 130, 131)]


def _id(c):
    return f"nu{c.n_u}-N{c.N}-S{c.S}-nc{c.n_c}-t{c.n_iter2}{'-unsup' if c.unsup else ''}"


def _problem(c, seed):
    V, D, Rt = osol.synthetic_problem(c.N, c.S, max(c.n_c, 1), c.n_u, seed=seed, depth=DEPTH)
    assert D.max() <= 127
    return V, D, (Rt if c.n_c else None)


def solver_inputs(c):
    """(V, D, Rt or None, u0, a0) of a case that runs through the solver"""
    V, D, Rt = _problem(c, 61 + c.n_u)
    if c.n_c:
        u0, _, a0 = osol.init_partial("uniform_", V, D, Rt, c.n_u, seed=5)
    else:
        u0, a0 = osol.init_unsupervised("uniform_", V, c.n_u, seed=5)
    return V, D, Rt, u0, a0


def solver_oracle(c, V, D, Rt, u0, a0, T1=1):
    if c.n_c:
        return osol.solve_partial(u0.copy(), np.c_[Rt, u0], a0.copy(), V, D, Rt, c.n_u, T1, c.n_iter2, 0.0,
                                  project=osol.simplex_project_columns_fast)
    return osol.solve_unsupervised(V, c.n_u, D, "uniform_", T1, c.n_iter2, 0.0, init=(u0.copy(), a0.copy()),
                                   project=osol.simplex_project_columns_fast)


def solver_run(ctx, c, V, D, Rt, u0, a0, expect, T1=1):
    """(u, alpha) after T1 outer iterations at level 0, on the path `expect` names"""
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    mode = L.DMF_MODE_UNSUPERVISED if c.unsup else L.DMF_MODE_PARTIAL
    with Problem(ctx, V, D, Rt) as p, Solver(p, u0, a0, mode) as s:
        path = s.describe(c.n_iter2)
        assert f"rowpass={expect} " in path, path
        it, _ = s.step(T1, c.n_iter2, 0.0)
        assert it == T1
        u, alpha, _, _ = s.get()
    return u, alpha


def update_u_inputs(c):
    """(V, D, Rt or None, u, u_prev, alpha, a1, l_w_prev, l_w): a NON-initial momentum state, alpha on the simplex"""
    V, D, Rt = _problem(c, 41 + c.n_u)
    rs = np.random.RandomState(9)
    u, u_prev = rs.uniform(size=(c.N, c.n_u)), rs.uniform(size=(c.N, c.n_u))
    alpha = rs.dirichlet(np.ones(c.n_c + c.n_u), c.S).T
    l_w = np.linalg.norm(alpha[-c.n_u:]) ** 2 * float(D.max()) ** 2
    return V, D, Rt, u, u_prev, alpha, 1.7, 0.9 * l_w, l_w


def update_u_oracle(c, V, D, Rt, u, u_prev, alpha, a1, l_w_prev, l_w):
    if not c.unsup:
        Rt = Rt if Rt is not None else np.zeros((c.N, 0))
        return osol.u_phase(u, alpha, c.n_iter2, a1, l_w_prev, l_w, u_prev, V, Rt, c.n_u, D)[:2]
    for _ in range(c.n_iter2):  # deconvolution.py:157-164: the unsupervised loop takes the gradient at the previous iterate
        a0 = a1
        a1, beta = osol.momentum_step(a0, l_w_prev, l_w)
        ut = u + beta * (u - u_prev)
        u_prev = u
        u = np.clip(ut + (D * (V - u @ alpha)) @ alpha.T / l_w, 0, 1)
        l_w_prev = l_w
    return u, u_prev


def update_u_run(ctx, c, V, D, Rt, u, u_prev, alpha, a1, l_w_prev, l_w):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem

    with Problem(ctx, V, D, Rt) as p:
        return p.update_u(u, u_prev, alpha, c.n_iter2, a1, l_w_prev, l_w,
                          mode=L.DMF_MODE_UNSUPERVISED if c.unsup else L.DMF_MODE_PARTIAL)[:2]


# ----------------------------------------------------------------------------------------- no GPU
def _describe(c):
    from demethify_amd import _lib as L

    buf = C.create_string_buffer(512)
    flags = L.DMF_SELECT_COUNTS_F32_EXACT | L.DMF_SELECT_X16
    assert L.load().dmf_select_describe(c.N, c.S, c.n_c, c.n_u, 1, 0, c.n_iter2, flags, buf, len(buf)) == L.DMF_OK
    return buf.value.decode()


def test_every_instance_is_in_the_matrix():
    """Every case describes (dmf_select_describe, level 0) as the kernels it claims, and the lists name every instance:
    k_u_inner_rows at 1..32 unknowns, k_inner_bu at 1..16 x {one, two sample groups} x {even, odd S}."""
    rows, bu = set(), set()
    for c in QUAD:
        assert _describe(c).startswith(f"rowpass={SPLIT} "), (c, _describe(c))
        assert c.n_iter2 == SPLIT_STEPS and c.N == 9 * (64 // c.n_u) + 1 and c.unsup == (c.n_c == 0)
        rows.add(c.n_u)
    for c in DPP:
        # the solver fuses the b_u stream in at up to 16 unknowns; the stand-alone u phase (dmf_update_u) runs the same
        # producer and k_u_inner_rows behind it
        assert _describe(c).startswith(f"rowpass={CM_BU if c.n_u <= 16 else CM_ROWS} "), (c, _describe(c))
        rows.add(c.n_u)
    assert {(c.n_u, c.n_c, c.unsup) for c in DPP} == {(n_u, n_c, unsup) for n_u in range(5, 33)
                                                      for n_c, unsup in ((0, False), (2, False), (0, True))}
    for c in CHUNKED:
        assert _describe(c).startswith(f"rowpass={SPLIT if c.n_u <= 4 else CM_ROWS} "), (c, _describe(c))
        assert c.n_iter2 == BETA_CHUNK + 1 and c.N <= 48
    assert [c.n_u for c in CHUNKED] == [2, 5, 17]  # one per lane layout
    for c in INNER_BU:
        assert _describe(c).startswith(f"rowpass={CM_BU} "), (c, _describe(c))
        nsg = 1 if c.S <= 128 else 2
        assert c.N == 2 * 16 * nsg + 3
        bu.add((c.n_u, nsg, c.S % 2 == 1))
    assert rows == set(range(1, 33)), sorted(set(range(1, 33)) - rows)
    want = {(n_u, nsg, odd) for n_u in range(1, 17) for nsg in (1, 2) for odd in (False, True)}
    assert bu == want and len(INNER_BU) == 64, sorted(want - bu)


# ----------------------------------------------------------------------------------------- the instances
@pytest.mark.gpu
@pytest.mark.parametrize("case", QUAD, ids=_id)
def test_row_groups_against_oracle(ctx, case):
    data = solver_inputs(case)
    wu, wa = solver_oracle(case, *data)
    u, alpha = solver_run(ctx, case, *data, SPLIT)
    assert rel_err(alpha, wa) < TIGHT and np.abs(alpha - wa).max() < TIGHT and np.abs(u - wu).max() < TIGHT


@pytest.mark.gpu
@pytest.mark.parametrize("case", DPP, ids=_id)
def test_dpp_rows_against_oracle(ctx, case):
    """One u phase from a non-initial momentum state: k_cm_i8 + k_u_inner_rows, one row per DPP row or per two."""
    data = update_u_inputs(case)
    want = update_u_oracle(case, *data)
    got = update_u_run(ctx, case, *data)
    assert np.abs(got[0] - want[0]).max() < KAT and np.abs(got[1] - want[1]).max() < KAT


@pytest.mark.gpu
@pytest.mark.parametrize("case", CHUNKED, ids=_id)
def test_chunked_momentum_table_against_oracle(ctx, case):
    data = solver_inputs(case)
    wu, wa = solver_oracle(case, *data)
    u, alpha = solver_run(ctx, case, *data, SPLIT if case.n_u <= 4 else CM_ROWS)
    assert np.abs(alpha - wa).max() < TIGHT and np.abs(u - wu).max() < TIGHT


@pytest.mark.gpu
@pytest.mark.parametrize("case", INNER_BU, ids=_id)
def test_inner_bu_against_oracle(ctx, case):
    data = solver_inputs(case)
    wu, wa = solver_oracle(case, *data)
    u, alpha = solver_run(ctx, case, *data, CM_BU)
    assert rel_err(alpha, wa) < TIGHT and np.abs(alpha - wa).max() < TIGHT and np.abs(u - wu).max() < TIGHT
