"""The row pass's pair schedule (two 16-row blocks per phase B, X16 form, 65..256 samples) against the one-block loop.

Each case creates the same problem and solver twice in one process, once with the context's pair switch off and once with
it on, and steps both the same way: the two forms sum every value in the same order, so every result must agree bit for
bit.  The cases cover odd and ragged sample counts, one to four unknowns, 0 to 16 known types, both modes, 1 to 50 inner
steps, two-digit counts, and row counts that leave the row pass's workgroups one, two or an odd number of blocks.  Each
run also reports how many of its row-pass launches ran the pair schedule: all of them with the switch on where the shape
admits it, none otherwise (two waves and four unknowns do not: four such workgroups per CU would not fit its LDS)."""
import numpy as np
import pytest

from oracle import solver as osol

import rowpass_schedule_model as model
from conftest import rel_err

pytestmark = pytest.mark.gpu

TIGHT = 1e-8  # oracle parity, as in tests/test_gpu_bench_paths.py


def _run(ctx, V, D, Rt, u0, a0, n_iter2, n_calls, pair, x16=True):
    """(describe, the get() trail of n_calls one-iteration steps, direct_cost(), rowpass_launches()) with the context's
    pair and X16 switches set before the Problem is created (X16 is built, or not, at creation); both are reset after.
    Shared with tests/test_gpu_rowpass_forms.py."""
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    mode = L.DMF_MODE_PARTIAL if Rt is not None else L.DMF_MODE_UNSUPERVISED
    ctx.set_x16(x16)
    ctx.set_rowpass_pair(pair)
    try:
        with Problem(ctx, V, D, Rt) as p, Solver(p, u0, a0, mode) as s:
            desc = s.describe(n_iter2)
            word = model.schedule_in_text(s.u_phase_describe(n_iter2))  # the plan's schedule, before any launch
            trail = []
            for _ in range(n_calls):
                s.step(1, n_iter2, 0.0)
                trail.append(s.get())
            launches = s.rowpass_launches()
            assert launches == model.expected_counts(word, launches[0])[:2], (word, launches)  # ... is what the launches ran
            return desc, trail, s.direct_cost(), launches
    finally:
        ctx.set_rowpass_pair(True)
        ctx.set_x16(True)


def _problem(N, S, n_c, n_u, depth, seed=0):
    V, D, Rt = osol.synthetic_problem(N, S, n_c, n_u, seed=seed, depth=depth)
    if n_c:
        u0, _, a0 = osol.init_partial("uniform_", V, D, Rt, n_u, seed=1)
    else:
        Rt = None
        u0, a0 = osol.init_unsupervised("uniform_", V, n_u, seed=1)
    return V, D, Rt, u0, a0


# (N, S, n_c, n_u, n_iter2, depth, paired, why).  Row pass grid: min(blocks, 512) workgroups at 3-4 waves, min(blocks,
# 1024) at 2.  paired: whether the pair schedule applies (the launch plan's rule: tests/rowpass_schedule_model.py, which
# tests/test_rowpass_plan_host.py holds this column to).
CASES = [
    (40_000, 256, 12, 4, 20, 50, True, "the bench's shape in everything but the row count; 4-5 blocks per workgroup"),
    (8192 + 3, 255, 12, 4, 19, 50, True, "odd S, ragged last column group and last block, odd step count"),
    (5000 + 7, 192, 3, 3, 50, 50, True, "three waves, one known type block, 50 inner steps"),
    (3000 + 1, 130, 0, 1, 1, 50, True, "unsupervised gradient point, no known types, one inner step, three waves"),
    (2000 + 9, 65, 16, 4, 20, 50, False, "two waves, four unknowns: one block at a time (LDS for four workgroups per CU)"),
    (16 * 1500 + 7, 128, 3, 3, 50, 50, True, "two waves, three unknowns, 50 inner steps: pairs"),
    (16 * 300 - 5, 256, 12, 2, 20, 50, True, "300 blocks: one block per workgroup (the pair schedule's lone last block only)"),
    (16 * 812, 256, 12, 4, 20, 50, True, "812 blocks: one or two per workgroup"),
    (16 * 1636 + 9, 200, 12, 4, 20, 50, True, "1637 blocks: three or four per workgroup, ragged last block"),
    (16 * 2100 + 3, 96, 3, 2, 19, 50, True, "two waves, 2101 blocks over 1024 workgroups: two or three each"),
    (6000, 256, 12, 4, 20, 120, True, "two count digits"),
]


@pytest.mark.parametrize("N,S,n_c,n_u,n_iter2,depth,paired,why", CASES)
def test_pair_schedule_is_bit_identical(ctx, N, S, n_c, n_u, n_iter2, depth, paired, why):
    V, D, Rt, u0, a0 = _problem(N, S, n_c, n_u, depth)
    d_one, one, c_one, l_one = _run(ctx, V, D, Rt, u0, a0, n_iter2, 3, False)
    d_two, two, c_two, l_two = _run(ctx, V, D, Rt, u0, a0, n_iter2, 3, True)
    assert "k_rowpass_v2" in d_two and " x16 " in d_two, d_two
    assert l_one[0] >= 3 and l_one[1] == 0, l_one
    assert l_two[0] >= 3 and l_two[1] == (l_two[0] if paired else 0), (why, l_two)
    assert d_one == d_two
    for k, (a, b) in enumerate(zip(one, two)):
        for name, x, y in zip(("u", "alpha", "cost", "iterations"), a, b):
            assert np.array_equal(x, y), (why, k, name)
    assert c_one == c_two


def test_pair_schedule_matches_the_oracle(ctx):
    N, S, n_c, n_u, T1 = 3000 + 5, 192, 3, 2, 3
    V, D, Rt, u0, a0 = _problem(N, S, n_c, n_u, 50)
    R = osol.init_partial("uniform_", V, D, Rt, n_u, seed=1)[1]
    wu, wa = osol.solve_partial(u0.copy(), R, a0.copy(), V, D, Rt, n_u, T1, 20, 0.0,
                                project=osol.simplex_project_columns_fast)
    desc, trail, _, launches = _run(ctx, V, D, Rt, u0, a0, 20, T1, True)
    assert "k_rowpass_v2" in desc and " x16 " in desc, desc
    assert launches[0] >= T1 and launches[1] == launches[0], launches
    u, alpha = trail[-1][:2]
    assert rel_err(alpha, wa) < TIGHT and np.abs(u - wu).max() < TIGHT
