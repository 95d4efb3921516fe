"""The row pass's written-out inner steps and its M combine with digit pairs joined in i32, on the pair schedule.

Two things changed in k_rowpass_v2 and neither may change a bit of any result.  The X16 form with up to four waves runs
its inner steps from a written-out loop when n_iter2 is the CLI's default of 20 (beta_t from a constant lane; the loop at
every other count), and phase A's M combine joins the digit sums mw[2k] + 256 mw[2k+1] in i32 before it converts them.
Each case therefore asks two things of three one-iteration steps: the pair schedule against the one-block loop bit for
bit, and the pair run against the numpy oracle at the bar of tests/test_gpu_rowpass_pair.py.

Shapes: row counts that give every workgroup exactly 1, 2, 3 and 5 blocks with a ragged last block (a lone last block,
one pair, a pair and a lone block, two pairs and a lone block); 1, 2, 19, 20, 21 and 50 inner steps (20 is the one
written-out count: 19 and 21 are its neighbours, which take the loop); one to four unknowns (three take the shuffle
step); 0, 3, 12 and 16 known types; two, three and four waves; the unsupervised gradient point, also at 20 steps; two
count digits, where the digit sums reach weight 256^7 and both halves of the combine carry."""
import numpy as np
import pytest

from oracle import solver as osol

from conftest import rel_err
from test_gpu_rowpass_pair import TIGHT, _problem, _run

pytestmark = pytest.mark.gpu

T1 = 3


def _rows(k, S):
    """A row count that gives every row-pass workgroup exactly k blocks, the last block of the grid ragged: the grid is
    512 workgroups at three or four waves and 1024 at two (two workgroups per SIMD pair of waves)."""
    return 16 * (1024 if S <= 128 else 512) * k - 5


# (blocks per workgroup, S, n_c, n_u, n_iter2, depth, why)
CASES = [
    (1, 256, 12, 4, 20, 50, "lone last block only"),
    (2, 256, 12, 4, 20, 50, "one pair per workgroup"),
    (3, 256, 12, 4, 20, 50, "a pair and a lone block"),
    (5, 130, 12, 4, 20, 50, "two pairs and a lone block, three waves, last column group of two samples"),
    (3, 256, 12, 4, 21, 120, "two count digits on the bench's instance, 21 inner steps: the loop"),
    (2, 255, 12, 4, 20, 120, "two count digits, the written-out steps, odd S"),
    (3, 192, 0, 1, 1, 50, "unsupervised gradient point, no known types, one inner step, three waves"),
    (2, 128, 3, 2, 2, 50, "two waves (1024 workgroups), one block of known types, two inner steps"),
    (3, 255, 12, 3, 19, 50, "odd S, shuffle step, 19 inner steps: the loop"),
    (2, 200, 3, 3, 20, 50, "shuffle step in the written-out steps, ragged column group"),
    (2, 192, 3, 3, 50, 120, "shuffle step, two count digits, 50 inner steps"),
    (2, 256, 16, 4, 21, 50, "16 known types"),
    (2, 96, 16, 3, 50, 50, "two waves, 16 known types, three unknowns, 50 inner steps"),
    (3, 200, 0, 4, 20, 50, "unsupervised with four unknowns, the written-out steps at the previous iterate"),
    (2, 255, 3, 1, 20, 50, "one unknown with known types"),
    (3, 128, 12, 2, 20, 50, "two waves, 12 known types, two unknowns"),
]


def _oracle(V, D, Rt, u0, a0, n_u, n_iter2):
    if Rt is not None:
        return osol.solve_partial(u0.copy(), np.c_[Rt, u0], a0.copy(), V, D, Rt, n_u, T1, n_iter2, 0.0,
                                  project=osol.simplex_project_columns_fast)
    return osol.solve_unsupervised(V, n_u, D, "uniform_", T1, n_iter2, 0.0, init=(u0.copy(), a0.copy()),
                                   project=osol.simplex_project_columns_fast)


@pytest.mark.parametrize("k,S,n_c,n_u,n_iter2,depth,why", CASES)
def test_pair_schedule_is_bit_identical_and_matches_the_oracle(ctx, k, S, n_c, n_u, n_iter2, depth, why):
    N = _rows(k, S)
    V, D, Rt, u0, a0 = _problem(N, S, n_c, n_u, depth)
    assert (D.max() > 127) == (depth == 120), D.max()  # one or two count digits, as the case says
    wu, wa = _oracle(V, D, Rt, u0, a0, n_u, n_iter2)
    d_one, one, c_one, l_one = _run(ctx, V, D, Rt, u0, a0, n_iter2, T1, False)
    d_two, two, c_two, l_two = _run(ctx, V, D, Rt, u0, a0, n_iter2, T1, True)
    assert "k_rowpass_v2" in d_two and " x16 " in d_two, d_two
    assert l_one == (T1, 0), l_one
    assert l_two == (T1, T1), (why, l_two)  # every row-pass launch ran the pair schedule
    assert d_one == d_two
    for step, (a, b) in enumerate(zip(one, two)):
        for name, x, y in zip(("u", "alpha", "cost", "iterations"), a, b):
            assert np.array_equal(x, y), (why, step, name)
    assert c_one == c_two
    u, alpha = two[-1][:2]
    du, da = float(np.abs(u - wu).max()), rel_err(alpha, wa)
    print(f"{why}: max|u - oracle| = {du:.3e}, rel |alpha - oracle| = {da:.3e}")
    assert da < TIGHT and du < TIGHT, (why, du, da)
