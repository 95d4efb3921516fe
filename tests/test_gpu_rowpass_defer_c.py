"""The row pass's deferred-C schedule (dmf_context_set_rowpass_defer_c) against the pair schedule it is built on.

Each case creates the same problem and solver twice in one process, with the switch on and off, on the same seeded inputs,
and runs K outer iterations: the two schedules add every sum on the same wave in the same order, so u, the momentum state's
u_prev and alpha_prev, alpha, the packed Gram of the last iteration and the direct cost must agree bit for bit.  The
solver's schedule counter must show the deferred schedule where it applies (four waves, X16, every count <= 255, not 13 to
16 known types with three or four unknowns) and nowhere else.  Row counts are derived from the grid rule so that a workgroup owns the block counts that exercise a lone
block, a pair and a lone block, the ring's wrap-around and the drain with one and with two pairs pending; the host model
(tests/rowpass_schedule_model.py) confirms the block counts and walks the schedule for them."""
import numpy as np
import pytest

import rowpass_schedule_model as model

pytestmark = pytest.mark.gpu

K_ITERS = 2


def _inputs(N, S, n_c, n_u, counts, seed):
    """Seeded V = X / D with integer X <= D, R_trunc and a starting point.  counts = (lo, hi, n_top): D uniform in
    lo..hi, and n_top elements with D = X = hi (so x reaches the largest count)."""
    lo, hi, n_top = counts
    rs = np.random.RandomState(seed)
    D = rs.randint(lo, hi + 1, size=(N, S)).astype(np.int64)
    X = np.floor(D * rs.random_sample((N, S))).astype(np.int64)
    top = rs.choice(N * S, size=n_top, replace=False)
    D.flat[top] = hi
    X.flat[top] = hi
    V = X / D
    Rt = rs.beta(0.5, 0.5, size=(N, n_c)) if n_c else None
    u0 = rs.uniform(0.05, 0.95, size=(N, n_u))
    a0 = rs.dirichlet(np.ones(n_c + n_u), S).T.copy()
    return V, D, Rt, u0, a0


def _run(ctx, V, D, Rt, u0, a0, n_iter2, defer_c, x16=True, derive=None):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    mode = L.DMF_MODE_PARTIAL if Rt is not None else L.DMF_MODE_UNSUPERVISED
    ctx.set_x16(x16)
    ctx.set_rowpass_defer_c(defer_c)
    try:
        with Problem(ctx, V, D, Rt) as full:
            p = derive(full) if derive is not None else full
            try:
                with Solver(p, u0, a0, mode) as s:
                    desc = s.describe(n_iter2)
                    word = model.schedule_in_text(s.u_phase_describe(n_iter2))  # the plan's schedule, before any launch
                    s.step(K_ITERS, n_iter2, 0.0)
                    u, alpha = s.get()[:2]
                    mom = s.momentum_state()
                    gram = s.gram("last")[0]
                    counts = s.rowpass_schedule_counts()
                    assert counts == model.expected_counts(word, counts[0])[:3], (word, counts)  # ... is what the launches ran
                    return {"u": u, "alpha": alpha, "u_prev": mom["u_prev"], "alpha_prev": mom["alpha_prev"], "gram": gram,
                            "direct_cost": np.float64(s.direct_cost())}, desc, counts, s.rowpass_launches()
            finally:
                if p is not full:
                    p.close()
    finally:
        ctx.set_rowpass_defer_c(True)
        ctx.set_x16(True)


def _rows(blocks, off):
    """N for `blocks` 16-row blocks with a ragged last one."""
    return 16 * blocks - off


def _mask(N, S):
    return np.random.RandomState(5).random_sample((N, S)) >= 0.2


def _gather_idx(N):
    return np.random.RandomState(6).randint(0, N, size=N - 37)


# (blocks, off, (nk lo, nk hi), S, n_c, n_u, n_iter2, (lo, hi, n_top), set-up, deferred, paired, why)
CASES = [
    (812, 5, (1, 2), 256, 12, 4, 20, (1, 255, 64), None, True, True, "lone block / one pair; x = 255; two digit planes"),
    (1224, 3, (2, 3), 193, 0, 1, 3, (1, 100, 8), None, True, True, "pair + lone block; unsupervised; ragged fourth wave"),
    (1636, 7, (3, 4), 255, 1, 2, 7, (128, 255, 64), None, True, True, "odd S, odd step count, counts in 128..255"),
    (2125, 1, (4, 5), 256, 16, 2, 20, (1, 120, 8), None, True, True, "ring wrap; drain with one and two pairs; one plane"),
    (1224, 3, (2, 3), 256, 16, 3, 20, (1, 120, 8), None, False, True, "16 known types, 3 unknowns: the instance is not built"),
    (3322, 9, (6, 7), 256, 12, 4, 20, (1, 200, 64), None, True, True, "six and seven blocks; the bench's kernel instance"),
    (300, 11, (1, 1), 256, 0, 4, 20, (1, 60, 8), None, True, True, "every workgroup a lone block; unsupervised, 4 unknowns"),
    (1224, 3, (2, 3), 256, 12, 4, 20, (1, 256, 64), None, False, True, "largest count 256: the pair schedule"),
    (1224, 3, (2, 3), 192, 12, 4, 20, (1, 100, 8), None, False, True, "three waves: the pair schedule"),
    (2100, 3, (2, 3), 128, 3, 2, 7, (1, 100, 8), None, False, True, "two waves: the pair schedule"),
    (1224, 3, (2, 3), 256, 12, 4, 20, (1, 100, 8), "no_x16", False, False, "no X16: the V form, one block at a time"),
    (1636, 7, (3, 4), 256, 12, 4, 20, (1, 255, 64), "masked", True, True, "a masked problem"),
    (1636, 7, (3, 4), 256, 12, 2, 20, (1, 255, 64), "gathered", True, True, "a gathered problem"),
]


@pytest.mark.parametrize("blocks,off,nk,S,n_c,n_u,n_iter2,counts,setup,deferred,paired,why", CASES)
def test_deferred_c_is_bit_identical(ctx, blocks, off, nk, S, n_c, n_u, n_iter2, counts, setup, deferred, paired, why):
    N = _rows(blocks, off)
    assert N % 16 != 0
    V, D, Rt, u0, a0 = _inputs(N, S, n_c, n_u, counts, seed=blocks + S)
    derive, x16, n_rows = None, True, N
    if setup == "masked":
        derive = lambda p: p.masked(_mask(N, S))
    elif setup == "gathered":
        idx = _gather_idx(N)
        derive, n_rows = (lambda p: p.gather(idx)), idx.size
        u0 = u0[:n_rows].copy()
    elif setup == "no_x16":
        x16 = False
    # the block counts this case is about, from the grid rule, and the schedule walked for them
    assert model.blocks_per_workgroup(n_rows, S) == nk, (why, model.blocks_per_workgroup(n_rows, S))
    for k in range(nk[0], nk[1] + 1):
        model.check(k)
    assert model.runs_deferred(S, n_c, n_u, n_iter2, counts[1], x16=x16) == deferred, why

    on, d_on, c_on, l_on = _run(ctx, V, D, Rt, u0, a0, n_iter2, True, x16, derive)
    off_, d_off, c_off, l_off = _run(ctx, V, D, Rt, u0, a0, n_iter2, False, x16, derive)
    assert "k_rowpass_v2" in d_on and d_on == d_off, (d_on, d_off)
    assert c_on[0] >= K_ITERS and c_on[:2] == l_on and c_off[:2] == l_off
    assert c_on[1] == (c_on[0] if paired else 0), (why, c_on)
    assert c_on[2] == (c_on[0] if deferred else 0), (why, c_on)
    assert c_off == (c_on[0], c_on[1], 0), (why, c_off)
    for name in ("u", "u_prev", "alpha_prev", "alpha", "gram", "direct_cost"):
        assert np.array_equal(on[name], off_[name]), (why, name)
    assert np.isfinite(on["u"]).all() and np.isfinite(on["gram"]).all() and np.isfinite(on["direct_cost"])
