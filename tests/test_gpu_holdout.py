"""Hold-out masks on the device: Problem.masked (dmf_problem_mask), Solver.holdout_error (dmf_solver_holdout_error) and the
bi-cross-validation driver built on them.

A  the masked problem derived on the device is the problem a re-upload of the host-masked arrays creates: same kernels
   (describe), same iterates, loop cost and streaming cost, bit for bit
B  the error pass against numpy on the GPU's own iterate, 1e-11 relative (the bar cost_f_w is held to); n_test exact
C  the solve against the oracle on the host-masked arrays, 1e-8 (the suite's bar)
D  bicross_validation / evaluate_best_ic give what the loop they replace gave (host masks, a fresh Problem per fold,
   numpy error), from one upload
E  refusals, and the lifetime rule: a masked problem is a full copy, its parent may be closed first
"""
import functools

import numpy as np
import pytest

from oracle import solver as osol

from conftest import load_toy, rel_err

pytestmark = pytest.mark.gpu

TIGHT = 1e-8    # oracle parity, as in tests/test_gpu_bench_paths.py
ERR_RTOL = 1e-11  # the error pass (cost_f_w's bar)

# name -> (N, S, n_c, n_u, depth, variant)
SHAPES = {
    "toy": (350, 10, 5, 1, None, "toy"),                 # the upstream toy
    "odd_s": (77, 13, 3, 2, 50, ""),                     # odd S, row tails of both 16 and 32
    "unsupervised": (1000, 70, 0, 3, 50, ""),            # no known types, ragged second column group
    "wide_rows": (257, 130, 2, 5, 50, ""),               # wide-row-group path (and the wide u16 cost kernel)
    "eight_waves": (96, 300, 1, 1, 50, ""),              # eight-wave row pass (and the two-samples-per-lane cost kernel)
    "two_digits": (200, 64, 2, 2, 300, ""),              # two count digits
    "count_40000": (64, 9, 2, 1, 50, "big"),             # a count of 40000: no integer copies
    "one_sample": (50, 1, 2, 1, 50, ""),                 # S = 1: no integer copies
    "x16_off": (77, 13, 3, 2, 50, "x16_off"),            # X16 switched off
    "two_decimals": (77, 13, 3, 2, 50, "round"),         # X16 rejected: the V form of the row pass
    "k_cost_u16": (40, 20, 1, 5, 50, ""),                # integer copies, but the any-shape k_cost: f64 weights on demand
}
FIRST_FOUR = ["toy", "odd_s", "unsupervised", "wide_rows"]
T2 = {"odd_s": 1, "eight_waves": 50}  # inner iterations (20 elsewhere)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(V, D, Rt or None, mask, u0, a0) -- computed once per session and never written to."""
    N, S, n_c, n_u, depth, variant = SHAPES[name]
    if variant == "toy":
        V, D, Rt, _ = load_toy()
        V, D, Rt = np.ascontiguousarray(V), np.ascontiguousarray(D, dtype=np.int64), np.ascontiguousarray(Rt, dtype=np.float64)
    else:
        V, D, Rt = osol.synthetic_problem(N, S, n_c, n_u, seed=len(name), depth=depth)
        if n_c == 0:
            Rt = None
    rs = np.random.RandomState(100 + N)
    mask = rs.rand(N, S) < 0.3  # (1 = train, as ic.py:68)
    mask[1, :] = False          # one fully held-out row
    if S > 1:
        mask[:, S - 1] = False  # one fully held-out sample
    mask[2, :max(S - 1, 1)] = True  # one kept row (all of it but the held-out sample)
    if variant == "big":
        D = D.copy()
        D[2, 0] = 40000         # (in the kept row: the masked problem has no integer copies either)
        V = V.copy()
        V[2, 0] = 12345 / 40000
    if variant == "round":
        V = np.round(V, 2)
    if n_c:
        u0, _, a0 = osol.init_partial("uniform_", V, D, Rt, n_u, seed=1)
    else:
        u0, a0 = osol.init_unsupervised("uniform_", V, n_u, seed=1)
    for a in (V, D, mask, u0, a0) + ((Rt,) if Rt is not None else ()):
        a.setflags(write=False)
    return V, D, Rt, mask, u0, a0


class _x16:
    def __init__(self, ctx, name):
        self.ctx, self.off = ctx, SHAPES[name][5] == "x16_off"

    def __enter__(self):
        if self.off:
            self.ctx.set_x16(False)

    def __exit__(self, *exc):
        self.ctx.set_x16(True)


def _mode(Rt):
    from demethify_amd import _lib as L

    return L.DMF_MODE_PARTIAL if Rt is not None else L.DMF_MODE_UNSUPERVISED


def _run(problem, u0, a0, Rt, n_outer, t2):
    """-> (describe, u, alpha, loop cost, streaming cost, solver still open)"""
    from demethify_amd.device import Solver

    s = Solver(problem, u0, a0, _mode(Rt))
    desc = s.describe(t2)
    s.step(n_outer, t2, 0.0)
    u, alpha, cost, _ = s.get()
    return desc, u, alpha, cost, s.direct_cost(), s


def _numpy_error(V, Rt, u, alpha, mask):
    R = np.hstack((Rt, u)) if Rt is not None else u
    return np.linalg.norm((V - R @ alpha) * ~mask, "fro") ** 2


# ---------------------------------------------------------------------------------------------- A and B
@pytest.mark.parametrize("name", list(SHAPES))
def test_derived_problem_is_the_reuploaded_one_and_error_pass_matches_numpy(ctx, name):
    from demethify_amd.device import Problem

    V, D, Rt, mask, u0, a0 = _case(name)
    t2 = T2.get(name, 20)
    with _x16(ctx, name), Problem(ctx, V, D, Rt) as parent, parent.masked(mask) as derived, \
            Problem(ctx, V * mask, D * mask, Rt) as again:
        d_desc, d_u, d_alpha, d_cost, d_direct, ds = _run(derived, u0, a0, Rt, 3, t2)
        a_desc, a_u, a_alpha, a_cost, a_direct, as_ = _run(again, u0, a0, Rt, 3, t2)
        try:
            # A
            assert d_desc == a_desc
            if name in ("count_40000", "one_sample"):
                assert "k_rowpass_v2" not in d_desc and "i8" not in d_desc, d_desc  # (no integer copies on either side)
            if name in ("x16_off", "two_decimals"):
                assert "k_rowpass_v2" in d_desc and "x16" not in d_desc, d_desc
            assert np.array_equal(d_u, a_u) and np.array_equal(d_alpha, a_alpha)
            assert d_cost == a_cost and d_direct == a_direct
            # B
            sum_sq, n_test = ds.holdout_error(parent)
            want = _numpy_error(V, Rt, d_u, d_alpha, mask)
            print(f"{name}: holdout {sum_sq!r} numpy {want!r} rel {abs(sum_sq - want) / want:.2e} n_test {n_test}")
            assert n_test == int((~mask).sum())
            assert abs(sum_sq - want) <= ERR_RTOL * want
        finally:
            ds.close()
            as_.close()


@pytest.mark.parametrize("name", ["odd_s", "count_40000"])
def test_nothing_held_out(ctx, name):
    """An all-ones mask: the masked problem is the parent (bit-identical solve), n_test = 0 and the error 0.0."""
    from demethify_amd.device import Problem

    V, D, Rt, mask, u0, a0 = _case(name)
    with Problem(ctx, V, D, Rt) as parent, parent.masked(np.ones_like(mask)) as derived:
        p_desc, p_u, p_alpha, p_cost, p_direct, ps = _run(parent, u0, a0, Rt, 3, 20)
        d_desc, d_u, d_alpha, d_cost, d_direct, ds = _run(derived, u0, a0, Rt, 3, 20)
        try:
            assert ds.holdout_error(parent) == (0.0, 0)
            assert d_desc == p_desc and np.array_equal(d_u, p_u) and np.array_equal(d_alpha, p_alpha)
            assert d_cost == p_cost and d_direct == p_direct
        finally:
            ps.close()
            ds.close()


def test_mask_forms_are_one_mask(ctx):
    """bool array, packed host bits, packed uint8 CUDA tensor, staged upload: the same masked problem."""
    import torch

    from demethify_amd.device import Problem, pack_mask
    from demethify_amd.staging import mask_to_device

    V, D, Rt, mask, u0, a0 = _case("odd_s")
    bits = pack_mask(mask)
    noisy = bits.copy()
    noisy[:, -1] |= 0xE0  # S = 13: bits 5..7 of the second byte are padding and are ignored
    with Problem(ctx, V, D, Rt) as parent:
        forms = [mask, bits, noisy, torch.from_numpy(bits).cuda(), mask_to_device(bits, ctx)]
        got = []
        for m in forms:
            with parent.masked(m) as derived:
                _, u, alpha, cost, _, s = _run(derived, u0, a0, Rt, 2, 20)
                got.append((u, alpha, cost, s.holdout_error(parent)))
                s.close()
    for u, alpha, cost, err in got[1:]:
        assert np.array_equal(u, got[0][0]) and np.array_equal(alpha, got[0][1]) and cost == got[0][2] and err == got[0][3]


def test_mask_that_removes_the_second_count_digit(ctx):
    """The mask removes every count above 127: the re-upload has one digit plane, the derived problem keeps the parent's
    two.  Both are exact integer arithmetic on the same counts, so they agree to 1e-10 instead of bit for bit -- which also
    pins max(D): the step lengths are 1 / (||.||^2 max(D)^2), and the parent's maximum (about 150 here against 127)
    would move the iterates by far more.  The oracle, whose d is (D * mask).max()**2, says the same at its own bar."""
    from demethify_amd.device import Problem

    N, S, n_c, n_u = 200, 64, 2, 2
    V, D, Rt = osol.synthetic_problem(N, S, n_c, n_u, seed=5, depth=110)
    mask = D <= 127
    assert D.max() > 140 and (D * mask).max() == 127 and 0.02 < (~mask).mean() < 0.5
    u0, R0, a0 = osol.init_partial("uniform_", V, D, Rt, n_u, seed=1)
    with Problem(ctx, V, D, Rt) as parent, parent.masked(mask) as derived, Problem(ctx, V * mask, D * mask, Rt) as again:
        d_desc, d_u, d_alpha, d_cost, d_direct, ds = _run(derived, u0, a0, Rt, 3, 20)
        a_desc, a_u, a_alpha, a_cost, a_direct, as_ = _run(again, u0, a0, Rt, 3, 20)
        ds.close()
        as_.close()
    assert "nd=2" in d_desc and "nd=1" in a_desc, (d_desc, a_desc)
    print("digit case:", rel_err(d_u, a_u), rel_err(d_alpha, a_alpha), abs(d_cost - a_cost) / a_cost)
    assert rel_err(d_u, a_u) <= 1e-10 and rel_err(d_alpha, a_alpha) <= 1e-10
    assert abs(d_cost - a_cost) <= 1e-10 * a_cost and abs(d_direct - a_direct) <= 1e-10 * a_direct
    wu, wa = osol.solve_partial(u0.copy(), R0, a0.copy(), V * mask, D * mask, Rt, n_u, 3, 20, 0.0,
                                project=osol.simplex_project_columns_fast)
    assert rel_err(d_alpha, wa) < TIGHT and np.abs(d_u - wu).max() < TIGHT


# ---------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("name", FIRST_FOUR)
def test_masked_solve_matches_the_oracle(ctx, name):
    from demethify_amd.device import Problem

    V, D, Rt, mask, u0, a0 = _case(name)
    n_u = SHAPES[name][3]
    Vm, Dm = V * mask, D * mask
    if Rt is not None:
        wu, wa = osol.solve_partial(u0.copy(), np.c_[Rt, u0], a0.copy(), Vm, Dm, Rt, n_u, 30, 20, 0.0,
                                    project=osol.simplex_project_columns_fast)
    else:
        wu, wa = osol.solve_unsupervised(Vm, n_u, Dm, "uniform_", 30, 20, 0.0, init=(u0.copy(), a0.copy()),
                                         project=osol.simplex_project_columns_fast)
    with Problem(ctx, V, D, Rt) as parent, parent.masked(mask) as derived:
        _, u, alpha, _, _, s = _run(derived, u0, a0, Rt, 30, 20)
        s.close()
    print(f"{name}: alpha {rel_err(alpha, wa):.2e} u {np.abs(u - wu).max():.2e}")
    assert rel_err(alpha, wa) < TIGHT and np.abs(u - wu).max() < TIGHT


# ---------------------------------------------------------------------------------------------- D
def _old_bicross_validation(meth_f, n_u, counts, iter1, iter2, tol, n_folds=10, seed=None, ref=None,
                            init_option="uniform_", fraction=0.3):
    """The loop bicross_validation replaces: host masks, a fresh Problem per fold, numpy error."""
    from demethify_amd.ic import run_deconvolution

    np.random.seed(seed)
    total_press, best_u, best_alpha, min_error, winner = 0, None, None, float("inf"), None
    for fold in range(n_folds):
        train_mask = np.random.rand(*meth_f.shape) < fraction
        test_mask = ~train_mask
        if np.sum(test_mask) == 0 or np.sum(train_mask) == 0:
            continue
        u, R, alpha = run_deconvolution(meth_f * train_mask, counts * train_mask, ref, n_u, init_option, seed,
                                        iter1, iter2, tol)
        test_error = np.linalg.norm((meth_f - R @ alpha) * test_mask, "fro") ** 2 / np.sum(test_mask)
        total_press += test_error
        if test_error < min_error:
            min_error, best_u, best_alpha, winner = test_error, u, alpha, fold
    return total_press, best_u, best_alpha, winner


ITERS = (40, 20, 1e-3)


@pytest.mark.parametrize("with_ref,n_u", [(True, 1), (False, 2)])
def test_bicross_validation_gives_what_the_old_loop_gave(ctx, toy, with_ref, n_u):
    from demethify_amd.ic import bicross_validation

    V, D, ref, _ = toy
    ref = ref if with_ref else None
    want_total, want_u, want_alpha, winner = _old_bicross_validation(V, n_u, D, *ITERS, n_folds=4, seed=1, ref=ref)
    total, best_u, best_alpha = bicross_validation(V, n_u, D, *ITERS, n_folds=4, seed=1, ref=ref)
    print(f"BCV total {total!r} old {want_total!r} winner fold {winner}")
    assert abs(total - want_total) <= 1e-11 * want_total
    # the same fold won: its factors come back, and they are the old loop's bit for bit
    assert np.array_equal(best_u, want_u) and np.array_equal(best_alpha, want_alpha)


@pytest.mark.parametrize("ic", ["BCV", "CCC"])
def test_model_selection_sweep_uploads_once_and_scores_as_before(ctx, toy, ic, monkeypatch):
    from demethify_amd import device
    from demethify_amd import ic as ic_mod

    V, D, ref, _ = toy
    n_restarts, seed, cands = 3, 1, [1, 2, 3]
    want_scores, want_best = [], (float("inf"), None)
    for n_u in cands:  # the sweep as it was: evaluate_best_ic's loop over the old per-candidate drivers
        if ic == "CCC":
            runs = [ic_mod.run_deconvolution(V, D, ref, n_u, "uniform_", seed + r, *ITERS)[2] for r in range(n_restarts)]
            score = -ic_mod.compute_ccc(runs)
            u, alpha = None, runs[-1]
        else:
            score, u, alpha, _ = _old_bicross_validation(V, n_u, D, *ITERS, n_folds=n_restarts, seed=seed, ref=ref)
        want_scores.append(score)
        if score < want_best[0]:
            want_best = (score, n_u, u, alpha)

    uploads = []
    init = device.Problem.__init__

    def counting_init(self, *args, **kwargs):
        uploads.append(1)
        return init(self, *args, **kwargs)

    monkeypatch.setattr(device.Problem, "__init__", counting_init)
    u, alpha, n_best, scores = ic_mod.evaluate_best_ic(V, ref, D, "uniform_", ic, seed, *ITERS, n_restarts=n_restarts,
                                                       n_u_values=cands)
    assert len(uploads) == 1
    print(ic, scores, want_scores)
    assert n_best == want_best[1]
    if ic == "CCC":
        # (the same solves on one upload instead of a fresh one each)
        assert np.array_equal(np.asarray(scores, dtype=float), np.asarray(want_scores, dtype=float), equal_nan=True)
    else:
        assert np.allclose(scores, want_scores, rtol=1e-11, atol=0.0)
        assert np.array_equal(u, want_best[2])
    assert np.array_equal(alpha, want_best[3])


# ---------------------------------------------------------------------------------------------- E
def test_refusals(ctx):
    from demethify_amd._lib import DemethifyHipError
    from demethify_amd.device import Problem, Solver, pack_mask

    V, D, Rt, mask, u0, a0 = _case("odd_s")
    N, S = V.shape
    bits = pack_mask(mask)
    with Problem(ctx, V, D, Rt) as parent, parent.masked(mask) as derived, \
            Problem(ctx, V[:-1], D[:-1], Rt[:-1]) as shorter, Problem(ctx, V, D, None) as no_ref:
        for bad in (bits[:-1], bits[:, :1], np.c_[bits, bits], bits.ravel(), mask[:, :-1], mask.T, bits.astype(np.int32)):
            with pytest.raises((ValueError, TypeError)):
                parent.masked(bad)
        with Solver(derived, u0, a0, _mode(Rt)) as s:
            for other in (shorter, no_ref):
                with pytest.raises(DemethifyHipError) as e:
                    s.holdout_error(other)
                assert e.value.status == 2  # DMF_ERR_BAD_SHAPE
            with pytest.raises(DemethifyHipError) as e:
                s.holdout_error(derived)  # a masked problem is not the full data
            assert e.value.status == 1
        with Solver(parent, u0, a0, _mode(Rt)) as s:
            with pytest.raises(DemethifyHipError) as e:
                s.holdout_error(parent)  # the solver's problem holds nothing out
            assert e.value.status == 1
        for idx in (np.arange(N), np.array([0, 0, 5])):
            with pytest.raises(DemethifyHipError) as e:
                derived.gather(idx)
            assert e.value.status == 1
        with pytest.raises(DemethifyHipError) as e:
            derived.masked(mask)  # one mask per problem
        assert e.value.status == 1


def test_masked_problem_outlives_its_parent(ctx):
    """dmf_problem_mask makes a full copy: closing the parent first is safe, and the solve is the same."""
    from demethify_amd._lib import DemethifyHipError
    from demethify_amd.device import Problem

    V, D, Rt, mask, u0, a0 = _case("odd_s")
    with Problem(ctx, V * mask, D * mask, Rt) as again:
        _, a_u, a_alpha, a_cost, _, as_ = _run(again, u0, a0, Rt, 3, 20)
        as_.close()
    parent = Problem(ctx, V, D, Rt)
    derived = parent.masked(mask)
    parent.close()
    # (other allocations take the parent's blocks in the meantime)
    with Problem(ctx, np.ones_like(V), D, Rt):
        pass
    _, d_u, d_alpha, d_cost, _, ds = _run(derived, u0, a0, Rt, 3, 20)
    try:
        assert np.array_equal(d_u, a_u) and np.array_equal(d_alpha, a_alpha) and d_cost == a_cost
        with pytest.raises(DemethifyHipError):
            ds.holdout_error(parent)  # the error pass needs the full data: a closed parent is refused, not read
    finally:
        ds.close()
        derived.close()
