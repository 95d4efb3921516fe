"""Every reachable instance of the first-generation FP64 row kernels against a plain numpy reference: k_u_phase_mfma (120
instances, one-launch and split), k_u_phase_big, k_u_phase_gram and k_u_step_direct through the stand-alone u phase
(Problem.update_u) at 1e-11, k_rowpass_fused through the solver at 1e-8, the Gram that its phase C accumulates held to exact
integers or the derived bound (Solver.gram("last")), and bit-stability of the multi-block launches.

The tables live in tests/fp64_rowpass.py; tests/test_fp64_rowpass_host.py proves without a GPU that they reach every
reachable instance and that each case runs the plan it names.  Here every case first asserts that plan on the LIVE problem
(Solver.u_phase_describe) and then the numbers.  Shapes are the smallest that reach the feature: two full workgroups, one
more block and a ragged tail per instance; the persistent loops are reached by N alone (2 grid + 1 blocks on S = 8).

Bars.  One u phase of up to 5 inner steps: 1e-11 absolute on u and u_prev (the bar of tests/test_gpu_u_inner.py).  Beyond 5
inner steps (the split mode of narrow row groups starts at 51; a 6200-entry momentum table) and whole outer iterations: the
project's TIGHT = 1e-8.  Each case prints the deviation it measured ("DEV ...") before it asserts."""
import functools

import numpy as np
import pytest

import fp64_rowpass as fr
import gram_exact as ge

from conftest import rel_err

pytestmark = pytest.mark.gpu


def _at_level(ctx, level):
    class Scope:
        def __enter__(self):
            self.before = ctx.generic_level
            ctx.set_generic(level)

        def __exit__(self, *exc):
            ctx.set_generic(self.before)

    return Scope()


# ------------------------------------------------------------------------------------------------ stand-alone u phase
@functools.lru_cache(maxsize=4)
def _inputs(c):
    data = fr.update_u_inputs(c)
    for a in data:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return data


def _update_u_case(ctx, c):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    V, D, Rt, u, u_prev, alpha, a1, lwp, lw = _inputs(c)
    want_text = fr.expected_text(c)
    with _at_level(ctx, c.level), Problem(ctx, V, D, Rt) as p:
        with Solver(p, u, alpha) as s:
            assert s.u_phase_describe(c.n_iter2, "update_u") == want_text
        for unsup in (False, True):   # gradient at the extrapolated point (deconvolution.py:88) / the previous iterate (:163)
            wu, wup = fr.update_u_oracle(c, unsup, V, D, Rt, u, u_prev, alpha, a1, lwp, lw)
            gu, gup = p.update_u(u, u_prev, alpha, c.n_iter2, a1, lwp, lw,
                                 mode=L.DMF_MODE_UNSUPERVISED if unsup else L.DMF_MODE_PARTIAL)[:2]
            dev = max(float(np.abs(gu - wu).max()), float(np.abs(gup - wup).max()))
            print(f"DEV {c.kernel} {'kat' if c.n_iter2 <= fr.KAT_STEPS else 'tight'} {dev:.3e} {fr.uid(c)}{'-unsup' if unsup else ''} "
                  f"[{want_text.split(' nw=')[0]}]")
            assert dev < fr.tolerance(c), (fr.uid(c), unsup, dev)
            assert gu.min() >= 0.0 and gu.max() <= 1.0   # the clip, exactly
            if c.n_iter2 == 0:      # nothing ran: u and u_prev come back untouched
                assert np.array_equal(gu, u) and np.array_equal(gup, u_prev)
            else:
                assert not np.array_equal(gu, u)


@pytest.mark.parametrize("case", fr.mfma_instance_cases(), ids=fr.uid)
def test_u_phase_mfma_instances(ctx, case):
    _update_u_case(ctx, case)


@pytest.mark.parametrize("case", fr.big_instance_cases(), ids=fr.uid)
def test_u_phase_big_instances(ctx, case):
    _update_u_case(ctx, case)


@pytest.mark.parametrize("case", fr.gram_instance_cases(), ids=fr.uid)
def test_u_phase_gram_instances(ctx, case):
    _update_u_case(ctx, case)


@pytest.mark.parametrize("case", fr.direct_instance_cases(), ids=fr.uid)
def test_u_step_direct_shapes(ctx, case):
    _update_u_case(ctx, case)


@pytest.mark.parametrize("case", fr.row_edge_cases(), ids=fr.uid)
def test_row_edges(ctx, case):
    _update_u_case(ctx, case)


@pytest.mark.parametrize("case", fr.wrap_cases(), ids=fr.uid)
def test_workgroups_take_one_two_and_three_blocks(ctx, case):
    _update_u_case(ctx, case)


@pytest.mark.parametrize("case", fr.sample_edge_cases(), ids=fr.uid)
def test_sample_edges(ctx, case):
    _update_u_case(ctx, case)


@pytest.mark.parametrize("case", fr.inner_step_cases(), ids=fr.uid)
def test_inner_step_counts(ctx, case):
    _update_u_case(ctx, case)


@pytest.mark.parametrize("case", fr.data_edge_cases(), ids=fr.uid)
def test_data_edges(ctx, case):
    _update_u_case(ctx, case)


# ------------------------------------------------------------------------------------------------ fused row pass
def _fused_case(ctx, c):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    V, D, Rt = fr.fused_inputs(c)
    u0, a0, wu, wa = fr.solver_oracle(V, D, Rt, c.n_u, c.T1, c.n_iter2)
    mode = L.DMF_MODE_PARTIAL if c.n_c else L.DMF_MODE_UNSUPERVISED
    with _at_level(ctx, 0 if c.big else 4), Problem(ctx, V, D, Rt) as p, Solver(p, u0, a0, mode) as s:
        assert s.u_phase_describe(c.n_iter2) == fr.fused_text(c.N, c.S, c.n_c, c.n_u, c.n_iter2)
        assert " gram=fused " in s.describe(c.n_iter2)
        it, _ = s.step(c.T1, c.n_iter2, 0.0)
        assert it == c.T1
        u, alpha, cost, _ = s.get()
        direct = s.direct_cost()
    dev = max(float(np.abs(alpha - wa).max()), float(np.abs(u - wu).max()))
    print(f"DEV fused tight {dev:.3e} {fr.fid(c)} [k_rowpass_fused<{(c.n_c + 3) // 4},{c.n_u}> nw={(c.S + 63) // 64}]")
    assert rel_err(alpha, wa) < fr.TIGHT and np.abs(alpha - wa).max() < fr.TIGHT, c.why
    assert np.abs(u - wu).max() < fr.TIGHT, c.why
    if c.n_iter2 == 0:
        assert np.array_equal(u, u0)
    want = fr.osol.weighted_cost(V, np.c_[Rt, wu] if c.n_c else wu, wa, D)
    assert cost == pytest.approx(want, rel=1e-9) and direct == pytest.approx(want, rel=1e-11)


@pytest.mark.parametrize("case", fr.fused_instance_cases(), ids=fr.fid)
def test_fused_instances(ctx, case):
    _fused_case(ctx, case)


@pytest.mark.parametrize("case", fr.fused_wide_cases(), ids=fr.fid)
def test_fused_column_groups(ctx, case):
    _fused_case(ctx, case)


@pytest.mark.parametrize("case", fr.fused_wrap_cases(), ids=fr.fid)
def test_fused_workgroups_take_one_two_and_three_blocks(ctx, case):
    _fused_case(ctx, case)


@pytest.mark.parametrize("case", fr.fused_small_cases(), ids=fr.fid)
def test_fused_small_and_no_inner_step(ctx, case):
    _fused_case(ctx, case)


@pytest.mark.parametrize("top,stays", [(2.0 ** 24, True), (2.0 ** 24 + 1, False)])
def test_fused_counts_at_the_f32_limit(ctx, top, stays):
    """A count of exactly 2^24 survives the f32 tile and stays on the fused kernel; 2^24 + 1 does not and must leave it."""
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    c = fr.FCase(53, 8, 5, 2, 20, 2, False, "")
    V, D, Rt = fr.fused_inputs(c)
    D[7, 3] = top
    V[7, 3] = 0.5
    u0, a0, wu, wa = fr.solver_oracle(V, D, Rt, c.n_u, c.T1, c.n_iter2)
    with _at_level(ctx, 4), Problem(ctx, V, D, Rt) as p, Solver(p, u0, a0, L.DMF_MODE_PARTIAL) as s:
        text = s.u_phase_describe(c.n_iter2)
        if stays:
            assert text == fr.fused_text(c.N, c.S, c.n_c, c.n_u, c.n_iter2)
        else:
            assert text.startswith("k_u_phase_mfma<2,2,vec> one-launch ") and "fused" not in s.describe(c.n_iter2)
        s.step(c.T1, c.n_iter2, 0.0)
        u, alpha, _, _ = s.get()
    dev = max(float(np.abs(alpha - wa).max()), float(np.abs(u - wu).max()))
    print(f"DEV {'fused' if stays else 'mfma'} tight {dev:.3e} count-{top:.0f}")
    assert np.abs(alpha - wa).max() < fr.TIGHT and np.abs(u - wu).max() < fr.TIGHT


# ------------------------------------------------------------------------------------------------ the loop's own Gram
def _check_last_gram(name, c, d, gb, u_now):
    """The u-dependent rows of a packed Gram for the iterate u_now: equality on the dyadic family (every product and
    partial sum representable), else the derived bound (N + 4) 2^-53 sum |term| of tests/test_gpu_gram_exact.py."""
    from test_gpu_gram_exact import _check_bound, _report, _rows

    K, feats = c.n_c + c.n_u, ge.solver_features(c.n_c, c.n_u)
    got, got_b = gb[_rows(feats)], gb[[ge.tri(c.n_c + j, K) for j in range(c.n_u)]]
    if c.family == "dyadic":
        assert np.array_equal(u_now, d.u)   # (no inner step ran: the iterate is still the dyadic u0)
        assert _report(f"{name} cross/uu", got, ge.dyadic_gram(d, feats))
        assert _report(f"{name} b_u", got_b, ge.dyadic_rhs(d)[0][c.n_c:])
    else:
        X = np.hstack([d.Rt, u_now]) if c.n_c else u_now
        _check_bound(f"{name} cross/uu", got, [X[:, [k for k, _ in feats]], X[:, [l for _, l in feats]]], [d.D], c.N)
        _check_bound(f"{name} b_u", got_b, [u_now], [d.D, d.V], c.N)


@pytest.mark.parametrize("case", fr.FUSED_GRAM, ids=fr.gid)
def test_fused_gram_is_exact(ctx, case):
    """The Gram of phase C, read back as the step left it.  Summation of phase C: a C wave adds its 8 rows of every block
    of its workgroup into one register per entry -- t = d u_j (one rounding), then one FMA per term (the product is not
    rounded) -- the two halves of a workgroup go to two slab rows, the tail's k_gram_u adds its slab rows, and
    k_gram_reduce adds the slabs in fixed order: N terms with at most one rounding each and N - 1 rounded additions of
    non-negative partial sums in SOME order, which is what the bound (N + 4) 2^-53 sum |term| was derived for; no other
    constant is needed.  On the dyadic family every such sum is exact, so the entries must be EQUAL."""
    from demethify_amd.device import Problem, Solver

    c = case
    d = ge.make(c.family, c.N, c.S, c.n_c, c.n_u, c.nd, seed=7 + c.N % 1000 + c.S)
    K = c.n_c + c.n_u
    with _at_level(ctx, 4), Problem(ctx, d.V, d.D, d.Rt) as p, Solver(p, d.u, np.full((K, c.S), 1.0 / K)) as s:
        assert s.u_phase_describe(c.n_iter2) == fr.fused_text(c.N, c.S, c.n_c, c.n_u, c.n_iter2)
        before, text0 = s.gram("last")
        assert text0 == "" and not before[[ge.tri(k, l) for k, l in ge.solver_features(c.n_c, c.n_u)]].any()
        s.step(1, c.n_iter2, 0.0)
        gb, text = s.gram("last")
        u_now = s.get()[0]
        again = s.gram("last")[0]
        gk = p.gram_known()[0] if c.n_c else None
    slabs = 2 * fr.fused_grid(c.N - c.N % 16, c.S)
    assert text == f"k_rowpass_fused<{(c.n_c + 3) // 4},{c.n_u}> phase C slabs={slabs}" + (" + k_gram_u tail" if c.N % 16 else "")
    assert np.array_equal(gb, again)
    _check_last_gram(f"fused {fr.gid(c)}", c, d, gb, u_now)
    for l in range(c.n_c):   # the known block is the problem's
        for k in range(l + 1):
            assert np.array_equal(gb[ge.tri(k, l)], gk[ge.tri(k, l)])


@pytest.mark.parametrize("family,n_iter2", [("dyadic", 0), ("full", 2)])
def test_last_gram_on_the_k_gram_u_route(ctx, family, n_iter2):
    """The accessor against a route that is exact-tested already: at level 3 the loop's Gram comes from k_gram_u; what the
    step left must be what Solver.gram("fp64") computes now for the same u, bit for bit, and hold the same checks."""
    from demethify_amd.device import Problem, Solver

    c = fr.GCase(family, 77, 13, 2, 3, 2, n_iter2, "")
    d = ge.make(family, c.N, c.S, c.n_c, c.n_u, c.nd, seed=11)
    with _at_level(ctx, 3), Problem(ctx, d.V, d.D, d.Rt) as p, Solver(p, d.u, np.full((5, c.S), 0.2)) as s:
        assert " gram=k_gram_u " in s.describe(n_iter2)
        s.step(1, n_iter2, 0.0)
        gb, text = s.gram("last")
        u_now = s.get()[0]
        now, text_now = s.gram("fp64")
        after = s.gram("last")[0]
    assert text.startswith("k_gram_u<4,3>") and text == text_now
    assert np.array_equal(gb, now) and np.array_equal(after, now)
    _check_last_gram(f"k_gram_u {family}", c, d, gb, u_now)


# ------------------------------------------------------------------------------------------------ bit-stability
REPEATS = 10


@pytest.mark.parametrize("case", fr.fused_wrap_cases()[1:], ids=fr.fid)   # one per column-group count
def test_fused_multi_block_launches_give_the_same_bits(ctx, case):
    """Workgroups that run three blocks, ten times: a barrier missing between the teams (tile buffer s & 1, the u rows a C
    wave stores one step late) shows up as different bits between repetitions -- every sum is in fixed order."""
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    c = case
    V, D, Rt = fr.fused_inputs(c, seed=5)
    rs = np.random.RandomState(4)
    u0, a0 = rs.uniform(size=(c.N, c.n_u)), rs.dirichlet(np.ones(c.n_c + c.n_u), c.S).T.copy()
    mode = L.DMF_MODE_PARTIAL if c.n_c else L.DMF_MODE_UNSUPERVISED
    first = None
    with _at_level(ctx, 4), Problem(ctx, V, D, Rt) as p:
        for rep in range(REPEATS):
            with Solver(p, u0, a0, mode) as s:
                assert s.u_phase_describe(c.n_iter2) == fr.fused_text(c.N, c.S, c.n_c, c.n_u, c.n_iter2)
                s.step(2, c.n_iter2, 0.0)
                got = s.get()[:3] + (s.gram("last")[0],)
            if first is None:
                first = got
            else:
                assert got[2] == first[2], rep
                for a, b in zip(got[:2] + got[3:], first[:2] + first[3:]):
                    np.testing.assert_array_equal(a, b, err_msg=f"repetition {rep}")


def test_mfma_split_multi_block_launch_gives_the_same_bits(ctx):
    from demethify_amd.device import Problem

    c = [w for w in fr.wrap_cases() if w.kernel == "mfma" and " split " in fr.expected_text(w) and "d16" in fr.expected_text(w)][0]
    V, D, Rt, u, u_prev, alpha, a1, lwp, lw = _inputs(c)
    first = None
    with _at_level(ctx, c.level), Problem(ctx, V, D, Rt) as p:
        for rep in range(REPEATS):
            got = p.update_u(u, u_prev, alpha, c.n_iter2, a1, lwp, lw)[:2]
            if first is None:
                first = got
            else:
                np.testing.assert_array_equal(got[0], first[0], err_msg=f"repetition {rep}")
                np.testing.assert_array_equal(got[1], first[1], err_msg=f"repetition {rep}")
