"""The momentum cap beta = min((a_prev - 1) / a_next, 0.9999 sqrt(l_prev / l_cur)) and the default alpha phase on every path
that forms them, against references in np.longdouble.  The tables, data and references live in tests/momentum_ref.py;
tests/test_momentum_host.py proves without a GPU that they reach every alpha kernel instance and branch and that the cap
decides the result of every case that claims it.

Leg A  one alpha phase through Problem.update_alpha on k_alpha_phase_row16, k_alpha_phase_lanes<32|64>, k_alpha_phase<4|8|16>
       and k_alpha_phase_dyn, under the scalar states QUIET, SQRT (cap on the first step) and FLAT (cap on every step).
Leg B  one u phase through Problem.update_u on every stand-alone route under SQRT and FLAT.
Leg C  whole outer iterations from a cold start that engages the caps, one step(1, ...) at a time, every phase and every
       scalar of the momentum state (Solver.momentum_state) checked against the state read before the step.
Leg D  the momentum rows of dmf_solver_step: batches, a stop test that cannot fire, rows switched on, off and on.

Bars.  alpha: 16 * max(noise, steps * 2^-53), noise = what the float64 references (the same phase in float64 on the float64
Gram, and oracle.solver.alpha_phase) deviate from the np.longdouble one -- measured on references alone, never on the GPU.
u: the project's 1e-11 for one phase.  Every case prints "DEV <kernel> <deviation> <bar> <deviation / bar>" before it asserts
and records the quotient (record_property).

Measured on an MI355X (worst deviation / bar per kernel over Leg A; a bar is 16 x the references' own noise, so 0.11 means
the kernel sits 1.8 x that noise from the np.longdouble reference):
  k_alpha_phase_row16 0.109   k_alpha_phase_lanes<32> 0.044   k_alpha_phase_lanes<64> 0.052   k_alpha_phase<4> 0.061
  k_alpha_phase<8> 0.075      k_alpha_phase<16> 0.098         k_alpha_phase_dyn 0.059
Leg B: 1.8e-15 at worst against the bar of 1e-11.  Leg C: alpha 0.096 of its bar, u 5.0e-12 (case a, one inner step: beta is
large against a u that has barely moved), cf 0.012 of its derived bound, closing agreement 7.2e-12 against 1e-8.
Smallest cap effect per leg (what dropping the cap changes in the reference; tests/test_momentum_host.py): Leg A 2.3e-6,
Leg B 8.3e-5 (FLAT) and 0.14 (SQRT), Legs C and D 1.0e-2 on u and 4.0e-3 on alpha."""
import functools

import numpy as np
import pytest

import fp64_rowpass as fr
import momentum_ref as mr
from oracle import solver as osol

pytestmark = pytest.mark.gpu


def _at_level(ctx, level, x16=True):
    class Scope:
        def __enter__(self):
            self.before = ctx.generic_level
            ctx.set_generic(level)
            ctx.set_x16(x16)

        def __exit__(self, *exc):
            ctx.set_generic(self.before)
            ctx.set_x16(True)

    return Scope()


def _advance(a, n):
    for _ in range(n):
        a = (1 + np.sqrt(1 + 4 * a * a)) / 2
    return a


# ------------------------------------------------------------------------------------------------ Leg A
@pytest.mark.parametrize("case", mr.alpha_cases(), ids=mr.aid)
def test_alpha_phase_on_every_path(ctx, case, record_property):
    from demethify_amd.device import Problem, Solver

    c, K, n = case, case.n_c + case.n_u, case.n_iter2
    V, D, Rt, u, alpha, alpha_prev, a2, lhp, lh = mr.alpha_inputs(c)
    ref, ref_prev, bar, noise, _ = mr.alpha_refs(c)
    with _at_level(ctx, c.level), Problem(ctx, V, D, Rt) as p:
        got = p.update_alpha(u, alpha, alpha_prev, n, a2, lhp, lh)
        with Solver(p, u, alpha) as s:
            path = s.describe(n)
    assert path.endswith(" alpha=" + mr.described_as(c.kernel)) and mr.kernel_of(K, c.level) == c.kernel, path
    dev = max(float(np.abs(got[0] - ref).max()), float(np.abs(got[1] - ref_prev).max()))
    print(f"DEV {c.kernel} {dev:.3e} {bar:.3e} {dev / bar:.3f} noise {noise:.2e} {mr.aid(c)}")
    record_property("dev_over_bar", dev / bar)
    assert dev <= bar
    # the simplex: no negative entry, columns sum to 1
    assert (got[0] >= 0.0).all()
    if n > 0:
        assert np.abs(got[0].sum(axis=0) - 1.0).max() <= K * 2.0 ** -52
    if n == 1:
        assert np.array_equal(got[1], alpha)
    if n == 0:
        assert np.array_equal(got[0], alpha) and np.array_equal(got[1], alpha_prev)
    # the returned scalars, as tests/test_gpu_kat.py asserts them
    assert got[2] == pytest.approx(_advance(a2, n), rel=1e-15) and got[3] == (lh if n > 0 else lhp)


# ------------------------------------------------------------------------------------------------ Leg B
@functools.lru_cache(maxsize=2)
def _u_inputs(c):
    return fr.update_u_inputs(c)


@pytest.mark.parametrize("state", ["SQRT", "FLAT"])
@pytest.mark.parametrize("name,case", mr.u_cases(), ids=[f"{n.split(' ')[0]}-{c.n_c}+{c.n_u}" + ("-split" if "split" in n else "")
                                                         for n, c in mr.u_cases()])
def test_u_phase_under_the_cap(ctx, name, case, state):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    c = case
    V, D, Rt, u, u_prev, alpha, _, _, l_w = _u_inputs(c)
    a1, lwp, lw = mr.u_state(l_w, state)
    assert mr.cap_steps(a1, lwp, lw, c.n_iter2)
    with _at_level(ctx, c.level), Problem(ctx, V, D, Rt) as p:
        with Solver(p, u, alpha) as s:
            assert s.u_phase_describe(c.n_iter2, "update_u").startswith(name + " ")
        for unsup in (False, True):
            wu, wup = fr.update_u_oracle(c, unsup, V, D, Rt, u, u_prev, alpha, a1, lwp, lw)
            got = p.update_u(u, u_prev, alpha, c.n_iter2, a1, lwp, lw,
                             mode=L.DMF_MODE_UNSUPERVISED if unsup else L.DMF_MODE_PARTIAL)
            dev = max(float(np.abs(got[0] - wu).max()), float(np.abs(got[1] - wup).max()))
            print(f"DEV {name.split(' ')[0]} {state}{' unsup' if unsup else ''} {dev:.3e}")
            assert dev < mr.KAT
            assert got[0].min() >= 0.0 and got[0].max() <= 1.0
            assert got[2] == pytest.approx(_advance(a1, c.n_iter2), rel=1e-15) and got[3] == lw


# ------------------------------------------------------------------------------------------------ Leg C
def _read(s):
    u, alpha, _, it = s.get()
    st = s.momentum_state()
    assert st["iters"] == it
    st["u"], st["alpha"] = u, alpha
    return st


def _open(ctx, c, stack):
    """(problem, solver) of a cold-start case inside `stack` (an ExitStack), at the case's level, on the path it names."""
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    V, D, Rt, u0, a0 = mr.cold_inputs(c)
    stack.enter_context(_at_level(ctx, c.level, c.x16))
    p = stack.enter_context(Problem(ctx, V, D, Rt))
    s = stack.enter_context(Solver(p, u0, a0, L.DMF_MODE_PARTIAL if c.n_c else L.DMF_MODE_UNSUPERVISED))
    return p, s


def _check_path(c, s, n):
    path = s.describe(n)
    assert path.endswith(" alpha=" + c.alpha), path
    if n == c.n_iter2:
        assert f"rowpass={c.row} " in path, path


def _check_step(c, before, after, gb, n, inner_total, u_its, alpha_its):
    """One outer iteration of n inner steps: `after` against what the references make of `before`.

    In-loop cost.  cf = sum_s vDv_s - 2 a_s . b_s + a_s^T G_s a_s on the Gram the iteration left (read back, so its own
    rounding is not in the bound).  With every term's absolute value in M = sum_s (vDv_s + 2 sum_k a_k |b_ks| +
    sum_kl a_k a_l |G_kls|), a chain of n fused multiply-adds is off by at most n 2^-53 times the absolute sum: K terms for
    G a, one product and the row's sum (1 + 4) for the quadratic form, K for a . b (inside the same bound), three roundings
    for cost - 2 lin + quad: K + 8 per sample; then the wave sum (6), the workgroup partials (a strided loop of at most two
    terms here, 2) and the closing wave sum (6): |cf - cost_ref| <= (K + 22) 2^-53 M (momentum_ref.cost_factor)."""
    V, D, Rt, _, _ = mr.cold_inputs(c)
    K, it = c.n_c + c.n_u, after["iters"]
    # ---- u phase
    wu, wup = mr.u_phase_oracle(c, before["u"], before["u_prev"], before["alpha"], before["a1"], before["l_w_prev"], before["l_w"],
                                V, D, Rt, n)
    dev_u = max(float(np.abs(after["u"] - wu).max()), float(np.abs(after["u_prev"] - wup).max()))
    # ---- alpha phase, from the GPU's own Gram
    args = (before["alpha"], before["alpha_prev"], before["a2"], before["l_h_prev"], after["l_h"], n)
    ref = mr.alpha_phase_ref(gb, *args, mr.LD)
    R = np.c_[Rt, after["u"]] if Rt is not None else after["u"]
    orc = osol.alpha_phase(n, before["alpha"], before["a2"], before["l_h_prev"], after["l_h"], before["alpha_prev"], R, D, V,
                           project=osol.simplex_project_columns_fast)
    noise = max(mr.phase_noise(gb, *args, ref), float(np.abs(orc[0] - ref[0]).max()), float(np.abs(orc[1] - ref[1]).max()))
    bar = mr.alpha_bar(noise, n)
    dev_a = max(float(np.abs(after["alpha"] - ref[0]).max()), float(np.abs(after["alpha_prev"] - ref[1]).max()))
    # ---- cost
    want_cf, mag = mr.cost_ref(gb, after["alpha"])
    cf_bound = mr.cost_factor(K, c.S) * mr.EPS * mag
    print(f"STEP {mr.cid(c)} it {it} n {n}: u {dev_u:.2e}  alpha {dev_a:.2e} bar {bar:.2e} ({dev_a / bar:.3f})  "
          f"cf {abs(after['cf'] - want_cf):.2e} bound {cf_bound:.2e}")
    assert dev_u <= mr.KAT
    assert dev_a <= bar
    assert abs(after["cf"] - want_cf) <= cf_bound
    # ---- scalars
    assert after["l_h"] == (after["rt_norm2"] + after["u_norm2"]) * after["dsq"]
    u2 = float((after["u"].astype(mr.LD) ** 2).sum())
    assert abs(after["u_norm2"] - u2) <= (c.N * c.n_u + 8) * mr.EPS * u2
    lw = float((after["alpha"][c.n_c:].astype(mr.LD) ** 2).sum()) * after["dsq"]
    assert abs(after["l_w"] - lw) <= (c.n_u * c.S + 8) * mr.EPS * lw
    assert after["dsq"] == float(D.max()) ** 2
    assert after["l_w_prev"] == before["l_w"]
    assert before["l_h_prev"] == before["l_h"] and after["l_h_prev"] == after["l_h"]   # (handed over behind the phase)
    assert after["cf_prev"] == before["cf"]
    assert after["iters"] == before["iters"] + 1 and after["arrive"] == 0 and after["done"] == 0
    # ---- momentum recurrence: bit for bit where the host ran it ahead (plain IEEE arithmetic), else to the chain's rounding
    rows = mr.uses_rows(c, n)
    assert (after["mom_n"] == n) == rows
    for name in ("a1", "a2"):
        want = _advance(before[name], n)
        if rows:
            assert after[name] == want
        else:
            assert abs(after[name] - want) <= inner_total * 2.0 ** -52 * want
    # ---- the caps are active exactly where the host test found them on the oracle's trajectory
    assert bool(mr.cap_steps(before["a1"], before["l_w_prev"], before["l_w"], n)) == (it in u_its)
    assert bool(mr.cap_steps(before["a2"], before["l_h_prev"], after["l_h"], n)) == (it in alpha_its)


def _run_trail(ctx, c, trail):
    """The cold-start case one step(1, n, 0.0) at a time over the inner-step counts `trail`, every iteration checked
    -> the final state."""
    from contextlib import ExitStack

    u_its, alpha_its = mr.cap_iterations(c, None if trail == (c.n_iter2,) * mr.T1 else trail)
    with ExitStack() as stack:
        _, s = _open(ctx, c, stack)
        state, inner = _read(s), 0
        assert state["iters"] == 0 and state["a1"] == 1.0 and state["a2"] == 1.0
        for n in trail:
            _check_path(c, s, n)
            assert s.step(1, n, 0.0) == (state["iters"] + 1, False)
            gb, _ = s.gram("last")
            after = _read(s)
            inner += n
            _check_step(c, state, after, gb, n, inner, u_its, alpha_its)
            state = after
    return state


@pytest.mark.parametrize("case", mr.COLD, ids=mr.cid)
def test_outer_iterations_from_the_cold_start(ctx, case):
    c = case
    last = _run_trail(ctx, c, (c.n_iter2,) * mr.T1)
    _, wu, wa = mr.cold_trajectory(c)
    dev = max(float(np.abs(last["u"] - wu).max()), float(np.abs(last["alpha"] - wa).max()))
    print(f"CLOSE {mr.cid(c)} {dev:.3e}")
    assert dev <= mr.TIGHT


# ------------------------------------------------------------------------------------------------ Leg D
# what the trails are compared on, bit for bit: the iterate and every scalar and array of the momentum state but mom_i, the
# index of the current row inside the last upload (bookkeeping of how the steps were batched)
def _same(x, y):
    return all(np.array_equal(x[k], y[k], equal_nan=True) for k in x if k != "mom_i") and x.keys() == y.keys()


def _trail(ctx, c, calls, touch=False):
    """The state after step(n_outer, n_iter2, tol) for each of `calls`; touch: the accessor is called between the steps."""
    from contextlib import ExitStack

    with ExitStack() as stack:
        _, s = _open(ctx, c, stack)
        for n_outer, n_iter2, tol in calls:
            s.step(n_outer, n_iter2, tol)
            if touch:
                s.momentum_state()
                s.momentum_state(arrays=False)
        return _read(s)


def test_momentum_rows_one_call_and_seventy(ctx):
    """step(70, 2, 0) uploads 64 rows and then 6; seventy calls upload one row each."""
    one = _trail(ctx, mr.LEG_D, [(70, 2, 0.0)])
    many = _trail(ctx, mr.LEG_D, [(1, 2, 0.0)] * 70)
    assert one["iters"] == 70 and one["mom_n"] == 2 and one["mom_i"] == 6 and many["mom_i"] == 1
    assert _same(one, many)


def test_momentum_rows_under_a_stop_test_that_cannot_fire(ctx):
    """tol = 1e-300 reads the state back after 8, 16 and 6 iterations; tol = 0 enqueues all thirty at once."""
    a = _trail(ctx, mr.LEG_D, [(30, 20, 1e-300)])
    b = _trail(ctx, mr.LEG_D, [(30, 20, 0.0)])
    assert a["iters"] == 30 and a["done"] == 0 and a["mom_i"] == 6 and b["mom_i"] == 30
    assert _same(a, b)


def test_momentum_rows_on_off_and_on(ctx):
    c = mr.LEG_D
    batched = _trail(ctx, c, [(2, 20, 0.0), (1, 51, 0.0), (2, 20, 0.0)])
    single = _run_trail(ctx, c, mr.LEG_D_TRAIL)
    assert batched["iters"] == 5 and _same(batched, single)


# ------------------------------------------------------------------------------------------------ the accessor
@pytest.mark.parametrize("case", [mr.LEG_D, mr.COLD[11]], ids=mr.cid)
def test_momentum_state_changes_nothing(ctx, case):
    """A trail of step(1, ...) calls with the accessor called in between equals the trail without it, bit for bit (on the
    momentum rows, and at level 2, where the u phase rotates three buffers)."""
    calls = [(1, case.n_iter2, 0.0)] * 4
    assert _same(_trail(ctx, case, calls, touch=True), _trail(ctx, case, calls))


def test_momentum_state_arguments(ctx):
    import ctypes as C
    from contextlib import ExitStack

    from demethify_amd import _lib as L

    lib = L.load()
    sc = (C.c_double * len(L.MOMENTUM_SCALARS))()
    assert lib.dmf_solver_momentum_state(None, sc, None, None) == L.DMF_ERR_BAD_ARG
    with ExitStack() as stack:
        _, s = _open(ctx, mr.LEG_D, stack)
        assert lib.dmf_solver_momentum_state(s._h, None, None, None) == L.DMF_ERR_BAD_ARG
        V, D, Rt, u0, a0 = mr.cold_inputs(mr.LEG_D)
        st = s.momentum_state()
        assert set(st) == set(L.MOMENTUM_SCALARS) | {"alpha_prev", "u_prev"} and len(L.MOMENTUM_SCALARS) == 16
        assert np.array_equal(st["u_prev"], u0) and np.array_equal(st["alpha_prev"], a0)   # (deconvolution.py:194-195)
        assert (st["a1"], st["a2"], st["iters"], st["done"], st["arrive"]) == (1.0, 1.0, 0, 0, 0)
        assert st["l_w"] == st["l_w_prev"] and st["l_h"] == st["l_h_prev"] and st["dsq"] == float(D.max()) ** 2
        assert st["rt_norm2"] == pytest.approx(np.linalg.norm(Rt) ** 2, rel=1e-13)
        assert set(s.momentum_state(arrays=False)) == set(L.MOMENTUM_SCALARS)
