"""The frozen iterate behind the stop test |cf - cf_0| < tol (deconvolution.py:218-220) on every kernel path of the solver's
loop, at shapes that take milliseconds (the table and the oracle's side: tests/stop_cases.py, proved on the CPU by
tests/test_stop_cases_host.py).

dmf_solver_step runs ahead of the device: it enqueues 8 outer iterations, then 16, and reads the state back between the
batches only, so every kernel of an iteration enqueued behind the stop -- or behind a pause inside the confirmation band --
must do nothing.  A kernel that misses the check leaves an iterate up to 63 iterations past the reference's stop: an error
of the order of the step size.  Per case, each leg on a fresh solver of one Problem:

  A  fixed work: step(k, n_iter2, 0.0), twice -- the two runs must agree bit for bit (no path may need an exemption: no
     floating-point atomics, slabs summed in a fixed order), and they are what the legs below are compared with
  B  step(24, n_iter2, tol) without confirmation: stops at k -- the oracle's stop -- with 24 - k no-op iterations enqueued
     behind it; u, alpha and cost at the oracle's bars (1e-8, 1e-9 relative); the whole device state bit-identical to A's:
     u, alpha, u_prev, alpha_prev, the packed Gram, a1, a2, l_w, l_w_prev, l_h, l_h_prev, u_norm2, cf, cf_prev, iters;
     a further step(5) changes nothing
  C  the same with the confirmation forced: pauses where tests/stop_cases.py's model of the loop says, decided on
     streaming costs where it says; the final state bit-identical to B's
  D  k_u_step_direct only, which has no done check and is safe because its loop reads the state after every iteration:
     a further step(3) launches nothing -- u, u_prev and the host's buffer roles stay where they are.

Measured on an MI355X over the 17 cases (per case: DESIGN.md section 6): largest max|u - oracle| 1.5e-13 and
max|alpha - oracle| 1.5e-14 (09-split-51-ints), cost 7.2e-15 relative (15-purity-general); every bit comparison holds on
every path.  With one done check removed on a scratch copy, cases failing: k_alpha_phase_row16 10 (all that run it),
k_u_inner_rows 3 (all that run it behind a solver that runs ahead: u off by 0.06 .. 0.20), the done_flag test of k_gram_u 0
-- that kernel writes only the slab, which behind a stop the guarded reduce never reads and which it refills with the
values already there: the check saves time, and no comparison of states can see it."""
import numpy as np
import pytest

import stop_cases as sc

pytestmark = pytest.mark.gpu

SCALARS = ("a1", "a2", "l_w", "l_w_prev", "l_h", "l_h_prev", "u_norm2", "cf", "cf_prev", "iters")
ARRAYS = ("u", "alpha", "u_prev", "alpha_prev", "gb")


def _state(s):
    """Everything of the solver's device state that an outer iteration writes, as fresh host copies."""
    u, alpha, cost, iters = s.get()
    m = s.momentum_state()
    gb, _ = s.gram("last")
    out = {"u": u, "alpha": alpha, "u_prev": m["u_prev"], "alpha_prev": m["alpha_prev"], "gb": gb, "cost": cost,
           "done": m["done"]}
    out.update({name: m[name] for name in SCALARS})
    assert iters == m["iters"] and cost == m["cf"]
    return out


def _same_bits(name, got, want):
    for key in ARRAYS:
        assert np.array_equal(got[key], want[key]), (name, key, float(np.abs(got[key] - want[key]).max()))
    for key in SCALARS:   # (bit patterns: a NaN equals itself)
        assert np.float64(got[key]).tobytes() == np.float64(want[key]).tobytes(), (name, key, got[key], want[key])


def _solver(problem, c, i):
    from demethify_amd import _lib as L
    from demethify_amd.device import Solver

    s = Solver(problem, i.u0, i.a0, L.DMF_MODE_PARTIAL if c.n_c else L.DMF_MODE_UNSUPERVISED)
    if c.purity:
        s.set_purity(i.purity)
    return s


def _legs(ctx, c, problem, record_property):
    i, a = sc.inputs(c), sc.analyse(c)
    k, tol, t2 = c.k, a.tol, c.n_iter2

    # ---- leg A: fixed work, twice
    fixed = []
    for _ in range(2):
        with _solver(problem, c, i) as s:
            desc = s.describe(t2)
            assert sc.kinds(desc) == (c.row, c.gram, c.alpha), (c.name, desc)
            for token in c.extra:
                assert token in desc, (c.name, token, desc)
            assert s.step(k, t2, 0.0) == (k, False)
            fixed.append(_state(s))
    _same_bits(f"{c.name}: fixed work, run to run", fixed[1], fixed[0])
    want = fixed[0]
    assert want["iters"] == k and want["done"] == 0

    # ---- leg B: the stop, with launches behind it
    ctx.set_stop_confirmation(2)
    with _solver(problem, c, i) as s:
        it, converged = s.step(sc.TRACE, t2, tol)
        info = s.stop_info()
        stopped = _state(s)
        du, da = float(np.abs(stopped["u"] - a.u).max()), float(np.abs(stopped["alpha"] - a.alpha).max())
        dc = abs(stopped["cost"] - a.cost) / a.cost
        print(f"stop {c.name}: k {k} tol {tol:.6g} margin {a.margin:.3f}  max|u - oracle| {du:.3e}  max|alpha - oracle| "
              f"{da:.3e}  cost rel {dc:.3e}  stopped at {it}")
        for key, v in (("oracle_du", du), ("oracle_da", da), ("oracle_cost_rel", dc)):
            record_property(key, v)
        assert converged and it == k == a.stop
        assert not info["confirm_stops"] and info["n_confirmed"] == 0 and info["n_unconfirmed"] == 0
        assert du <= sc.TIGHT and da <= sc.TIGHT
        assert stopped["cost"] == pytest.approx(a.cost, rel=sc.COST_RTOL)
        assert stopped["done"] == 1
        _same_bits(f"{c.name}: stop against fixed work", stopped, want)
        assert s.step(5, t2, tol) == (k, True)
        again = _state(s)
        assert again["done"] == 1
        _same_bits(f"{c.name}: a further step()", again, want)
        if c.row == sc.DIRECT:
            # ---- leg D: k_u_step_direct has no done check of its own.  Were its launches enqueued behind a stop, u would
            # move and the host's rotation of u / u_prev / u_next would name other buffers: get() and momentum_state()
            # read through those roles.
            assert s.step(3, t2, tol) == (k, True)
            after = _state(s)
            assert after["iters"] == k and after["done"] == 1
            assert np.array_equal(after["u"], want["u"]) and np.array_equal(after["u_prev"], want["u_prev"])
            _same_bits(f"{c.name}: step(3) behind the stop", after, want)
            assert sc.kinds(s.describe(t2))[0] == sc.DIRECT

    # ---- leg C: pause and resume
    ctx.set_stop_confirmation(1)
    with _solver(problem, c, i) as s:
        it, converged = s.step(sc.TRACE, t2, tol)
        info = s.stop_info()
        direct = s.direct_cost()
        resumed = _state(s)
        print(f"stop {c.name}: confirmation forced: stopped at {it}, {info}, model pauses {a.pauses}")
        assert converged and it == k
        assert info["confirm_stops"]
        assert (info["n_confirmed"], info["n_unconfirmed"]) == (a.n_confirmed, a.n_unconfirmed)
        assert info["last_stream_cost"] == direct
        assert resumed["done"] == 1
        _same_bits(f"{c.name}: pause and resume against the plain stop", resumed, stopped)


@pytest.mark.parametrize("c", sc.CASES, ids=sc.IDS)
def test_iterate_is_frozen_behind_the_stop(ctx, record_property, c):
    from demethify_amd.device import Problem

    i = sc.inputs(c)
    ctx.set_generic(c.level)
    ctx.set_x16(c.x16)
    try:
        with Problem(ctx, i.V, i.D, i.Rt) as parent:
            if c.masked:
                with parent.masked(i.mask) as derived:
                    _legs(ctx, c, derived, record_property)
            else:
                _legs(ctx, c, parent, record_property)
    finally:
        ctx.set_generic(0)
        ctx.set_x16(True)
        ctx.set_stop_confirmation(0)
