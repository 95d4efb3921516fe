"""Without a GPU: the tables of tests/momentum_ref.py do what tests/test_gpu_momentum.py relies on.  Every case describes
(dmf_select_describe, dmf_u_phase_describe) as the kernels it names; the alpha cases reach every instance, every side of the
K > 2 / 4 / 8 / 12 branches, every sample count, scalar state and step count the issue lists; and wherever a case claims the
cap, the cap decides: dropping it changes the reference by at least 1e-6 and the two arguments of the min are not near a tie.

Smallest cap effects measured here (np.longdouble references for alpha, the float64 oracle for u): Leg A 2.3e-6, Leg B
8.3e-5 under FLAT and 0.14 under SQRT, Legs C and D 1.0e-2 on u and 4.0e-3 on alpha (each test prints its own).

One bound differs from the plan this file was written to: under FLAT (l_prev = l) the ratio is below 1 and the cap is 0.9999,
so the two arguments of the min can never be 1e-3 apart; FLAT cases are held to momentum_ref.FLAT_GAP = 4e-5 (a = 3e4 leaves
5e-5, eleven orders above rounding), every other decision -- SQRT and all cold-start steps, engaged or not -- to 1e-3."""
from collections import defaultdict

import numpy as np
import pytest

import fp64_rowpass as fr
import momentum_ref as mr
from oracle import solver as osol


# ------------------------------------------------------------------------------------------------ kernel names
def test_alpha_cases_describe_as_the_kernels_they_name():
    for c in mr.alpha_cases():
        K = c.n_c + c.n_u
        assert mr.kernel_of(K, c.level) == c.kernel, mr.aid(c)
        text = mr.select_describe(c.N, c.S, c.n_c, c.n_u, c.level, c.n_iter2)
        assert text is not None and text.endswith(" alpha=" + mr.described_as(c.kernel)), (mr.aid(c), text)
        assert 64 <= c.N <= 200


def test_u_cases_describe_as_the_routes_they_name():
    names = [name for name, _ in mr.u_cases()]
    for want in ("k_u_phase_mfma<1,3,vec> one-launch", "k_u_phase_mfma<0,7,vec> split", "k_u_phase_mfma<1,3,vec,d16> one-launch",
                 "k_u_phase_big", "k_u_phase_gram", "k_u_step_direct"):
        assert sum(n.startswith(want) for n in names) == 1
    assert sorted(c.n_u for n, c in mr.u_cases() if n.startswith("k_cm_i8")) == [5, 12, 20]
    for name, c in mr.u_cases():
        text = fr.describe(c)
        assert text is not None and text.startswith(name + " "), (name, text)
        assert c.n_iter2 == mr.UCAP_STEPS == fr.KAT_STEPS


def test_cold_cases_describe_as_the_paths_they_name():
    assert [c.name for c in mr.COLD[:12]] == ["a1", "a20", "a50", "b", "c", "d", "e", "f", "g", "h", "i", "j"]
    for c in mr.COLD + [mr.LEG_D]:
        text = mr.select_describe(c.N, c.S, c.n_c, c.n_u, c.level, c.n_iter2, x16=c.x16)
        assert text is not None and f"rowpass={c.row} " in text and text.endswith(" alpha=" + c.alpha), (mr.cid(c), text)
        assert (" x16 " in text) == (c.x16 and c.row.startswith("k_rowpass_v2"))
        assert c.N <= 300 and c.S <= 70
    by = {c.name: c for c in mr.COLD}
    assert (by["c"].n_c, by["c"].n_u) == (16, 2) and by["e"].n_u == 6 and by["f"].n_c == 0 and by["d"].n_iter2 == 51
    # the momentum rows: k_rowpass_v2 with k_alpha_phase_row16 up to 64 inner steps -- (a), (b), (f); not (c), not (d)
    assert [c.name for c in mr.COLD[:12] if mr.uses_rows(c, c.n_iter2)] == ["a1", "a20", "a50", "b", "f"]
    # Leg D's third trail switches them on, off and on
    assert [mr.uses_rows(mr.LEG_D, n) for n in mr.LEG_D_TRAIL] == [True, True, False, True, True]


# ------------------------------------------------------------------------------------------------ instance coverage
def test_alpha_cases_reach_every_instance_and_branch():
    cases = mr.alpha_cases()
    assert len(cases) == len(set(cases)) == 241 and len(mr.grid_cases()) == 199
    assert len(mr.step_cases()) == 7 * 5 and len(mr.edge_cases()) == 7
    grid = defaultdict(set)
    for c in mr.grid_cases():
        grid[c.kernel, c.level].add((c.n_c + c.n_u, c.n_c, c.S))
    want = {
        ("k_alpha_phase_row16", 0): {(K, n_c, S) for K in mr.ROW16_K for n_c in {0, K // 2} for S in mr.ROW16_S},
        ("k_alpha_phase_lanes<32>", 0): {(K, n_c, S) for K in (17, 24, 32) for n_c in (0, K // 2) for S in (1, 5)},
        ("k_alpha_phase_lanes<64>", 0): {(K, n_c, S) for K in (33, 48, 64) for n_c in (0, K // 2) for S in (1, 3)},
        ("k_alpha_phase<4>", 1): {(K, n_c, S) for K in (1, 2, 4) for n_c in {0, K // 2} for S in mr.PHASE_S},
        ("k_alpha_phase<8>", 1): {(K, n_c, S) for K in (5, 8) for n_c in (0, K // 2) for S in mr.PHASE_S},
        ("k_alpha_phase<16>", 1): {(K, n_c, S) for K in (9, 12, 13, 16) for n_c in (0, K // 2) for S in mr.PHASE_S},
        ("k_alpha_phase_dyn", 1): {(K, n_c, S) for K in mr.DYN_K for n_c in (0, K // 2) for S in mr.DYN_S},
    }
    assert dict(grid) == want
    # both sides of every K > 2 / 4 / 8 / 12 branch, every S % 4, 75 workgroups of k_alpha_phase_row16 (two passes of 64)
    assert {mr.branch_of(K) for K in mr.ROW16_K} == {0, 1, 2, 3, 4}
    for edge in (2, 4, 8, 12):
        assert edge in mr.ROW16_K and edge + 1 in mr.ROW16_K
    assert {S % 4 for S in mr.ROW16_S} == {0, 1, 2, 3} and (max(mr.ROW16_S) + 3) // 4 == 75
    # k_alpha_phase<16> from 13 types on: its 64 Gram columns take more than 48 KB of dynamic LDS
    assert 14 * 15 // 2 * 64 * 8 > 48 * 1024 >= 13 * 14 // 2 * 64 * 8
    # every (kernel, K) sees the three scalar states and 1, 4 and 20 inner steps
    seen = defaultdict(lambda: (set(), set()))
    for c in mr.grid_cases():
        seen[c.kernel, c.n_c + c.n_u][0].add(c.state)
        seen[c.kernel, c.n_c + c.n_u][1].add(c.n_iter2)
    for key, (states, steps) in seen.items():
        assert states == set(mr.STATE_NAMES) and steps == {1, 4, 20}, key
    # every kernel sees 0, 2, 64, 65 and 500 inner steps and the edge data
    for kernel in mr.KERNELS:
        assert {c.n_iter2 for c in mr.step_cases() if c.kernel == kernel} == {0, 2, 64, 65, 500}
        assert sum(c.edges and c.kernel == kernel and c.S >= 5 and c.state != "QUIET" for c in mr.edge_cases()) == 1
    assert all(c.S <= 5 for c in cases if c.n_iter2 >= 500)


def test_edge_data_holds_the_four_edges():
    for c in mr.edge_cases():
        V, D, Rt, u, alpha, alpha_prev, _, _, _ = mr.alpha_inputs(c)
        K = c.n_c + c.n_u
        gb = mr.gram_ref(V, D, Rt, u, np.float64)
        assert not gb[:, 0].any()                                              # a zero-coverage sample: G = 0, b = 0
        assert alpha[K - 1, 1] == 1.0 and alpha[:, 1].sum() == 1.0             # a column on a vertex
        assert (alpha[:, 2] == 1.0 / K).all() and (alpha_prev[:, 2] == alpha[:, 2]).all()
        same = (alpha == alpha_prev).all(axis=0)
        assert same[3::2].all() and not same[4::2].any() and same[3::2].size >= (c.S - 3) // 2


# ------------------------------------------------------------------------------------------------ cap effect
def _gap_ok(ratio, capv, state=None):
    return abs(ratio - capv) >= (mr.FLAT_GAP if state == "FLAT" else mr.CAP_GAP) * capv


def test_the_cap_decides_every_alpha_case_that_claims_it():
    smallest = np.inf
    for c in mr.alpha_cases():
        _, _, _, _, alpha, alpha_prev, a2, lhp, lh = mr.alpha_inputs(c)
        steps = mr.cap_steps(a2, lhp, lh, c.n_iter2)
        if c.state == "QUIET":
            assert not steps, mr.aid(c)
            continue
        assert [t for t, _, _ in steps] == ([0] if c.state == "SQRT" else list(range(c.n_iter2)))[:c.n_iter2], mr.aid(c)
        assert all(_gap_ok(r, v, c.state) for _, r, v in steps), mr.aid(c)
        if c.n_iter2 == 0 or c.n_c + c.n_u == 1:
            continue   # (nothing runs; one type: every projected column is 1, whatever beta)
        ref, ref_prev, _, _, gb = mr.alpha_refs(c)
        free = mr.alpha_phase_ref(gb, alpha, alpha_prev, a2, lhp, lh, c.n_iter2, mr.LD, cap=False)
        effect = max(float(np.abs(free[0] - ref).max()), float(np.abs(free[1] - ref_prev).max()))
        smallest = min(smallest, effect)
        assert effect >= mr.CAP_EFFECT, (mr.aid(c), effect)
    print(f"smallest cap effect, Leg A: {smallest:.2e}")


@pytest.mark.parametrize("state", ["SQRT", "FLAT"])
def test_the_cap_decides_every_u_case(state):
    smallest = np.inf
    for name, c in mr.u_cases():
        V, D, Rt, u, u_prev, alpha, _, _, l_w = fr.update_u_inputs(c)
        a1, lwp, lw = mr.u_state(l_w, state)
        steps = mr.cap_steps(a1, lwp, lw, c.n_iter2)
        assert [t for t, _, _ in steps] == ([0] if state == "SQRT" else list(range(c.n_iter2)))
        assert all(_gap_ok(r, v, state) for _, r, v in steps)
        for unsup in (False, True):
            want = fr.update_u_oracle(c, unsup, V, D, Rt, u, u_prev, alpha, a1, lwp, lw)
            same = mr.u_phase_nocap(c, unsup, V, D, Rt, u, u_prev, alpha, a1, lwp, lw)
            assert np.array_equal(same[0], want[0]) and np.array_equal(same[1], want[1])   # (the loop itself agrees)
            free = mr.u_phase_nocap(c, unsup, V, D, Rt, u, u_prev, alpha, a1, lwp, lw, cap=False)
            effect = float(np.abs(free[0] - want[0]).max())
            smallest = min(smallest, effect)
            assert effect >= mr.CAP_EFFECT, (name, unsup, effect)
    print(f"smallest cap effect, Leg B {state}: {smallest:.2e}")


# ------------------------------------------------------------------------------------------------ cold start
def _cold_checks(c, n_steps=None):
    traj, _, _ = mr.cold_trajectory(c, n_steps)
    u_its, alpha_its = mr.cap_iterations(c, n_steps)
    for rec in traj:
        # no near-tie in any min, whichever way it goes: the GPU recomputes the same decisions from its own scalars
        assert all(_gap_ok(r, v) for _, r, v in rec["u_all"] + rec["alpha_all"]), (mr.cid(c), rec)
        if rec["u_cap"]:
            assert rec["u_effect"] >= mr.CAP_EFFECT
        if rec["alpha_cap"]:
            assert rec["alpha_effect"] >= mr.CAP_EFFECT
    assert traj[0]["u_cap"] == [] and traj[0]["alpha_cap"] == []   # (a = 1: the ratio of the first step is 0)
    return u_its, alpha_its


@pytest.mark.parametrize("case", mr.COLD, ids=mr.cid)
def test_cold_start_engages_the_caps_it_claims(case):
    u_its, alpha_its = _cold_checks(case)
    assert case.u_cap or case.alpha_cap
    assert bool(u_its) == case.u_cap and bool(alpha_its) == case.alpha_cap, (u_its, alpha_its)
    assert all(2 <= i <= mr.T1 for i in u_its + alpha_its)
    print(f"{mr.cid(case)}: u cap in iterations {u_its}, alpha cap in {alpha_its}")


def test_leg_d_trail_engages_the_u_cap():
    u_its, alpha_its = _cold_checks(mr.LEG_D, mr.LEG_D_TRAIL)
    assert u_its and not alpha_its and len(mr.LEG_D_TRAIL) == 5


# ------------------------------------------------------------------------------------------------ references
def test_references_agree_with_the_oracle():
    c = mr.ACase("k_alpha_phase_row16", 0, 120, 5, 3, 4, 20, "SQRT", False)
    V, D, Rt, u, alpha, alpha_prev, a2, lhp, lh = mr.alpha_inputs(c)
    R = np.c_[Rt, u]
    gb = mr.gram_ref(V, D, Rt, u, np.float64)
    K = 7
    for s in range(c.S):   # the packed Gram, entry by entry
        X = np.c_[R, V[:, s]]
        full = X.T @ (D[:, s:s + 1] * X)
        for l in range(K + 1):
            for k in range(l + 1):
                assert gb[mr.tri(k, l), s] == pytest.approx(full[k, l], rel=1e-13)
    got = mr.alpha_phase_ref(gb, alpha, alpha_prev, a2, lhp, lh, c.n_iter2, np.float64)
    want = osol.alpha_phase(c.n_iter2, alpha, a2, lhp, lh, alpha_prev, R, D, V)   # (the reference's own projection loop)
    assert np.abs(got[0] - want[0]).max() <= 1e-13 and np.abs(got[1] - want[1]).max() <= 1e-13
    ref, ref_prev, bar, noise, _ = mr.alpha_refs(c)
    assert noise <= 1e-13 and bar == mr.MARGIN * max(noise, 20 * mr.EPS)
    assert np.abs(got[0] - ref).max() <= noise
    cost, mag = mr.cost_ref(mr.gram_ref(V, D, Rt, u, mr.LD), alpha)
    assert cost == pytest.approx(osol.weighted_cost(V, R, alpha, D), rel=1e-12) and mag >= cost
    # the projection, against the reference's loop
    X = np.random.RandomState(0).randn(6, 40)
    assert np.abs(mr.project(X) - osol.simplex_project_columns(X)).max() <= 1e-15
    # momentum(): numpy's recurrence in float64, bit for bit
    a, beta = osol.momentum_step(2.7, 0.8, 1.0)
    assert mr.momentum(np.float64(2.7), np.float64(0.8), np.float64(1.0))[:2] == (a, beta)
