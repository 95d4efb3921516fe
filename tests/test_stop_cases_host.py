"""The case table of tests/test_gpu_stop_paths.py (tests/stop_cases.py) on the numpy oracle and the pure selection calls:
every case's stop is a reachable one with room on both sides of the threshold, has enqueued iterations behind it, pauses
where the model says, and lands on the kernels it names; the table reaches every RowKind, GramKind and AlphaKind of
dmf_select.h (read from the header's text, so a new enumerator fails here until it gets a case).  No GPU."""
import numpy as np
import pytest

import stop_cases as sc

CASES = pytest.mark.parametrize("c", sc.CASES, ids=sc.IDS)


@CASES
def test_stop_is_reachable_with_a_margin(c, record_property):
    """The conditions on a case's inputs, on the oracle alone."""
    a = sc.analyse(c)
    d, k, tol = a.d, c.k, a.tol
    print(f"{c.name}: k {k} tol {tol:.6g} margin {a.margin:.3f} band clearance {a.clearance:.3f} pauses {a.pauses} "
          f"confirmed {a.n_confirmed} unconfirmed {a.n_unconfirmed} cost {a.cost:.6g}")
    for name in ("tol", "margin", "clearance"):
        record_property(name, getattr(a, name))
    assert len(d) == sc.TRACE + 1 and np.all(np.isfinite(d[1:])) and np.all(d[1:] > 0)
    assert k >= 2
    assert d[k] < d[1:k].min()                              # reachable: nothing before k is below what stops at k
    assert d[k] < tol < d[1:k].min()
    assert a.stop == k                                      # ... and the oracle's own loop stops there under tol
    assert a.margin >= sc.MARGIN
    assert a.clearance >= sc.MARGIN                         # no d_j, j <= k, within 1 % of the band's edge 10 tol
    if not sc.runs_ahead(c):
        assert k in range(2, sc.TRACE + 1)                  # (the host looks at the state after every iteration)
    else:
        assert k in sc.FIRST_BATCH or k in sc.SECOND_BATCH  # at least two enqueued iterations behind the stop
        assert 1 <= a.pauses[0] <= 6                        # ... and behind the first pause
    assert a.pauses[-1] == k and a.n_confirmed + a.n_unconfirmed == len(a.pauses)
    # The device's Gram-form costs are held to COST_RTOL of the oracle's: its differences lie within 2 COST_RTOL cf of
    # d_j.  Every decision -- stop, pause -- must have a hundred times that to spare.
    noise = 2 * sc.COST_RTOL * a.cf_max
    assert sc.MARGIN * tol >= 100 * noise and a.clearance * sc.BAND * tol >= 100 * noise
    assert a.gap >= sc.GAP                                  # purity: no Frank-Wolfe vertex decision is a near tie (else inf)


def test_both_batches_are_stopped_in():
    first = [c.name for c in sc.CASES if sc.runs_ahead(c) and c.k in sc.FIRST_BATCH]
    second = [c.name for c in sc.CASES if sc.runs_ahead(c) and c.k in sc.SECOND_BATCH]
    assert len(first) >= 4 and len(second) >= 4, (first, second)
    # the pause model is exercised on both of its branches, and by a first pause that is not the first iteration
    assert sum(sc.analyse(c).n_unconfirmed > 0 for c in sc.CASES) >= 4
    assert sum(sc.analyse(c).n_unconfirmed == 0 for c in sc.CASES) >= 4
    assert any(sc.analyse(c).pauses[0] > 1 for c in sc.CASES if sc.runs_ahead(c))
    # the host runs ahead in every case but k_u_step_direct's own and the 17-unknown one, whose fall-back u path it is
    assert [c.name for c in sc.CASES if not sc.runs_ahead(c)] == ["05-cm-rows-wide", "13-direct"]


def test_pause_model_follows_the_step_loop():
    """pause_model on hand-made differences (tol = 1: the band is d < 10)."""
    inf = np.inf
    assert sc.pause_model(np.array([inf, 5.0, 4.0, 0.5]), 3, 1.0) == ([1, 2, 3], 3, 0)   # the start's cost is a streaming cost
    assert sc.pause_model(np.array([inf, 50.0, 4.0, 0.5]), 3, 1.0) == ([2, 3], 1, 1)     # first inside the band: Gram form
    assert sc.pause_model(np.array([inf, 5.0, 50.0, 4.0, 40.0, 3.0, 0.5]), 6, 1.0) == ([1, 3, 5, 6], 2, 2)
    assert sc.pause_model(np.array([inf, 50.0, 40.0, 0.5]), 3, 1.0) == ([3], 0, 1)
    assert sc.threshold(np.array([inf, 8.0, 4.0, 1.0]), 3) == (2.0, 0.5)
    assert [r[0] for r in sc.reachable(np.array([inf, 8.0, 9.0, 4.0, 4.0, 1.0]))] == [3, 5]


@CASES
def test_case_lands_on_the_kernels_it_names(c):
    desc = sc.select_describe(c)
    assert desc is not None and sc.kinds(desc) == (c.row, c.gram, c.alpha), (c.name, desc)
    for token in c.extra:
        assert token in desc, (c.name, token, desc)
    # the u phase's own launch plan (dmf_u_phase_describe, solver route) names the same row kernel
    text = sc.u_phase_text(c)
    head = {sc.V2: "k_rowpass_v2<", sc.V2X: "k_rowpass_v2<", sc.CM_BU: "k_cm_i8<nd=1>+k_inner_bu ",
            sc.CM_ROWS: "k_cm_i8<nd=1>+k_u_inner_rows ", sc.FUSED: "k_rowpass_fused<", sc.BIG: "k_u_phase_big<",
            sc.SPLIT: "k_u_phase_mfma<", sc.MFMA: "k_u_phase_mfma<", sc.UGRAM: "k_u_phase_gram<", sc.DIRECT: "k_u_step_direct "}
    assert text is not None and text.startswith(head[c.row]), (c.name, text)
    if c.row in (sc.SPLIT, sc.MFMA):
        assert (" split " in text) == (c.row == sc.SPLIT) and (" one-launch " in text) == (c.row == sc.MFMA), text
    if c.row in (sc.V2, sc.V2X):
        assert (" x16 " in text) == (c.row == sc.V2X), text
    if c.row == sc.FUSED:
        assert c.N % 16 != 0 and text.endswith(f"tail={c.N % 16}"), text
    assert 53 <= c.N <= 400 or c.row == sc.DIRECT
    assert 6 <= c.S <= 128 or c.name == "17-cm-rows-257"   # (k_u_inner_rows behind k_cm_i8 with run-ahead: S > 256 only)


def test_table_reaches_every_enumerator():
    rows, grams, alphas = sc.enumerators("RowKind"), sc.enumerators("GramKind"), sc.enumerators("AlphaKind")
    assert len(rows) == 9 and len(grams) == 6 and len(alphas) == 6, (rows, grams, alphas)   # (the parse found the lists)
    # every enumerator has a describe text here: a new one fails until ROW_TEXT / GRAM_TEXT / ALPHA_TEXT and the table know it
    assert set(rows) == set(sc.ROW_TEXT) and set(grams) == set(sc.GRAM_TEXT) and set(alphas) == set(sc.ALPHA_TEXT)
    got = [sc.kinds(sc.select_describe(c)) for c in sc.CASES]
    ahead = [g for g, c in zip(got, sc.CASES) if sc.runs_ahead(c)]
    for e in rows:
        assert any(g[0] in sc.ROW_TEXT[e] for g in got), f"no case on RowKind::{e}"
        # ... and, but for k_u_step_direct, by a case with enqueued iterations behind its stop
        assert e == "UStepDirect" or any(g[0] in sc.ROW_TEXT[e] for g in ahead), f"no run-ahead case on RowKind::{e}"
    for e in grams:
        assert any(g[1] == sc.GRAM_TEXT[e] for g in ahead), f"no run-ahead case on GramKind::{e}"
    for e in alphas:
        assert any(g[2] == sc.ALPHA_TEXT[e] for g in ahead), f"no run-ahead case on AlphaKind::{e}"
    # both forms of the one-launch row pass, the purity solver on both of its kernels, a masked problem
    assert {sc.V2, sc.V2X} <= {g[0] for g in got}
    assert any(c.masked for c in sc.CASES) and any(not c.ints for c in sc.CASES)
    # the kernels a mutation run removes the check from, one at a time: each must have cases behind it
    assert sum(g[2] == sc.ROW16 for g in ahead) >= 4
    assert sum(g[0] in (sc.CM_ROWS, sc.SPLIT) for g in ahead) >= 3          # k_u_inner_rows
    assert sum(g[1] == sc.GU or g[0] == sc.FUSED for g in ahead) >= 4       # k_gram_u (the fused pass: its ragged tail)
