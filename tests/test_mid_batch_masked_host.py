"""Host side of the hold-out masks and the model-selection route of the mid-size batch (no GPU): dmf_solve_mid_masked is
declared, bound and exported, the ValueErrors of Problem.solve_many_mid_masked come before any device call,
batched_ic_ineligible(kernel=...), the DEMETHIFY_BATCH_MID_IC switch, the chunk bound with masks, and the committed gates."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, UPSTREAM

PARTIAL, UNSUPERVISED = 0, 1


@pytest.fixture(scope="module", autouse=True)
def _library():
    from demethify_amd import _build

    _build.build()


def test_the_masked_entry_is_declared_bound_and_exported():
    import ctypes as C
    from demethify_amd import _lib as L

    header = (ROOT / "include" / "demethify_hip.h").read_text()
    decl = re.search(r"\nint dmf_solve_mid_masked\(([^;]*)\);", header)
    assert decl is not None
    args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
    # dmf_solve_mid's arguments with train_bits in idx's place, then dmf_solve_small_masked's two extra outputs
    plain = re.search(r"\nint dmf_solve_mid\(([^;]*)\);", header).group(1).replace("\n", " ")
    want = [a.strip() for a in plain.split(",")]
    assert want[3] == "const int64_t* idx"
    want[3] = "const uint8_t* train_bits"
    assert [" ".join(a.split()) for a in args] == [" ".join(a.split()) for a in want] + ["double* out_holdout_sum_sq",
                                                                                          "int64_t* out_n_test"]
    lib = L.load()
    fn = lib.dmf_solve_mid_masked  # (exported: ctypes resolves the symbol here)
    assert fn.restype is C.c_int and len(fn.argtypes) == len(args) == 20
    assert fn.argtypes[10] is C.c_double and fn.argtypes[13] is C.c_int
    assert lib.dmf_abi_version() == 1


@pytest.fixture
def hollow_problem(monkeypatch):
    """A Problem of the toy's shape whose library fails the test when it is called."""
    from demethify_amd import device

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"the library was asked for {name}")

    p = device.Problem.__new__(device.Problem)
    p.N, p.S, p.n_c, p._lib, p.ctx, p._h = 350, 10, 5, NoLibrary(), None, None
    monkeypatch.setattr(device.Problem, "__del__", lambda self: None, raising=False)
    return p


@pytest.mark.parametrize("method", ["solve_many_mid_masked", "solve_many_masked"])
def test_shape_errors_are_raised_before_any_device_call(hollow_problem, method):
    p = hollow_problem
    solve = getattr(p, method)
    u0s, a0s = np.full((2, 350, 1), 0.5), np.full((2, 6, 10), 1 / 6)
    ok = np.ones((2, 350, 10), dtype=bool)
    with pytest.raises(ValueError, match="u0s is B x 350 x n_u"):
        solve(np.full((2, 349, 1), 0.5), a0s, ok, PARTIAL, 5, 5, 0.0)
    with pytest.raises(ValueError, match="alpha0s shape"):
        solve(u0s, np.full((2, 5, 10), 0.2), ok, PARTIAL, 5, 5, 0.0)
    with pytest.raises(ValueError, match=r"train_masks shape \(3, 350, 10\)"):
        solve(u0s, a0s, np.ones((3, 350, 10), dtype=bool), PARTIAL, 5, 5, 0.0)
    with pytest.raises(ValueError, match=r"packed train_masks shape \(2, 350, 1\)"):
        solve(u0s, a0s, np.ones((2, 350, 1), dtype=np.uint8), PARTIAL, 5, 5, 0.0)
    with pytest.raises(ValueError, match="bool .* or packed uint8"):
        solve(u0s, a0s, np.ones((2, 350, 10)), PARTIAL, 5, 5, 0.0)
    with pytest.raises(AssertionError, match="the library was asked for dmf_solve_"):  # a valid call gets that far
        solve(u0s, a0s, np.ones((2, 350, 2), dtype=np.uint8), PARTIAL, 5, 5, 0.0)


def test_batched_ic_ineligible_by_kernel():
    from demethify_amd.ic import batched_ic_ineligible

    # 10 000 x 64 lies inside both envelopes (what keeps the command line from the one-launch batch there is its measured
    # gate), 32 768 x 64 inside the mid-size batch's only
    for kernel in ("small", "mid"):
        assert batched_ic_ineligible(4, 10000, 64, 12, PARTIAL, kernel=kernel) is None
        assert "no unknown cell type" in batched_ic_ineligible(0, 10000, 64, 12, PARTIAL, kernel=kernel)
        assert "envelope" in batched_ic_ineligible(5, 10000, 64, 11, PARTIAL, kernel=kernel)
    assert batched_ic_ineligible(4, 10000, 64, 12, PARTIAL) is None
    assert "batched kernel's envelope" in batched_ic_ineligible(4, 32768, 64, 12, PARTIAL)
    assert batched_ic_ineligible(4, 32768, 64, 12, PARTIAL) == batched_ic_ineligible(4, 32768, 64, 12, PARTIAL, kernel="small")
    assert batched_ic_ineligible(4, 32768, 64, 12, PARTIAL, kernel="mid") is None
    assert batched_ic_ineligible(4, 32768, 64, 12, PARTIAL, "mid") is None
    assert "mid-size batch's envelope" in batched_ic_ineligible(1, (1 << 17) + 1, 64, 0, UNSUPERVISED, kernel="mid")
    with pytest.raises(ValueError, match="kernel"):
        batched_ic_ineligible(4, 10000, 64, 12, PARTIAL, kernel="large")


def test_the_drivers_refuse_an_unknown_batch_kernel_before_any_device_call(toy, monkeypatch):
    from demethify_amd import ic

    V, D, ref, _ = toy
    monkeypatch.setattr(ic, "get_context", lambda *a: (_ for _ in ()).throw(AssertionError("the device was asked for")))
    for batched in (False, True):
        with pytest.raises(ValueError, match="batch_kernel"):
            ic.evaluate_best_ic(V, ref, D, "uniform_", "BCV", 1, 5, 5, 0.0, n_u_values=(1,), batched=batched, batch_kernel="large")
        with pytest.raises(ValueError, match="batch_kernel"):
            ic.bicross_validation(V, 1, D, 5, 5, 0.0, ref=ref, batched=batched, batch_kernel="large")
    with pytest.raises(ValueError, match="mid-size batch's envelope"):
        ic.bicross_validation(V, 5, D, 5, 5, 0.0, ref=ref, batched=True, batch_kernel="mid")


def test_command_line_refuses_an_unknown_mid_ic_switch(tmp_path):
    samples = [str(UPSTREAM / "output_gen" / f"sample{i}.bed") for i in range(1, 11)]
    proc = subprocess.run([sys.executable, "-m", "demethify_amd", "--ref", str(UPSTREAM / "output_gen" / "ref_matrix.bed"),
                           "--methfreq", *samples, "--bedmethyl", "--ic", "BCV", "3", "1", "2", "--outdir", str(tmp_path / "out"),
                           "--noprint"],
                          cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, DEMETHIFY_BATCH_MID_IC="2"))
    assert proc.returncode == 1, proc.stderr[-2000:]
    assert 'Error: DEMETHIFY_BATCH_MID_IC must be "0" or "1", got "2".' in proc.stderr
    assert not (tmp_path / "out").exists()  # before any output, and before any GPU work


class _Stop(Exception):
    pass


@pytest.fixture
def sweep(tmp_path, toy, monkeypatch, capsys):
    """run(criterion, **environment) -> (the keywords evaluate_best_ic was called with, the run's Note lines): the command line
    on the toy up to the sweep, which is not run."""
    from demethify_amd import demethify, ic

    calls = []

    def evaluate_best_ic(*a, **k):
        calls.append(k)
        raise _Stop

    monkeypatch.setattr(ic, "evaluate_best_ic", evaluate_best_ic)
    files = [str(UPSTREAM / "output_gen" / f"sample{i}.bed") for i in range(1, 11)]

    def run(criterion, **env):
        for name in ("DEMETHIFY_BATCH", "DEMETHIFY_BATCH_MID", "DEMETHIFY_BATCH_MID_IC"):
            monkeypatch.delenv(name, raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        calls.clear()
        with pytest.raises(_Stop):
            demethify.main(["--ref", str(UPSTREAM / "output_gen" / "ref_matrix.bed"), "--methfreq", *files, "--bedmethyl",
                            "--noprint", "--ic", criterion, "3", "1", "2", "--outdir", str(tmp_path / "out")])
        assert len(calls) == 1
        notes = [line for line in capsys.readouterr().out.splitlines() if line.startswith("Note:")]
        return {k: v for k, v in calls[0].items() if k in ("batched", "batch_kernel")}, "\n".join(notes)

    return run


def open_gates(monkeypatch, size, criteria=("CCC", "BCV", "AIC", "BIC")):
    from demethify_amd import ic

    monkeypatch.setattr(ic, "MID_BATCH_IC_MIN_ELEMENTS", size)
    monkeypatch.setattr(ic, "MID_BATCH_IC_MAX_ELEMENTS", size)
    monkeypatch.setattr(ic, "MID_BATCH_IC_CRITERIA", tuple(criteria))


def test_command_line_mid_ic_switch_off_on_and_its_notes(sweep, toy, monkeypatch):
    from demethify_amd import ic

    size = toy[0].size
    open_gates(monkeypatch, size)
    # 0 and unset: the call is what it was, whatever the gates say
    assert sweep("BCV") == ({}, "")
    assert sweep("BCV", DEMETHIFY_BATCH_MID_IC="0") == ({}, "")
    # 1 inside the gate: every gated criterion takes the route
    for criterion in ("BCV", "CCC", "AIC"):
        assert sweep(criterion, DEMETHIFY_BATCH_MID_IC="1") == ({"batched": True, "batch_kernel": "mid"}, "")
    # the criterion refuses
    open_gates(monkeypatch, size, ("CCC",))
    kw, out = sweep("BCV", DEMETHIFY_BATCH_MID_IC="1")
    assert kw == {}
    assert out.count("Note:") == 1 and "Note: DEMETHIFY_BATCH_MID_IC=1 is not used for --ic: BCV was not measured faster" in out
    assert "MID_BATCH_IC_CRITERIA" in out and out.rstrip().endswith("taking the per-solve path.")
    # the size range refuses: below, above, and a closed gate
    for lo, hi, closed in ((size + 1, 10 * size, False), (1, size - 1, False), (1, 0, True)):
        monkeypatch.setattr(ic, "MID_BATCH_IC_MIN_ELEMENTS", lo)
        monkeypatch.setattr(ic, "MID_BATCH_IC_MAX_ELEMENTS", hi)
        kw, out = sweep("CCC", DEMETHIFY_BATCH_MID_IC="1")
        assert kw == {}
        assert out.count("Note:") == 1 and f"350 x 10 elements are outside [MID_BATCH_IC_MIN_ELEMENTS, MID_BATCH_IC_MAX_ELEMENTS] = [{lo}, {hi}]" in out
        assert ("(the gate is closed)" in out) is closed


def test_command_line_mid_batch_switch_alone_leaves_ic_sweeps_as_they_are(sweep, toy, monkeypatch):
    open_gates(monkeypatch, toy[0].size)
    for criterion in ("BCV", "CCC", "AIC"):
        assert sweep(criterion, DEMETHIFY_BATCH_MID="1") == ({}, "")


def test_command_line_asks_the_mid_ic_switch_after_the_batch_switch(sweep, toy, monkeypatch):
    from demethify_amd import ic

    size = toy[0].size
    open_gates(monkeypatch, size)
    # DEMETHIFY_BATCH's own --ic route is taken: the mid-size switch is not asked
    monkeypatch.setattr(ic, "SMALL_BATCH_IC_MAX_ELEMENTS", size)
    assert sweep("BCV", DEMETHIFY_BATCH="1", DEMETHIFY_BATCH_MID_IC="1") == ({"batched": True}, "")
    # ... is not taken (its note says why): the mid-size switch takes the sweep
    monkeypatch.setattr(ic, "SMALL_BATCH_IC_MAX_ELEMENTS", size - 1)
    kw, out = sweep("BCV", DEMETHIFY_BATCH="1", DEMETHIFY_BATCH_MID_IC="1")
    assert kw == {"batched": True, "batch_kernel": "mid"}
    assert out.count("Note:") == 1 and "DEMETHIFY_BATCH=1 is not used for --ic" in out
    kw, out = sweep("AIC", DEMETHIFY_BATCH="1", DEMETHIFY_BATCH_MID_IC="1")  # (AIC is not among the small batch's criteria)
    assert kw == {"batched": True, "batch_kernel": "mid"} and out.count("Note:") == 1
    # both refuse: two notes, the per-solve path
    open_gates(monkeypatch, size, ())
    kw, out = sweep("BCV", DEMETHIFY_BATCH="1", DEMETHIFY_BATCH_MID_IC="1")
    assert kw == {} and out.count("Note:") == 2
    assert out.index("DEMETHIFY_BATCH=1 is not used") < out.index("DEMETHIFY_BATCH_MID_IC=1 is not used")


def per_solve_bytes(N, S, n_c, n_u, masked):
    from demethify_amd.device import mid_solve_plan

    W = mid_solve_plan(N, S)[1]
    K = n_c + n_u
    known = n_c * (n_c + 1) // 2 + n_c
    jobs = max(known, K * (K + 1) // 2 + K - known)
    return 8 * (W * jobs * S + N * n_u) + (N * ((S + 7) // 8) + 16 * W if masked else 0)


CORNERS = [(350, 10, 5, 1), (1, 1, 0, 1), (256, 64, 12, 4), (10000, 64, 12, 4), (32768, 64, 12, 4), (131072, 64, 12, 4),
           (131072, 64, 15, 1), (131072, 64, 0, 4), (1 << 23, 1, 0, 4), (1 << 23, 1, 12, 4), (1 << 20, 8, 0, 1), (932067, 9, 3, 2)]


def test_chunk_bound_with_masks_stays_within_its_budget_and_the_plain_one_is_unchanged():
    from demethify_amd.bootstrap import mid_batch_chunk

    for N, S, n_c, n_u in CORNERS:
        plain, masked = mid_batch_chunk(N, S, n_c, n_u), mid_batch_chunk(N, S, n_c, n_u, masked=True)
        # today's answers: the bound of tests/test_mid_batch_host.py, restated
        per = per_solve_bytes(N, S, n_c, n_u, False)
        assert plain == mid_batch_chunk(N, S, n_c, n_u, False) == int(max(1, min(1024, (1 << 28) // per)))
        # with masks: the mask bytes and the two framing passes' partials are counted too
        per = per_solve_bytes(N, S, n_c, n_u, True)
        assert 1 <= masked <= plain
        assert masked == 1 or masked * per <= 1 << 28
        assert masked == 1024 or (masked + 1) * per > 1 << 28
    assert [mid_batch_chunk(*c) for c in CORNERS[:6]] == [1024, 1024, 1024, 124, 67, 37]  # (the values before the argument)
    assert [mid_batch_chunk(*c, masked=True) for c in CORNERS[3:6]] == [119, 63, 32]


def test_committed_gates_and_criteria_are_consistent():
    from demethify_amd import _lib as L
    from demethify_amd import ic

    lo, hi, criteria = ic.MID_BATCH_IC_MIN_ELEMENTS, ic.MID_BATCH_IC_MAX_ELEMENTS, ic.MID_BATCH_IC_CRITERIA
    assert isinstance(lo, int) and isinstance(hi, int) and isinstance(criteria, tuple)
    assert set(criteria) <= {"CCC", "BCV", "AIC", "BIC"} and len(set(criteria)) == len(criteria)
    if lo <= hi:  # an open gate: inside the envelope, and for at least one criterion
        assert 1 <= lo and hi <= L.MID_MAX_ELEMENTS and criteria
    else:  # a closed gate names no criterion
        assert criteria == ()
    for name in ("MID_BATCH_IC_MIN_ELEMENTS", "MID_BATCH_IC_MAX_ELEMENTS", "MID_BATCH_IC_CRITERIA"):
        assert name in ic.__all__
