"""Host side of the purity-constrained mid-size batch (no GPU): the mid_purity switch of batched_ineligible, the refusal of
bt_ci(batch_kernel="mid", batched_mid_purity=True) before any device call, the DEMETHIFY_BATCH_MID_PURITY switch and its
gate, the Python checks of solve_many_mid(purity=...), and the preconditions of every oracle run the GPU file uses."""
import os
import subprocess
import sys

import numpy as np
import pytest

import small_batch_purity_cases as cases
from conftest import ROOT, UPSTREAM

PARTIAL, UNSUPERVISED = 0, 1
PINNED = "the purity-constrained alpha phase is not part of the mid-size batch"


@pytest.fixture(scope="module", autouse=True)
def _library():
    from demethify_amd import _build

    _build.build()


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to get at the device fails the test (as in tests/test_mid_batch_host.py)."""
    from demethify_amd import bootstrap, device

    def refuse(*a, **k):
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(device, "get_context", refuse)
    monkeypatch.setattr(bootstrap, "get_context", refuse)
    monkeypatch.setattr(device.Problem, "__init__", refuse)


class _Stop(Exception):
    pass


def test_every_oracle_run_of_the_gpu_file_meets_its_preconditions():
    """Stop margin >= 1e-4 tol for every natural stop and smallest Frank-Wolfe argmin gap >= 1e-9 for every case of
    tests/test_gpu_mid_batch_purity.py (the runs of tests/small_batch_purity_cases.py)."""
    cases.check_preconditions("toy restart", cases.toy_restarts(), cases.TOL)
    cases.check_preconditions("toy replicate 100 x 20", cases.toy_replicates(20)[1], cases.TOL)
    chosen = [b for b, r in enumerate(cases.toy_replicates(500)[1]) if cases.qualifies(r)]
    print(f"toy replicates 100 x 500 that meet both preconditions: {chosen}")
    assert len(chosen) >= 12
    for edge in cases.EDGES:
        runs = cases.edge_runs(*edge)[2]
        cases.check_preconditions(f"edge {edge}", runs, 0.0)
        assert all(len(r.trace) == cases.EDGE_ITERS for r in runs)
    costs = np.sort([r.trace[-1] for r in cases.toy_restarts()[:8]])
    assert (costs[1] - costs[0]) / costs[0] > 10 * cases.COST_RTOL  # (the command-line test's pick is not a near tie)


def test_the_symbol_and_the_keyword_exist():
    import inspect

    from demethify_amd import _lib as L
    from demethify_amd.device import Problem

    assert hasattr(L.load(), "dmf_solve_mid_purity")
    assert inspect.signature(Problem.solve_many_mid).parameters["purity"].default is None


def test_mid_purity_opens_exactly_the_purity_case():
    from demethify_amd.bootstrap import batched_ineligible

    purity = list(cases.P)
    assert batched_ineligible(1, 350, 10, 5, "uniform_", purity, PARTIAL, kernel="mid", mid_purity=True) is None
    assert batched_ineligible(1, 350, 10, 5, "beta", np.array(purity), PARTIAL, kernel="mid", mid_purity=True) is None
    assert batched_ineligible(4, 10000, 64, 12, "uniform_", [50.0] * 64, PARTIAL, kernel="mid", mid_purity=True) is None
    # the small kernel's purity reasons
    assert "no known block" in batched_ineligible(1, 350, 10, 0, "uniform_", purity, UNSUPERVISED, kernel="mid", mid_purity=True)
    assert "no known block" in batched_ineligible(1, 350, 10, 0, "uniform_", purity, PARTIAL, kernel="mid", mid_purity=True)
    # the default still gives the pinned sentence, whatever the small kernel's switch says
    for kw in ({}, {"mid_purity": False}, {"purity_batched": True}, {"purity_batched": True, "mid_purity": False}):
        assert batched_ineligible(1, 350, 10, 5, "uniform_", purity, PARTIAL, kernel="mid", **kw) == PINNED
    # the switch opens nothing for the small kernel, and changes nothing without a purity vector
    assert "batched_purity=True" in batched_ineligible(1, 350, 10, 5, "uniform_", purity, PARTIAL, mid_purity=True)
    assert batched_ineligible(1, 350, 10, 5, "uniform_", None, PARTIAL, kernel="mid", mid_purity=True) is None
    # every other reason stands
    assert "mid-size batch's envelope" in batched_ineligible(5, 350, 10, 5, "uniform_", purity, PARTIAL, kernel="mid",
                                                             mid_purity=True)
    assert "reads the resampled data" in batched_ineligible(1, 350, 10, 5, "uniform", purity, PARTIAL, kernel="mid",
                                                            mid_purity=True)
    assert "cpg" in batched_ineligible(1, 350, 10, 5, "uniform_", purity, PARTIAL, profile_rows="cpg", kernel="mid",
                                       mid_purity=True)


@pytest.mark.parametrize("change,word", [(dict(ref=None), "purity"), (dict(init_option="uniform"), "reads the resampled data"),
                                         (dict(n_u=5), "mid-size batch's envelope"), (dict(profile_rows="cpg"), "cpg")])
def test_ineligible_mid_purity_bootstrap_raises_before_any_device_call(tmp_path, toy, no_device, change, word):
    from demethify_amd.bootstrap import bt_ci

    V, D, ref, header = toy
    kw = dict(n_u=1, ref=ref, init_option="uniform_", profile_rows="position")
    kw.update(change)
    samples = [f"s{k}" for k in range(V.shape[1])]
    with pytest.raises(ValueError, match=word) as e:
        bt_ci(90, 4, kw["n_u"], V, D, kw["ref"], kw["init_option"], 5, 5, 0.0, header if kw["ref"] is not None else [],
              str(tmp_path), samples, list(cases.P), 1, profile_rows=kw["profile_rows"], batched=True, batch_kernel="mid",
              batched_mid_purity=True)
    assert 'batch_kernel="mid"' in str(e.value)
    assert not list(tmp_path.iterdir())


def test_batched_mid_purity_alone_is_no_route(tmp_path, toy, no_device):
    """Without batched_mid_purity the mid kernel keeps refusing a purity vector; the switch is looked at only with
    batched=True, batch_kernel="mid" (with the small kernel the small kernel's own refusal stands)."""
    from demethify_amd.bootstrap import bt_ci

    V, D, ref, header = toy
    samples = [f"s{k}" for k in range(V.shape[1])]
    with pytest.raises(ValueError, match="not part of the mid-size batch"):
        bt_ci(90, 4, 1, V, D, ref, "uniform_", 5, 5, 0.0, header, str(tmp_path), samples, list(cases.P), 1, batched=True,
              batch_kernel="mid")
    with pytest.raises(ValueError, match="batched_purity=True"):
        bt_ci(90, 4, 1, V, D, ref, "uniform_", 5, 5, 0.0, header, str(tmp_path), samples, list(cases.P), 1, batched=True,
              batched_mid_purity=True)
    assert not list(tmp_path.iterdir())


def test_solve_many_mid_refuses_a_bad_purity_before_any_device_call():
    """A wrong length, a matrix, an unsupervised mode, a problem without a reference: ValueError from the Python layer, no
    library call (the problem here has no handle at all)."""
    from demethify_amd import device

    class Lib:
        def __getattr__(self, name):
            raise AssertionError(f"the library was asked for {name}")

    def problem(n_c):
        p = device.Problem.__new__(device.Problem)
        p.N, p.S, p.n_c, p._lib, p._h, p.ctx = 6, 3, n_c, Lib(), None, None
        return p

    u0s, good = np.full((2, 6, 1), 0.5), np.array([0.2, 0.5, 1.0])
    with pytest.raises(ValueError, match="purity"):
        problem(2).solve_many_mid(u0s, np.full((2, 3, 3), 1 / 3), PARTIAL, 1, 1, 0.0, purity=good[:2])
    with pytest.raises(ValueError, match="purity"):
        problem(2).solve_many_mid(u0s, np.full((2, 3, 3), 1 / 3), PARTIAL, 1, 1, 0.0, purity=np.tile(good, (2, 1)))
    with pytest.raises(ValueError, match="purity"):
        problem(2).solve_many_mid(u0s, np.full((2, 3, 3), 1 / 3), UNSUPERVISED, 1, 1, 0.0, purity=good)
    with pytest.raises(ValueError, match="purity"):
        problem(0).solve_many_mid(u0s, np.full((2, 1, 3), 1.0), PARTIAL, 1, 1, 0.0, purity=good)


def test_the_gate_constants_are_a_range_or_closed():
    from demethify_amd import bootstrap

    lo, hi = bootstrap.MID_BATCH_PURITY_MIN_ELEMENTS, bootstrap.MID_BATCH_PURITY_MAX_ELEMENTS
    assert isinstance(lo, int) and isinstance(hi, int) and lo >= 1 and hi >= 0  # (MIN > MAX is a closed gate)
    # nothing below the small batch's own purity gate was measured against it, and nothing outside the envelope can be inside
    assert lo > hi or (bootstrap.SMALL_BATCH_PURITY_MAX_ELEMENTS <= lo and hi <= 1 << 23)


def test_command_line_refuses_an_unknown_mid_purity_switch(tmp_path):
    samples = [str(UPSTREAM / "output_gen" / f"sample{i}.bed") for i in range(1, 11)]
    proc = subprocess.run([sys.executable, "-m", "demethify_amd", "--ref", str(UPSTREAM / "output_gen" / "ref_matrix.bed"),
                           "--methfreq", *samples, "--bedmethyl", "--nbunknown", "1", "--restart", "4", "--purity",
                           *[str(int(p)) for p in cases.P], "--outdir", str(tmp_path / "out"), "--noprint"],
                          cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, DEMETHIFY_BATCH_MID_PURITY="2"))
    assert proc.returncode == 1, proc.stderr[-2000:]
    assert "DEMETHIFY_BATCH_MID_PURITY" in proc.stderr and '"2"' in proc.stderr
    assert not (tmp_path / "out").exists()  # before any output, and before any GPU work


def test_command_line_routes_purity_restarts_through_the_mid_batch_inside_its_gate_only(tmp_path, toy, monkeypatch, capsys):
    """DEMETHIFY_BATCH_MID_PURITY=1 --purity P --restart 4 on the toy: with the gate away from the toy's size a note names the
    reason and the restarts reach shard.sharded_restarts; with the gate around it they reach Problem.solve_many_mid with the
    purity vector the point estimate uses (1 - P / 100); without --purity the switch is silent."""
    from demethify_amd import bootstrap, demethify, device, shard
    import demethify_amd.staging as staging

    V = toy[0]
    seen = []
    monkeypatch.delenv("DEMETHIFY_BATCH", raising=False)
    monkeypatch.delenv("DEMETHIFY_BATCH_MID", raising=False)
    monkeypatch.setenv("DEMETHIFY_BATCH_MID_PURITY", "1")
    monkeypatch.setattr(device.Problem, "__init__", lambda self, *a, **k: None)
    monkeypatch.setattr(device.Problem, "close", lambda self: None)
    monkeypatch.setattr(device, "get_context", lambda *a: None)
    monkeypatch.setattr(staging, "reserve", lambda *a, **k: None)

    def restarts(*a, **k):
        seen.append("sharded_restarts")
        raise _Stop

    def solve_many_mid(self, u0s, a0s, *a, **k):
        seen.append(("solve_many_mid", len(u0s), None if k.get("purity") is None else np.array(k["purity"])))
        raise _Stop

    monkeypatch.setattr(shard, "sharded_restarts", restarts)
    monkeypatch.setattr(device.Problem, "solve_many_mid", solve_many_mid)
    monkeypatch.setattr(device.Problem, "solve_many", lambda *a, **k: seen.append("solve_many"))
    files = [str(UPSTREAM / "output_gen" / f"sample{i}.bed") for i in range(1, 11)]
    argv = ["--ref", str(UPSTREAM / "output_gen" / "ref_matrix.bed"), "--methfreq", *files, "--bedmethyl", "--noprint",
            "--nbunknown", "1", "--restart", "4", "--outdir", str(tmp_path / "out")]
    with_purity = argv + ["--purity", *[str(int(p)) for p in cases.P]]

    monkeypatch.setattr(bootstrap, "MID_BATCH_PURITY_MIN_ELEMENTS", V.size + 1)
    monkeypatch.setattr(bootstrap, "MID_BATCH_PURITY_MAX_ELEMENTS", 10 * V.size)
    with pytest.raises(_Stop):
        demethify.main(with_purity)
    assert seen == ["sharded_restarts"]
    note = capsys.readouterr().out
    assert "DEMETHIFY_BATCH_MID_PURITY=1 is not used for --restart" in note and "MID_BATCH_PURITY_MIN_ELEMENTS" in note

    # a closed gate says so
    seen.clear()
    monkeypatch.setattr(bootstrap, "MID_BATCH_PURITY_MAX_ELEMENTS", V.size)
    with pytest.raises(_Stop):
        demethify.main(with_purity)
    assert seen == ["sharded_restarts"]
    assert "the gate is closed" in capsys.readouterr().out

    seen.clear()
    monkeypatch.setattr(bootstrap, "MID_BATCH_PURITY_MIN_ELEMENTS", V.size)
    with pytest.raises(_Stop):
        demethify.main(with_purity)
    assert len(seen) == 1 and seen[0][:2] == ("solve_many_mid", 4)
    assert np.array_equal(seen[0][2], 1 - cases.P / 100)
    assert "is not used" not in capsys.readouterr().out

    # without --purity the switch routes nothing and says nothing
    seen.clear()
    with pytest.raises(_Stop):
        demethify.main(argv)
    assert seen == ["sharded_restarts"]
    assert "DEMETHIFY_BATCH_MID_PURITY" not in capsys.readouterr().out

    # with DEMETHIFY_BATCH_MID=1 as well, a purity run is the purity route's to speak about
    seen.clear()
    monkeypatch.setenv("DEMETHIFY_BATCH_MID", "1")
    with pytest.raises(_Stop):
        demethify.main(with_purity)
    assert len(seen) == 1 and seen[0][:2] == ("solve_many_mid", 4)
    assert "is not used" not in capsys.readouterr().out
