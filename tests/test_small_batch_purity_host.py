"""Host side of the batched purity-constrained solve (no GPU): the preconditions of every case the GPU file runs, on the
oracle's own f64 trajectory; the purity opt-in of batched_ineligible and bt_ci; and that nothing reaches
Problem.solve_many for a purity run while the switches are off."""
import numpy as np
import pytest

import small_batch_purity_cases as cases
from conftest import UPSTREAM

PARTIAL, UNSUPERVISED = 0, 1
TODAY = "the purity-constrained alpha phase is not part of the batched kernel"


@pytest.fixture(scope="module", autouse=True)
def _library():
    from demethify_amd import _build

    _build.build()


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to get at the device fails the test (as in tests/test_small_batch_host.py)."""
    from demethify_amd import bootstrap, device

    def refuse(*a, **k):
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(device, "get_context", refuse)
    monkeypatch.setattr(bootstrap, "get_context", refuse)
    monkeypatch.setattr(device.Problem, "__init__", refuse)


class _Stop(Exception):
    pass


def test_no_case_has_a_near_tie():
    """Stop margin >= 1e-4 tol for every natural stop and smallest Frank-Wolfe argmin gap >= 1e-9 for every case of
    tests/test_gpu_small_batch_purity.py.  On record: the toy restarts have smallest gap 1.1e-9 .. 1.5e-9 (by BLAS) and
    smallest margin 0.079; all 24 replicates qualify at 100 x 20; at 100 x 500 the 15 replicates 2, 4, 6, 7, 8, 9, 12, 14,
    15, 17, 18, 20, 21, 22, 23 do; the edge shapes' smallest gap is 1.7e-8 (+inf where both blocks have one row)."""
    cases.check_preconditions("toy restart", cases.toy_restarts(), cases.TOL)
    cases.check_preconditions("toy replicate 100 x 20", cases.toy_replicates(20)[1], cases.TOL)
    chosen = [b for b, r in enumerate(cases.toy_replicates(500)[1]) if cases.qualifies(r)]
    print(f"toy replicates 100 x 500 that meet both preconditions: {chosen}")
    assert len(chosen) >= 12
    for edge in cases.EDGES:
        runs = cases.edge_runs(*edge)[2]
        cases.check_preconditions(f"edge {edge}", runs, 0.0)
        assert all(len(r.trace) == cases.EDGE_ITERS for r in runs)
    assert cases.edge_runs(64, 1, 1, 1, 7)[2][0].gap == np.inf


def test_purity_is_eligible_only_when_asked_for():
    from demethify_amd.bootstrap import batched_ineligible

    purity = list(cases.P)
    for kw in ({}, {"purity_batched": False}):
        reason = batched_ineligible(1, 350, 10, 5, "uniform_", purity, PARTIAL, **kw)
        assert reason.startswith(TODAY) and "batched_purity=True" in reason
    assert batched_ineligible(1, 350, 10, 5, "uniform_", purity, PARTIAL, purity_batched=True) is None
    assert batched_ineligible(1, 350, 10, 5, "beta", np.array(purity), PARTIAL, purity_batched=True) is None
    # without a purity vector the switch changes nothing
    assert batched_ineligible(1, 350, 10, 5, "uniform_", None, PARTIAL, purity_batched=True) is None
    assert batched_ineligible(1, 350, 10, 5, "uniform_", [], PARTIAL, purity_batched=True) is None
    # still refused: no reference to hold at that mass, a shape outside the envelope, and every other reason
    assert "purity" in batched_ineligible(1, 350, 10, 0, "uniform_", purity, UNSUPERVISED, purity_batched=True)
    assert "purity" in batched_ineligible(1, 350, 10, 0, "uniform_", purity, PARTIAL, purity_batched=True)
    assert "envelope" in batched_ineligible(5, 350, 10, 5, "uniform_", purity, PARTIAL, purity_batched=True)
    assert "envelope" in batched_ineligible(1, 16385, 64, 5, "uniform_", [50.0] * 64, PARTIAL, purity_batched=True)
    assert "reads the resampled data" in batched_ineligible(1, 350, 10, 5, "uniform", purity, PARTIAL, purity_batched=True)
    assert "cpg" in batched_ineligible(1, 350, 10, 5, "uniform_", purity, PARTIAL, profile_rows="cpg", purity_batched=True)


def test_batched_purity_bootstrap_without_a_reference_raises_before_any_device_call(tmp_path, toy, no_device):
    from demethify_amd.bootstrap import bt_ci

    V, D, _, _ = toy
    samples = [f"s{k}" for k in range(V.shape[1])]
    with pytest.raises(ValueError, match="purity") as e:
        bt_ci(90, 4, 1, V, D, None, "uniform_", 5, 5, 0.0, [], str(tmp_path), samples, list(cases.P), 1, batched=True,
              batched_purity=True)
    assert "without a reference" in str(e.value)
    assert not list(tmp_path.iterdir())


def test_batched_purity_alone_changes_nothing(tmp_path, toy, no_device):
    """batched=True keeps refusing a purity vector, now with a pointer to the opt-in; batched_purity without batched is not
    a route of its own (it is looked at only when batched is set)."""
    from demethify_amd.bootstrap import bt_ci

    V, D, ref, header = toy
    samples = [f"s{k}" for k in range(V.shape[1])]
    with pytest.raises(ValueError, match="batched_purity=True") as e:
        bt_ci(90, 4, 1, V, D, ref, "uniform_", 5, 5, 0.0, header, str(tmp_path), samples, list(cases.P), 1, batched=True)
    assert TODAY in str(e.value) and "batched=True" in str(e.value)
    assert not list(tmp_path.iterdir())


def test_solve_many_refuses_a_bad_purity_before_any_device_call():
    """A wrong length, an unsupervised mode, a problem without a reference: ValueError from the Python layer, no library
    call (the problem here has no handle at all)."""
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
        problem(2).solve_many(u0s, np.full((2, 3, 3), 1 / 3), PARTIAL, 1, 1, 0.0, purity=good[:2])
    with pytest.raises(ValueError, match="purity"):
        problem(2).solve_many(u0s, np.full((2, 3, 3), 1 / 3), PARTIAL, 1, 1, 0.0, purity=np.tile(good, (2, 1)))
    with pytest.raises(ValueError, match="purity"):
        problem(2).solve_many(u0s, np.full((2, 3, 3), 1 / 3), UNSUPERVISED, 1, 1, 0.0, purity=good)
    with pytest.raises(ValueError, match="purity"):
        problem(0).solve_many(u0s, np.full((2, 1, 3), 1.0), PARTIAL, 1, 1, 0.0, purity=good)


def test_without_the_switches_a_purity_run_never_reaches_solve_many(tmp_path, toy, monkeypatch):
    """batched=False and an unset DEMETHIFY_BATCH with a purity vector: bt_ci goes to a Problem and its per-replicate
    gathers, the command line's restarts to shard.sharded_restarts -- Problem.solve_many is never called."""
    from demethify_amd import bootstrap, demethify, device, shard
    import demethify_amd.staging as staging

    V, D, ref, header = toy
    seen = []
    monkeypatch.setattr(device.Problem, "solve_many", lambda *a, **k: seen.append("solve_many"))

    def problem_init(self, *a, **k):
        seen.append("Problem")
        raise _Stop

    monkeypatch.setattr(device.Problem, "__init__", problem_init)
    monkeypatch.setattr(bootstrap, "get_context", lambda *a: None)
    monkeypatch.setattr(bootstrap.shard, "my_items", lambda *a: [])
    monkeypatch.setattr(staging, "reserve", lambda *a, **k: None)
    samples = [f"s{k}" for k in range(V.shape[1])]
    for kw in ({}, {"batched_purity": True}):  # (the second switch alone is no route)
        seen.clear()
        with pytest.raises(_Stop):
            bootstrap.bt_ci(90, 4, 1, V, D, ref, "uniform_", 5, 5, 0.0, header, str(tmp_path), samples, list(cases.P), 1, **kw)
        assert seen == ["Problem"]

    seen.clear()
    monkeypatch.delenv("DEMETHIFY_BATCH", raising=False)
    monkeypatch.setattr(device.Problem, "__init__", lambda self, *a, **k: None)
    monkeypatch.setattr(device.Problem, "close", lambda self: None)
    monkeypatch.setattr(device, "get_context", lambda *a: None)

    def restarts(*a, **k):
        seen.append("sharded_restarts")
        raise _Stop

    monkeypatch.setattr(shard, "sharded_restarts", restarts)
    monkeypatch.setattr(shard, "sharded_restarts_batched", lambda *a, **k: seen.append("sharded_restarts_batched"))
    files = [str(UPSTREAM / "output_gen" / f"sample{i}.bed") for i in range(1, 11)]
    with pytest.raises(_Stop):
        demethify.main(["--ref", str(UPSTREAM / "output_gen" / "ref_matrix.bed"), "--methfreq", *files, "--bedmethyl",
                        "--noprint", "--nbunknown", "1", "--restart", "4", "--purity", *[str(int(p)) for p in cases.P],
                        "--outdir", str(tmp_path / "out")])
    assert seen == ["sharded_restarts"]
