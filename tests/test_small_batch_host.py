"""Host side of the batched small-problem path (no GPU): the envelope of dmf_solve_small_supported, the refusals of
bt_ci(batched=True) before any device call, the DEMETHIFY_BATCH switch, and that nothing changes while it is off."""
import os
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


@pytest.mark.parametrize("N,S,n_c,n_u,mode,want", [
    (350, 10, 5, 1, PARTIAL, True), (350, 10, 0, 4, UNSUPERVISED, True),
    (1, 1, 0, 1, PARTIAL, True), (0, 1, 0, 1, PARTIAL, False), (10, 0, 0, 1, PARTIAL, False),
    (100, 64, 2, 1, PARTIAL, True), (100, 65, 2, 1, PARTIAL, False),                      # S <= 64
    (100, 8, 12, 4, PARTIAL, True), (100, 8, 13, 4, PARTIAL, False), (100, 8, 15, 1, PARTIAL, True),
    (100, 8, 16, 1, PARTIAL, False),                                                       # K <= 16
    (100, 8, 0, 4, UNSUPERVISED, True), (100, 8, 0, 5, UNSUPERVISED, False), (100, 8, 3, 0, PARTIAL, False),  # 1 <= n_u <= 4
    (16384, 64, 0, 1, PARTIAL, True), (16385, 64, 0, 1, PARTIAL, False),                   # N S <= 2^20 (2^20 + 64 is out)
    (1 << 20, 1, 1, 1, PARTIAL, True), ((1 << 20) + 1, 1, 1, 1, PARTIAL, False),
    (100, 8, 2, 1, 2, False), (100, 8, 2, 1, -1, False), (100, 8, -1, 2, PARTIAL, False),   # modes, a negative n_c
])
def test_envelope_of_small_solve_supported(N, S, n_c, n_u, mode, want):
    from demethify_amd import _lib as L
    from demethify_amd.device import small_solve_supported

    assert small_solve_supported(N, S, n_c, n_u, mode) is want
    assert (L.SMALL_MAX_S, L.SMALL_MAX_K, L.SMALL_MAX_NU, L.SMALL_MAX_ELEMENTS) == (64, 16, 4, 1 << 20)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to get at the device fails the test."""
    from demethify_amd import bootstrap, device

    def refuse(*a, **k):
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(device, "get_context", refuse)
    monkeypatch.setattr(bootstrap, "get_context", refuse)
    monkeypatch.setattr(device.Problem, "__init__", refuse)


INELIGIBLE = {  # name -> (bt_ci arguments that differ from an eligible call, a word of the reason)
    "no unknown type": (dict(n_u=0), "no unknown cell type"),
    "purity": (dict(purity=[80.0] * 10), "purity"),
    "an observer": (dict(_observe=lambda *a: None), "_observe"),
    "alignment": (dict(n_u=2, align_unknown=True), "aligning"),
    "alignment by default without a reference": (dict(n_u=2, ref=None), "aligning"),
    "rows by CpG": (dict(profile_rows="cpg"), "cpg"),
    "uniform reads the data": (dict(init_option="uniform"), "reads the resampled data"),
    "SVD reads the data": (dict(init_option="SVD"), "reads the resampled data"),
    "too many unknown types": (dict(n_u=5), "envelope"),
    "too many types": (dict(n_u=4, ref=np.full((350, 13), 0.5)), "envelope"),
}


@pytest.mark.parametrize("name", sorted(INELIGIBLE))
def test_ineligible_batched_bootstrap_raises_before_any_device_call(tmp_path, toy, no_device, name):
    from demethify_amd.bootstrap import bt_ci

    V, D, ref, header = toy
    change, word = INELIGIBLE[name]
    kw = dict(n_u=1, ref=ref, init_option="uniform_", purity=None, _observe=None, align_unknown=None, profile_rows="position")
    kw.update(change)
    samples = [f"s{k}" for k in range(V.shape[1])]
    with pytest.raises(ValueError, match=word) as e:
        bt_ci(90, 4, kw["n_u"], V, D, kw["ref"], kw["init_option"], 5, 5, 0.0, header, str(tmp_path), samples, kw["purity"], 1,
              _observe=kw["_observe"], align_unknown=kw["align_unknown"], profile_rows=kw["profile_rows"], batched=True)
    assert "batched=True" in str(e.value)
    assert not list(tmp_path.iterdir())


def test_too_many_samples_or_elements_are_outside_the_envelope(tmp_path, no_device):
    from demethify_amd.bootstrap import batched_ineligible, bt_ci

    V = np.full((20, 65), 0.5)
    D = np.full((20, 65), 3, dtype=np.int64)
    ref = np.full((20, 2), 0.5)
    with pytest.raises(ValueError, match="envelope"):
        bt_ci(90, 4, 1, V, D, ref, "uniform_", 5, 5, 0.0, ["a", "b"], str(tmp_path), [f"s{k}" for k in range(65)], None, 1,
              batched=True)
    assert "envelope" in batched_ineligible(1, 16385, 64, 0, "uniform_", None, UNSUPERVISED)
    # what is eligible: the data-free initialisers, and the silent replacement by uniform_ beyond S unknown types
    assert batched_ineligible(1, 350, 10, 5, "uniform_", None, PARTIAL) is None
    assert batched_ineligible(4, 350, 10, 0, "beta", None, UNSUPERVISED) is None
    assert batched_ineligible(3, 350, 2, 0, "SVD", None, UNSUPERVISED) is None
    assert batched_ineligible(3, 350, 2, 0, "uniform", None, UNSUPERVISED) is None


def test_command_line_refuses_an_unknown_batch_switch(tmp_path):
    samples = [str(UPSTREAM / "output_gen" / f"sample{i}.bed") for i in range(1, 11)]
    proc = subprocess.run([sys.executable, "-m", "demethify_amd", "--ref", str(UPSTREAM / "output_gen" / "ref_matrix.bed"),
                           "--methfreq", *samples, "--bedmethyl", "--nbunknown", "1", "--restart", "4", "--outdir",
                           str(tmp_path / "out"), "--noprint"],
                          cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, DEMETHIFY_BATCH="2"))
    assert proc.returncode == 1, proc.stderr[-2000:]
    assert "DEMETHIFY_BATCH" in proc.stderr and '"2"' in proc.stderr
    assert not (tmp_path / "out").exists()  # before any output, and before any GPU work


class _Stop(Exception):
    pass


def test_without_the_switch_the_call_sequence_is_todays(tmp_path, toy, monkeypatch):
    """batched=False and an unset DEMETHIFY_BATCH: Problem.solve_many is never called, and the loops go where they went --
    bt_ci to a Problem and its per-replicate gathers, the command line's restarts to shard.sharded_restarts."""
    from demethify_amd import bootstrap, demethify, device, shard

    V, D, ref, header = toy
    seen = []
    monkeypatch.setattr(device.Problem, "solve_many", lambda *a, **k: seen.append("solve_many"))

    def problem_init(self, *a, **k):
        seen.append("Problem")
        raise _Stop

    monkeypatch.setattr(device.Problem, "__init__", problem_init)
    monkeypatch.setattr(bootstrap, "get_context", lambda *a: None)
    monkeypatch.setattr(bootstrap.shard, "my_items", lambda *a: [])
    import demethify_amd.staging as staging

    monkeypatch.setattr(staging, "reserve", lambda *a, **k: None)
    samples = [f"s{k}" for k in range(V.shape[1])]
    with pytest.raises(_Stop):
        bootstrap.bt_ci(90, 4, 1, V, D, ref, "uniform_", 5, 5, 0.0, header, str(tmp_path), samples, None, 1)
    assert seen == ["Problem"]

    # the command line, DEMETHIFY_BATCH unset: the restarts reach sharded_restarts, never its batched sibling
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
                        "--noprint", "--nbunknown", "1", "--restart", "4", "--outdir", str(tmp_path / "out")])
    assert seen == ["sharded_restarts"]


def test_batched_restart_pick_keeps_the_first_minimum():
    from demethify_amd import shard

    costs = np.array([3.0, 1.0, 2.0, 1.0, 5.0])

    def solve_many(ks):
        assert ks == [0, 1, 2, 3, 4]
        return np.arange(5.0)[:, None, None] * np.ones((5, 2, 1)), np.arange(5.0)[:, None, None] * np.ones((5, 1, 2)), costs

    u, alpha, best, vec = shard.sharded_restarts_batched(5, solve_many, ((2, 1), (1, 2)))
    assert best == 1 and np.all(u == 1.0) and np.all(alpha == 1.0)
    np.testing.assert_array_equal(vec, costs)
