"""Host side of the mid-size batch (no GPU): the envelope of dmf_solve_mid_supported, the plan of dmf_solve_mid_plan, the
kernel="mid" branch of batched_ineligible, the refusals of bt_ci(batched=True, batch_kernel="mid") before any device call,
and the DEMETHIFY_BATCH_MID switch."""
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
    (350, 10, 5, 1, PARTIAL, True), (10000, 64, 12, 4, PARTIAL, True), (1, 1, 0, 1, PARTIAL, True),
    (0, 1, 0, 1, PARTIAL, False), (10, 0, 0, 1, PARTIAL, False),
    (100, 64, 2, 1, PARTIAL, True), (100, 65, 2, 1, PARTIAL, False),                                     # S <= 64
    (100, 8, 12, 4, PARTIAL, True), (100, 8, 13, 4, PARTIAL, False), (100, 8, 15, 1, PARTIAL, True),
    (100, 8, 16, 1, PARTIAL, False),                                                                      # K <= 16
    (100, 8, 3, 0, PARTIAL, False), (100, 8, 0, 4, UNSUPERVISED, True), (100, 8, 0, 5, UNSUPERVISED, False),  # 1 <= n_u <= 4
    (1 << 17, 64, 0, 1, PARTIAL, True), ((1 << 17) + 1, 64, 0, 1, PARTIAL, False),                        # N S <= 2^23
    (1 << 23, 1, 1, 1, PARTIAL, True), ((1 << 23) + 1, 1, 1, 1, PARTIAL, False),
    (100, 8, 2, 1, 2, False), (100, 8, 2, 1, -1, False), (100, 8, -1, 2, PARTIAL, False),                  # modes, a negative n_c
])
def test_envelope_of_mid_solve_supported(N, S, n_c, n_u, mode, want):
    from demethify_amd import _lib as L
    from demethify_amd.device import mid_solve_supported

    assert mid_solve_supported(N, S, n_c, n_u, mode) is want
    assert (L.MID_MAX_S, L.MID_MAX_K, L.MID_MAX_NU, L.MID_MAX_ELEMENTS) == (64, 16, 4, 1 << 23)
    assert ((1 << 17) + 1) * 64 == (1 << 23) + 64


def test_plan_covers_the_rows_with_at_most_64_slabs():
    from demethify_amd.device import mid_solve_plan, mid_solve_supported

    seen = 0
    for S in (1, 3, 10, 16, 33, 64):
        for N in (1, 255, 256, 257, 350, 1000, 10000, 16384, 16385, 32768, 100003, 131072, (1 << 23) // S):
            if not mid_solve_supported(N, S, 2, 1, PARTIAL):
                continue
            rows, W, every = mid_solve_plan(N, S)
            assert rows > 0 and rows % 256 == 0
            assert (W - 1) * rows < N <= W * rows
            assert 1 <= W <= 64
            assert every >= 1
            assert (rows, W, every) == mid_solve_plan(N, S, 0)
            seen += 1
    assert seen > 60
    assert mid_solve_plan(10000, 64)[:2] == (256, 40)  # the default: as many slabs as the envelope allows
    assert mid_solve_plan(131072, 64)[:2] == (2048, 64)


@pytest.mark.parametrize("N,rows,W", [(350, 256, 2), (700, 256, 3), (257, 256, 2), (256, 256, 1), (350, 512, 1), (1000, 512, 2)])
def test_plan_with_explicit_rows(N, rows, W):
    from demethify_amd.device import mid_solve_plan

    got = mid_solve_plan(N, 10, rows)
    assert got[:2] == (rows, W)
    assert got[2] == mid_solve_plan(N, 10)[2]  # check_every does not depend on the rows


@pytest.mark.parametrize("N,S,rows", [(350, 10, 255), (350, 10, 100), (350, 10, -256), (350, 10, 384), (16385, 8, 256),
                                      (0, 10, 0), (350, 0, 0), (-5, 10, 256)])
def test_plan_refuses_bad_values(N, S, rows):
    from demethify_amd import _lib as L
    from demethify_amd.device import mid_solve_plan
    import ctypes as C

    with pytest.raises(ValueError):
        mid_solve_plan(N, S, rows)
    out = [C.c_int64(-7) for _ in range(3)]
    assert L.load().dmf_solve_mid_plan(N, S, rows, *[C.byref(o) for o in out]) == L.DMF_ERR_BAD_ARG
    assert [o.value for o in out] == [-7, -7, -7]


def bootstrap_gate():
    from demethify_amd import bootstrap

    return bootstrap.SMALL_BATCH_MAX_ELEMENTS


def test_batched_ineligible_for_the_mid_kernel():
    from demethify_amd.bootstrap import batched_ineligible

    # 10 000 x 64 with 12 + 4 types is eligible.  (6.4e5 elements are inside the one-launch batch's envelope of 2^20 as well --
    # what keeps the command line from it there is the measured gate, not the envelope.)  32 768 x 64 is where the default
    # kernel says "envelope" and the mid-size one takes the case.
    assert batched_ineligible(4, 10000, 64, 12, "uniform_", None, PARTIAL, kernel="mid") is None
    assert batched_ineligible(4, 10000, 64, 12, "uniform_", None, PARTIAL) is None
    assert 10000 * 64 > bootstrap_gate()
    assert "envelope" in batched_ineligible(4, 32768, 64, 12, "uniform_", None, PARTIAL)
    assert batched_ineligible(4, 32768, 64, 12, "uniform_", None, PARTIAL, kernel="mid") is None
    assert batched_ineligible(4, 10000, 64, 12, "uniform_", [], PARTIAL, kernel="mid") is None
    for purity_batched in (False, True):
        assert batched_ineligible(1, 350, 10, 5, "uniform_", [80.0] * 10, PARTIAL, purity_batched=purity_batched,
                                  kernel="mid") == "the purity-constrained alpha phase is not part of the mid-size batch"
    # its own envelope, and every other reason as for the default kernel
    assert "envelope" in batched_ineligible(1, (1 << 17) + 1, 64, 0, "uniform_", None, UNSUPERVISED, kernel="mid")
    assert "envelope" in batched_ineligible(5, 350, 10, 0, "uniform_", None, UNSUPERVISED, kernel="mid")
    assert "no unknown cell type" in batched_ineligible(0, 350, 10, 5, "uniform_", None, PARTIAL, kernel="mid")
    assert "_observe" in batched_ineligible(1, 350, 10, 5, "uniform_", None, PARTIAL, observe=print, kernel="mid")
    assert "aligning" in batched_ineligible(2, 350, 10, 5, "uniform_", None, PARTIAL, align=True, kernel="mid")
    assert "cpg" in batched_ineligible(1, 350, 10, 5, "uniform_", None, PARTIAL, profile_rows="cpg", kernel="mid")
    assert "reads the resampled data" in batched_ineligible(1, 350, 10, 5, "uniform", None, PARTIAL, kernel="mid")
    with pytest.raises(ValueError, match="kernel"):
        batched_ineligible(1, 350, 10, 5, "uniform_", None, PARTIAL, kernel="large")


def test_batched_ineligible_with_the_default_kernel_is_unchanged():
    """The cases of tests/test_small_batch_host.py: kernel="small" and no kernel argument give the same sentence, the one
    those tests pin."""
    from demethify_amd.bootstrap import batched_ineligible

    cases = [  # (arguments, keyword arguments, a word of the reason or None)
        ((0, 350, 10, 5, "uniform_", None, PARTIAL), {}, "no unknown cell type"),
        ((1, 350, 10, 5, "uniform_", [80.0] * 10, PARTIAL), {}, "purity"),
        ((1, 350, 10, 5, "uniform_", [80.0] * 10, PARTIAL), {"purity_batched": True}, None),
        ((1, 350, 10, 0, "uniform_", [80.0] * 10, UNSUPERVISED), {"purity_batched": True}, "no known block"),
        ((1, 350, 10, 5, "uniform_", None, PARTIAL), {"observe": print}, "_observe"),
        ((2, 350, 10, 5, "uniform_", None, PARTIAL), {"align": True}, "aligning"),
        ((1, 350, 10, 5, "uniform_", None, PARTIAL), {"profile_rows": "cpg"}, "cpg"),
        ((1, 350, 10, 5, "uniform", None, PARTIAL), {}, "reads the resampled data"),
        ((1, 350, 10, 5, "SVD", None, PARTIAL), {}, "reads the resampled data"),
        ((5, 350, 10, 5, "uniform_", None, PARTIAL), {}, "envelope"),
        ((4, 350, 10, 13, "uniform_", None, PARTIAL), {}, "envelope"),
        ((1, 16385, 64, 0, "uniform_", None, UNSUPERVISED), {}, "batched kernel's envelope"),
        ((1, 350, 10, 5, "uniform_", None, PARTIAL), {}, None),
        ((4, 350, 10, 0, "beta", None, UNSUPERVISED), {}, None),
        ((3, 350, 2, 0, "SVD", None, UNSUPERVISED), {}, None),
        ((3, 350, 2, 0, "uniform", None, UNSUPERVISED), {}, None),
    ]
    for args, kw, word in cases:
        plain = batched_ineligible(*args, **kw)
        assert plain == batched_ineligible(*args, kernel="small", **kw)
        if word is None:
            assert plain is None
        else:
            assert word in plain and "mid-size" not in plain


def test_mid_batch_chunk_keeps_workspace_and_stack_within_256_mb():
    from demethify_amd.bootstrap import mid_batch_chunk
    from demethify_amd.device import mid_solve_plan

    for N, S, n_c, n_u in [(350, 10, 5, 1), (10000, 64, 12, 4), (10000, 64, 6, 2), (131072, 64, 12, 4), (1 << 23, 1, 0, 4),
                           (131072, 64, 15, 1)]:
        chunk = mid_batch_chunk(N, S, n_c, n_u)
        W = mid_solve_plan(N, S)[1]
        K = n_c + n_u
        known = n_c * (n_c + 1) // 2 + n_c
        jobs = max(known, K * (K + 1) // 2 + K - known)
        per_solve = 8 * (W * jobs * S + N * n_u)
        assert 1 <= chunk <= 1024
        assert chunk == 1 or chunk * per_solve <= 1 << 28
        assert chunk == 1024 or (chunk + 1) * per_solve > 1 << 28


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
    "purity": (dict(purity=[80.0] * 10), "not part of the mid-size batch"),
    "an observer": (dict(_observe=lambda *a: None), "_observe"),
    "alignment": (dict(n_u=2, align_unknown=True), "aligning"),
    "rows by CpG": (dict(profile_rows="cpg"), "cpg"),
    "uniform reads the data": (dict(init_option="uniform"), "reads the resampled data"),
    "too many unknown types": (dict(n_u=5), "mid-size batch's envelope"),
}


@pytest.mark.parametrize("name", sorted(INELIGIBLE))
def test_ineligible_mid_bootstrap_raises_before_any_device_call(tmp_path, toy, no_device, name):
    from demethify_amd.bootstrap import bt_ci

    V, D, ref, header = toy
    change, word = INELIGIBLE[name]
    kw = dict(n_u=1, ref=ref, init_option="uniform_", purity=None, _observe=None, align_unknown=None, profile_rows="position")
    kw.update(change)
    samples = [f"s{k}" for k in range(V.shape[1])]
    for batched_purity in (False, True):  # (the small kernel's purity switch opens nothing here)
        with pytest.raises(ValueError, match=word) as e:
            bt_ci(90, 4, kw["n_u"], V, D, kw["ref"], kw["init_option"], 5, 5, 0.0, header, str(tmp_path), samples, kw["purity"], 1,
                  _observe=kw["_observe"], align_unknown=kw["align_unknown"], profile_rows=kw["profile_rows"], batched=True,
                  batched_purity=batched_purity, batch_kernel="mid")
        assert 'batch_kernel="mid"' in str(e.value)
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("batched", [False, True])
def test_an_unknown_batch_kernel_raises(tmp_path, toy, no_device, batched):
    from demethify_amd.bootstrap import bt_ci

    V, D, ref, header = toy
    with pytest.raises(ValueError, match="batch_kernel"):
        bt_ci(90, 4, 1, V, D, ref, "uniform_", 5, 5, 0.0, header, str(tmp_path), [f"s{k}" for k in range(V.shape[1])], None, 1,
              batched=batched, batch_kernel="large")
    assert not list(tmp_path.iterdir())


def test_command_line_refuses_an_unknown_mid_batch_switch(tmp_path):
    samples = [str(UPSTREAM / "output_gen" / f"sample{i}.bed") for i in range(1, 11)]
    proc = subprocess.run([sys.executable, "-m", "demethify_amd", "--ref", str(UPSTREAM / "output_gen" / "ref_matrix.bed"),
                           "--methfreq", *samples, "--bedmethyl", "--nbunknown", "1", "--restart", "4", "--outdir",
                           str(tmp_path / "out"), "--noprint"],
                          cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, DEMETHIFY_BATCH_MID="2"))
    assert proc.returncode == 1, proc.stderr[-2000:]
    assert "DEMETHIFY_BATCH_MID" in proc.stderr and '"2"' in proc.stderr
    assert not (tmp_path / "out").exists()  # before any output, and before any GPU work


class _Stop(Exception):
    pass


def test_command_line_routes_restarts_through_the_mid_batch_inside_the_gate_only(tmp_path, toy, monkeypatch, capsys):
    """DEMETHIFY_BATCH_MID=1 --restart 4 on the toy: with the gate moved away from the toy's size a note names the reason
    and the restarts reach shard.sharded_restarts; with the gate opened around the toy's size they reach
    sharded_restarts_batched and Problem.solve_many_mid."""
    from demethify_amd import bootstrap, demethify, device, shard

    V = toy[0]
    seen = []
    monkeypatch.delenv("DEMETHIFY_BATCH", raising=False)
    monkeypatch.setenv("DEMETHIFY_BATCH_MID", "1")
    monkeypatch.setattr(device.Problem, "__init__", lambda self, *a, **k: None)
    monkeypatch.setattr(device.Problem, "close", lambda self: None)
    monkeypatch.setattr(device, "get_context", lambda *a: None)
    import demethify_amd.staging as staging

    monkeypatch.setattr(staging, "reserve", lambda *a, **k: None)

    def restarts(*a, **k):
        seen.append("sharded_restarts")
        raise _Stop

    def solve_many_mid(self, u0s, a0s, *a, **k):
        seen.append(("solve_many_mid", len(u0s)))
        raise _Stop

    monkeypatch.setattr(shard, "sharded_restarts", restarts)
    monkeypatch.setattr(device.Problem, "solve_many_mid", solve_many_mid)
    monkeypatch.setattr(device.Problem, "solve_many", lambda *a, **k: seen.append("solve_many"))
    files = [str(UPSTREAM / "output_gen" / f"sample{i}.bed") for i in range(1, 11)]
    argv = ["--ref", str(UPSTREAM / "output_gen" / "ref_matrix.bed"), "--methfreq", *files, "--bedmethyl", "--noprint",
            "--nbunknown", "1", "--restart", "4", "--outdir", str(tmp_path / "out")]

    monkeypatch.setattr(bootstrap, "MID_BATCH_MIN_ELEMENTS", V.size + 1)
    monkeypatch.setattr(bootstrap, "MID_BATCH_MAX_ELEMENTS", 10 * V.size)
    with pytest.raises(_Stop):
        demethify.main(argv)
    assert seen == ["sharded_restarts"]
    assert "DEMETHIFY_BATCH_MID=1 is not used for --restart" in capsys.readouterr().out

    seen.clear()
    monkeypatch.setattr(bootstrap, "MID_BATCH_MIN_ELEMENTS", V.size)
    with pytest.raises(_Stop):
        demethify.main(argv)
    assert seen == [("solve_many_mid", 4)]
    assert "is not used" not in capsys.readouterr().out

    # --purity is not wired: the note gives the sentence, the per-solve path runs
    seen.clear()
    with pytest.raises(_Stop):
        demethify.main(argv + ["--purity", *["80"] * 10])
    assert seen == ["sharded_restarts"]
    assert "not part of the mid-size batch" in capsys.readouterr().out
