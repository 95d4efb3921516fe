"""Host side of the masked batch (no GPU): dmf_solve_small_masked is declared, bound and exported; the shape errors of
Problem.solve_many_masked; the sentences of ic.batched_ic_ineligible on the envelope's edges; that nothing in ic.py reaches
the batch while the switches are off; and that bicross_validation(batched=True) hands solve_many_masked the very masks and
starting points the serial route hands its fold solver, in the reference's draw order."""
import ctypes
import re

import numpy as np
import pytest

from conftest import ROOT, UPSTREAM

PARTIAL, UNSUPERVISED = 0, 1


@pytest.fixture(scope="module", autouse=True)
def _library():
    from demethify_amd import _build

    _build.build()


def test_entry_point_is_declared_bound_and_exported():
    from demethify_amd import _lib

    header = (ROOT / "include" / "demethify_hip.h").read_text()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    name = "dmf_solve_small_masked"
    assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert "ic.py:58-89" in header
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    # dmf_solve_small's arguments with train_bits in idx's place, then the two hold-out outputs
    assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES["dmf_solve_small"][1]) + 2 == 19
    assert _lib.load().dmf_abi_version() == 1  # additive: no signature changed


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was asked for {name}")


def _bare_problem(N=6, S=13, n_c=2):
    from demethify_amd import device

    p = device.Problem.__new__(device.Problem)
    p.N, p.S, p.n_c, p._lib, p._h, p.ctx = N, S, n_c, _NoLibrary(), None, None
    return p


def test_solve_many_masked_refuses_bad_shapes_before_any_device_call():
    p = _bare_problem()
    u0s, a0s = np.full((2, 6, 1), 0.5), np.full((2, 3, 13), 1 / 3)
    good = np.ones((2, 6, 13), dtype=bool)
    bad = [
        (u0s[:, :5], a0s, good, "u0s"), (u0s[0], a0s, good, "u0s"), (u0s, a0s[:1], good, "alpha0s"),
        (u0s, a0s[:, :2], good, "alpha0s"), (u0s, a0s, good[:1], "train_masks"), (u0s, a0s, good[:, :5], "train_masks"),
        (u0s, a0s, good[:, :, :12], "train_masks"), (u0s, a0s, good[0], "train_masks"),
        (u0s, a0s, np.ones((2, 6, 1), dtype=np.uint8), "packed"), (u0s, a0s, np.ones((2, 6, 13), dtype=np.uint8), "packed"),
        (u0s, a0s, np.ones((2, 6, 13)), "bool"), (u0s, a0s, np.ones((2, 6, 2), dtype=np.int64), "bool"),
    ]
    for u, a, m, word in bad:
        with pytest.raises(ValueError, match=word):
            p.solve_many_masked(u, a, m, PARTIAL, 1, 1, 0.0)


def test_packed_masks_round_trip_pack_mask(monkeypatch):
    """Both forms of train_masks reach the library as pack_mask's bytes, one mask after the other (S = 13: two bytes per
    row, three padding bits)."""
    from demethify_amd import _lib as L
    from demethify_amd.device import pack_mask

    masks = np.random.RandomState(4).rand(3, 6, 13) < 0.5
    want = np.stack([pack_mask(m) for m in masks])
    assert want.shape == (3, 6, 2)
    assert np.array_equal(np.unpackbits(want, axis=2, bitorder="little")[:, :, :13].astype(bool), masks)
    seen = []

    class Lib:
        def dmf_solve_small_masked(self, ctx, h, B, bits, *rest):
            seen.append(bytes(ctypes.string_at(bits, B * 6 * 2)))
            return L.DMF_OK

    class Ctx:
        _h = None

    p = _bare_problem()
    p._lib, p.ctx = Lib(), Ctx()
    u0s, a0s = np.full((3, 6, 1), 0.5), np.full((3, 3, 13), 1 / 3)
    out = p.solve_many_masked(u0s, a0s, masks, PARTIAL, 1, 1, 0.0)
    p.solve_many_masked(u0s, a0s, want, PARTIAL, 1, 1, 0.0)
    p.solve_many_masked(u0s, a0s, want[:, :, ::-1][:, :, ::-1], PARTIAL, 1, 1, 0.0)  # (a view is made contiguous)
    assert seen == [want.tobytes()] * 3
    assert [x.shape for x in out] == [(3, 6, 1), (3, 3, 13), (3,), (3,), (3,), (3,)]
    assert out[5].dtype == np.int64 and out[4].dtype == np.float64


def test_batched_ic_ineligible_on_the_edges_of_the_envelope():
    from demethify_amd.ic import batched_ic_ineligible

    for args in [(1, 350, 10, 5, PARTIAL), (4, 350, 10, 0, UNSUPERVISED), (4, 100, 8, 12, PARTIAL), (1, 100, 8, 15, PARTIAL),
                 (1, 100, 64, 2, PARTIAL), (1, 16384, 64, 0, UNSUPERVISED), (1, 1 << 20, 1, 1, PARTIAL)]:
        assert batched_ic_ineligible(*args) is None, args
    for args in [(5, 350, 10, 5, PARTIAL), (5, 100, 8, 0, UNSUPERVISED), (4, 100, 8, 13, PARTIAL), (1, 100, 8, 16, PARTIAL),
                 (1, 100, 65, 2, PARTIAL), (1, 16385, 64, 0, UNSUPERVISED), (1, (1 << 20) + 1, 1, 1, PARTIAL)]:
        reason = batched_ic_ineligible(*args)
        assert "envelope" in reason and f"{args[1]} x {args[2]} with {args[3]} + {args[0]} cell types" in reason, args
        assert "n_u <= 4, K <= 16, S <= 64, N S <= 1048576" in reason
    assert "no unknown cell type" in batched_ic_ineligible(0, 350, 10, 5, PARTIAL)


class _Stop(Exception):
    pass


def test_without_the_switches_ic_never_reaches_the_batch(tmp_path, toy, monkeypatch):
    """batched=False and an unset DEMETHIFY_BATCH: neither solve_many nor solve_many_masked is called from ic.py -- the
    sweeps go to a Solver per solve and the folds to the per-fold route."""
    from demethify_amd import demethify, device, ic

    V, D, ref, _ = toy

    def refuse(*a, **k):
        raise AssertionError("the batch was asked for")

    monkeypatch.setattr(device.Problem, "solve_many", refuse)
    monkeypatch.setattr(device.Problem, "solve_many_masked", refuse)
    monkeypatch.setattr(device.Problem, "__init__", lambda self, *a, **k: None)
    monkeypatch.setattr(device.Problem, "close", lambda self: None)
    monkeypatch.setattr(ic, "get_context", lambda *a: None)
    seen = []

    def solver(*a, **k):
        seen.append("Solver")
        raise _Stop

    monkeypatch.setattr(ic, "Solver", solver)
    import demethify_amd.deconvolution as deconvolution

    monkeypatch.setattr(deconvolution, "Solver", solver)
    for name in ("CCC", "AIC", "BIC"):
        seen.clear()
        with pytest.raises(_Stop):
            ic.evaluate_best_ic(V, ref, D, "uniform_", name, 1, 5, 5, 0.0, n_restarts=2, n_u_values=(1, 2))
        assert seen == ["Solver"]
    folds = []

    def fold_solver(fold, best):
        folds.append(fold)
        return 1.0, (fold[1], fold[2]) if 1.0 < best else None

    ic.bicross_validation(V, 1, D, 5, 5, 0.0, n_folds=2, seed=1, ref=ref, _fold_solver=fold_solver)
    assert len(folds) == 2
    # BCV inside a sweep: the per-fold route (a masked problem per fold), never the batch
    monkeypatch.setattr(device.Problem, "masked", lambda self, bits: (_ for _ in ()).throw(_Stop()))
    monkeypatch.setattr(ic._DeviceFolds, "stage", lambda self, m: type("Bits", (), {"close": lambda s: None})())
    with pytest.raises(_Stop):
        ic.evaluate_best_ic(V, ref, D, "uniform_", "BCV", 1, 5, 5, 0.0, n_restarts=2, n_u_values=(1,))

    # the command line with DEMETHIFY_BATCH unset passes no batched keyword at all
    monkeypatch.delenv("DEMETHIFY_BATCH", raising=False)
    calls = []

    def sweep(*a, **k):
        calls.append(k)
        raise _Stop

    monkeypatch.setattr(ic, "evaluate_best_ic", sweep)
    files = [str(UPSTREAM / "output_gen" / f"sample{i}.bed") for i in range(1, 11)]
    with pytest.raises(_Stop):
        demethify.main(["--ref", str(UPSTREAM / "output_gen" / "ref_matrix.bed"), "--methfreq", *files, "--bedmethyl",
                        "--noprint", "--ic", "BCV", "2", "1", "2", "--outdir", str(tmp_path / "out")])
    assert len(calls) == 1 and "batched" not in calls[0]


class _FakeProblem:
    """Records what bicross_validation(batched=True) passes to solve_many_masked and answers with rising errors."""

    def __init__(self, N, S, n_c):
        self.N, self.S, self.n_c = N, S, n_c
        self.calls = []

    def solve_many_masked(self, u0s, alpha0s, train_masks, mode, n_iter1, n_iter2, tol, iters_per_launch=0):
        first = sum(len(c[0]) for c in self.calls)
        self.calls.append((np.array(u0s), np.array(alpha0s), np.array(train_masks), mode, n_iter1, n_iter2, tol))
        B = len(u0s)
        # fold k (0-based, over all calls) has error 5, 4.5, then 4 from fold 2 on: the first strict minimum is fold 2
        errs = np.array([(10.0 - k) if k < 2 else 8.0 for k in range(first, first + B)])
        return (np.array(u0s) + 1.0, np.array(alpha0s) + 1.0, np.zeros(B), np.ones(B, dtype=np.int64), errs,
                np.full(B, 2, dtype=np.int64))


@pytest.mark.parametrize("option", ["uniform_", "uniform"])
def test_batched_folds_are_the_serial_routes_folds_in_order(toy, option, monkeypatch):
    from demethify_amd import bootstrap, ic

    V, D, ref, _ = toy
    serial = []

    def stub(fold, best):
        serial.append((fold[0].copy(), fold[1].copy(), fold[2].copy()))
        return 1.0, (fold[1], fold[2]) if 1.0 < best else None

    ic.bicross_validation(V, 1, D, 5, 20, 1e-3, n_folds=5, seed=1, ref=ref, init_option=option, _fold_solver=stub)
    assert len(serial) == 5
    after_serial = np.random.rand()
    # chunks of two: the folds arrive in order over three calls
    monkeypatch.setattr(bootstrap, "batch_chunk", lambda n_rows, n_u: 2)
    fake = _FakeProblem(V.shape[0], V.shape[1], ref.shape[1])
    total, best_u, best_alpha = ic.bicross_validation(V, 1, D, 5, 20, 1e-3, n_folds=5, seed=1, ref=ref, init_option=option,
                                                      problem=fake, batched=True)
    assert np.random.rand() == after_serial  # the generator is where the serial route leaves it
    assert [len(c[0]) for c in fake.calls] == [2, 2, 1]
    got = [(m, u0, a0) for c in fake.calls for u0, a0, m in zip(c[0], c[1], c[2])]
    for (m, u0, a0), (wm, wu, wa) in zip(got, serial):
        assert m.dtype == np.bool_ and np.array_equal(m, wm)
        assert np.array_equal(u0, wu.reshape(u0.shape)) and np.array_equal(a0, wa)
    assert all(c[3:] == (PARTIAL, 5, 20, 1e-3) for c in fake.calls)
    # ic.py:80-86 replayed in fold order: the sum of sum_sq / n_test, the first strict minimum (fold 2 of 8, 8, 8) wins
    assert total == (10.0 + 9.0 + 8.0 + 8.0 + 8.0) / 2
    assert np.array_equal(best_u, serial[2][1].reshape(best_u.shape) + 1.0) and np.array_equal(best_alpha, serial[2][2] + 1.0)


def test_batched_folds_with_an_empty_train_or_test_set_are_dropped_without_a_further_draw(toy):
    from demethify_amd import ic

    V, D, ref, _ = toy
    for fraction in (0.0, 1.0):
        fake = _FakeProblem(V.shape[0], V.shape[1], ref.shape[1])
        out = ic.bicross_validation(V, 1, D, 5, 20, 1e-3, n_folds=3, seed=1, ref=ref, fraction=fraction, problem=fake,
                                    batched=True)
        assert fake.calls == [] and out == (0, None, None)
        after = np.random.rand()
        np.random.seed(1)
        for _ in range(3):  # three masks and nothing else were drawn after the one seed() call
            np.random.rand(*V.shape)
        assert np.random.rand() == after


def test_batched_bicross_validation_outside_the_envelope_raises_before_any_device_call(toy, monkeypatch):
    from demethify_amd import device, ic

    V, D, ref, _ = toy
    monkeypatch.setattr(device.Problem, "__init__", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the device")))
    with pytest.raises(ValueError, match="envelope") as e:
        ic.bicross_validation(V, 5, D, 5, 20, 1e-3, n_folds=3, seed=1, ref=ref, batched=True)
    assert "batched=True" in str(e.value)
