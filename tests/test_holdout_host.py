"""CPU-only tests of the hold-out masks: the two C-ABI entry points exist, the bit packing is the documented one, and
bicross_validation draws its masks and initialisations in the reference's order (ic.py:59-75) -- checked through the
seam between its host half (the draws, on a worker thread) and its device half (stubbed here: no GPU)."""
import ctypes
import re

import numpy as np
import pytest

from oracle import solver as osol

from conftest import ROOT


def test_entry_points_are_declared_bound_and_exported():
    from demethify_amd import _build, _lib

    _build.build()
    header = (ROOT / "include" / "demethify_hip.h").read_text()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("dmf_problem_mask", "dmf_solver_holdout_error"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert len(_lib.SIGNATURES["dmf_problem_mask"][1]) == 5
    assert len(_lib.SIGNATURES["dmf_solver_holdout_error"][1]) == 4
    assert _lib.load().dmf_abi_version() == 1  # additive: no signature changed


@pytest.mark.parametrize("S", [1, 7, 8, 9, 13, 64, 65])
def test_pack_mask_round_trips(S):
    from demethify_amd.device import pack_mask

    rs = np.random.RandomState(S)
    mask = rs.rand(37, S) < 0.3
    mask[3], mask[5] = True, False
    bits = pack_mask(mask)
    assert bits.dtype == np.uint8 and bits.shape == (37, (S + 7) // 8) and bits.flags.c_contiguous
    assert np.array_equal(np.unpackbits(bits, axis=1, bitorder="little")[:, :S].astype(bool), mask)
    # sample s is bit (s & 7) of byte (s >> 3); padding bits are zero
    for s in (0, S // 2, S - 1):
        assert np.array_equal((bits[:, s >> 3] >> (s & 7)) & 1, mask[:, s].astype(np.uint8))
    assert not np.unpackbits(bits, axis=1, bitorder="little")[:, S:].any()
    assert np.array_equal(pack_mask(mask.astype(np.float64)), bits)  # 0 / 1 in any dtype


def _reference_stream(V, D, ref, n_u, option, seed, n_folds, fraction=0.3):
    """ic.py:59-75 restated: seed once, then per fold the mask and the initialiser (which reseeds) on the masked arrays."""
    np.random.seed(seed)
    out = []
    for _ in range(n_folds):
        mask = np.random.rand(*V.shape) < fraction
        if np.sum(~mask) == 0 or np.sum(mask) == 0:
            continue
        u0, _, a0 = osol.init_partial(option, V * mask, D * mask, ref, n_u, seed=seed)
        out.append((mask, u0, a0))
    return out


@pytest.mark.parametrize("option", ["uniform_", "uniform"])
def test_draw_order_is_the_references(toy, option):
    from demethify_amd.ic import bicross_validation

    V, D, ref, _ = toy
    want = _reference_stream(V, D, ref, 1, option, 1, 4)
    seen = []

    def stub(fold, best):  # the device half: records what the host half drew, "solves" nothing
        mask, u0, a0, staged = fold
        assert staged is None
        seen.append((mask.copy(), u0.copy(), a0.copy()))
        return float(len(seen)), (u0, a0) if len(seen) < best else None

    total, best_u, best_alpha = bicross_validation(V, 1, D, 5, 20, 1e-3, n_folds=4, seed=1, ref=ref, init_option=option,
                                                   _fold_solver=stub)
    assert len(seen) == len(want) == 4
    for (m, u0, a0), (wm, wu, wa) in zip(seen, want):
        assert np.array_equal(m, wm) and np.array_equal(u0, wu) and np.array_equal(a0, wa)
    # every fold has a non-empty train and test set.  The sizes are those of the restated stream on this fixture: the
    # initialiser's reseed makes folds 1..3 draw one and the same mask, which one depends on how much the initialiser
    # drew (uniform_: u and the Dirichlet proportions; uniform: u alone)
    later = {"uniform_": (1059, 2441), "uniform": (1064, 2436)}[option]
    assert [(int(m.sum()), int((~m).sum())) for m, _, _ in want] == [(1057, 2443)] + [later] * 3
    assert [(int(m.sum()), int((~m).sum())) for m, _, _ in seen] == [(1057, 2443)] + [later] * 3
    # the SUM over the folds, the strict '<' (the first fold wins a tie-free run of rising errors)
    assert total == 1.0 + 2.0 + 3.0 + 4.0
    assert np.array_equal(best_u, want[0][1]) and np.array_equal(best_alpha, want[0][2])


def test_empty_train_or_test_sets_are_skipped_without_drawing_an_initialisation(toy):
    from demethify_amd.ic import bicross_validation

    V, D, ref, _ = toy
    for fraction in (0.0, 1.5):
        calls = []
        out = bicross_validation(V, 1, D, 5, 20, 1e-3, n_folds=3, seed=1, ref=ref, fraction=fraction,
                                 _fold_solver=lambda fold, best: calls.append(fold) or (0.0, None))
        assert calls == [] and out == (0, None, None)
        # three masks and nothing else were drawn after the one seed() call
        np.random.seed(1)
        for _ in range(3):
            np.random.rand(*V.shape)
        want_next = np.random.rand()
        np.random.seed(1)
        bicross_validation(V, 1, D, 5, 20, 1e-3, n_folds=3, seed=1, ref=ref, fraction=fraction,
                           _fold_solver=lambda fold, best: (0.0, None))
        assert np.random.rand() == want_next
