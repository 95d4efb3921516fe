"""CPU-only tests of the device mask draw's host side: the integer threshold that stands for ``x < fraction``, and the order
in which bicross_validation draws when its device half offers a ``draw`` -- emulated here on the host, where it takes the
global generator's state, calls ``np.random.rand`` itself and packs: the masks, the initialisations and the generator
afterwards must be those of the reference's order (ic.py:59-75), with the skip rule taken on the count alone."""
import numpy as np
import pytest

from oracle import solver as osol


def _fractions():
    x = np.random.RandomState(11).random_sample(3)
    return [0.0, 1.0, 1.5, 2.0 ** -53, 1e-300, 0.3, 1.0 / 3.0, 0.5, float("nan"), -1.0, float(x[1]),
            float(np.nextafter(x[1], 2.0))]


def test_threshold_is_the_compare():
    from demethify_amd.device import mask_threshold

    x = np.random.RandomState(11).random_sample(200000)
    k = (x * 2.0 ** 53).astype(np.uint64)  # (exact: every draw is an integer below 2^53 over 2^53)
    assert np.array_equal(k.astype(np.float64) / 2.0 ** 53, x)
    for f in _fractions():
        T = mask_threshold(f)
        assert isinstance(T, int) and 0 <= T <= 1 << 53, f
        assert np.array_equal(x < f, k < np.uint64(T)), f
    assert mask_threshold(0.3) == 2702159776422298
    assert mask_threshold(float("nan")) == 0 and mask_threshold(-1.0) == 0 and mask_threshold(0.0) == 0
    assert mask_threshold(1.0) == mask_threshold(1.5) == 1 << 53
    assert mask_threshold(2.0 ** -53) == 1 and mask_threshold(1e-300) == 1


def test_entry_point_is_declared_and_bound():
    import re

    from conftest import ROOT
    from demethify_amd import _lib

    header = (ROOT / "include" / "demethify_hip.h").read_text()
    assert re.search(r"\bint\s+dmf_mask_draw\s*\(", header) and "ic.py:68" in header
    assert len(_lib.SIGNATURES["dmf_mask_draw"][1]) == 8


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


class _HostDevice:
    """The device half with a ``draw`` that does on the host what dmf_mask_draw does on the GPU: from the global
    generator's state, the packed mask and its count, the generator left behind the draw."""

    def __init__(self):
        self.draws, self.folds = [], []

    def draw(self, shape, fraction):
        from demethify_amd.device import pack_mask

        state = np.random.get_state()
        assert state[0] == "MT19937" and 0 <= state[2] <= 624
        mask = np.random.rand(*shape) < fraction
        self.draws.append((tuple(shape), fraction))
        return pack_mask(mask), int(mask.sum())

    def __call__(self, fold, best):
        self.folds.append(fold)
        return float(len(self.folds)), (fold[1], fold[2]) if len(self.folds) < best else None


@pytest.mark.parametrize("option", ["uniform_", "beta"])
def test_draw_order_through_the_device_draw(toy, option, monkeypatch):
    from demethify_amd import ic

    V, D, ref, _ = toy
    monkeypatch.setattr(ic, "DEVICE_MASK_MIN_ELEMENTS", 0)
    want = _reference_stream(V, D, ref, 1, option, 1, 4)
    dev = _HostDevice()
    total, best_u, best_alpha = ic.bicross_validation(V, 1, D, 5, 20, 1e-3, n_folds=4, seed=1, ref=ref, init_option=option,
                                                      _fold_solver=dev)
    after = np.random.get_state()
    assert dev.draws == [(V.shape, 0.3)] * 4  # once per fold
    assert len(dev.folds) == len(want) == 4
    for (mask, u0, a0, bits), (wm, wu, wa) in zip(dev.folds, want):
        assert mask is None  # the fold carries no bool mask
        assert bits.dtype == np.uint8 and bits.shape == (V.shape[0], (V.shape[1] + 7) // 8)
        got = np.unpackbits(bits, axis=1, bitorder="little")[:, :V.shape[1]].astype(bool)
        assert np.array_equal(got, wm) and np.array_equal(u0, wu) and np.array_equal(a0, wa)
    assert total == 1.0 + 2.0 + 3.0 + 4.0
    assert np.array_equal(best_u, want[0][1]) and np.array_equal(best_alpha, want[0][2])
    # ... and the generator is where the reference's order leaves it
    _reference_stream(V, D, ref, 1, option, 1, 4)
    ref_after = np.random.get_state()
    assert np.array_equal(after[1], ref_after[1]) and after[2:] == ref_after[2:]


def test_an_initialiser_that_reads_the_data_keeps_the_host_draw(toy, monkeypatch):
    from demethify_amd import ic

    V, D, ref, _ = toy
    monkeypatch.setattr(ic, "DEVICE_MASK_MIN_ELEMENTS", 0)
    want = _reference_stream(V, D, ref, 1, "uniform", 1, 4)
    dev = _HostDevice()
    ic.bicross_validation(V, 1, D, 5, 20, 1e-3, n_folds=4, seed=1, ref=ref, init_option="uniform", _fold_solver=dev)
    assert dev.draws == [] and len(dev.folds) == 4
    for (mask, u0, a0, staged), (wm, wu, wa) in zip(dev.folds, want):
        assert mask.dtype == np.bool_ and staged is None  # the fold carries the bool mask as before
        assert np.array_equal(mask, wm) and np.array_equal(u0, wu) and np.array_equal(a0, wa)


def test_below_the_gate_the_host_draws(toy, monkeypatch):
    from demethify_amd import ic

    V, D, ref, _ = toy
    monkeypatch.setattr(ic, "DEVICE_MASK_MIN_ELEMENTS", V.size + 1)
    want = _reference_stream(V, D, ref, 1, "uniform_", 1, 4)
    dev = _HostDevice()
    ic.bicross_validation(V, 1, D, 5, 20, 1e-3, n_folds=4, seed=1, ref=ref, init_option="uniform_", _fold_solver=dev)
    assert dev.draws == [] and len(dev.folds) == 4
    for (mask, u0, a0, staged), (wm, wu, wa) in zip(dev.folds, want):
        assert staged is None
        assert np.array_equal(mask, wm) and np.array_equal(u0, wu) and np.array_equal(a0, wa)
    monkeypatch.setattr(ic, "DEVICE_MASK_MIN_ELEMENTS", V.size)  # "from N x S elements on"
    dev = _HostDevice()
    ic.bicross_validation(V, 1, D, 5, 20, 1e-3, n_folds=4, seed=1, ref=ref, init_option="uniform_", _fold_solver=dev)
    assert len(dev.draws) == 4


def test_the_shipped_gate_is_an_element_count():
    from demethify_amd import ic

    assert isinstance(ic.DEVICE_MASK_MIN_ELEMENTS, int) and ic.DEVICE_MASK_MIN_ELEMENTS > 0


@pytest.mark.parametrize("fraction", [0.0, 1.5])
def test_skip_rule_is_taken_on_the_count(toy, fraction, monkeypatch):
    from demethify_amd import ic

    V, D, ref, _ = toy
    monkeypatch.setattr(ic, "DEVICE_MASK_MIN_ELEMENTS", 0)
    dev = _HostDevice()
    out = ic.bicross_validation(V, 1, D, 5, 20, 1e-3, n_folds=3, seed=1, ref=ref, fraction=fraction, _fold_solver=dev)
    got_next = np.random.rand()
    assert dev.folds == [] and out == (0, None, None) and len(dev.draws) == 3
    # three masks and nothing else (no initialiser: it would reseed) were drawn after the one seed() call
    np.random.seed(1)
    for _ in range(3):
        np.random.rand(*V.shape)
    assert got_next == np.random.rand()
