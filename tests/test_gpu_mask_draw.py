"""The hold-out mask drawn on the device (dmf_mask_draw): numpy's legacy MT19937 stream continued by the kernel.  numpy on
the host is the oracle and every comparison is for equality: the packed bits against ``pack_mask(np.random.rand(N, S) < f)``
from the same state, the count of ones, the key and position afterwards against ``np.random.get_state()`` after the host
draw, and three further ``np.random.rand()`` values after ``set_state``.

A  shapes: one element, rows that end inside a byte, rows of 311 / 312 / 313 (a regeneration yields 312 doubles), rows longer
   than a regeneration, more doubles than the 2048-bit ring holds many times over
B  start positions: 624 (a fresh seed) and positions inside the key -- the odd ones make a double straddle a regeneration
C  fractions at and beyond both ends, 2^-53 (only an exact zero is below it), 1/3, 0.5
D  refusals leave nothing behind: the next valid call is right
E  the mask feeds Problem.masked like the host's; bicross_validation gives the same with the draw on either side
"""
import ctypes as C

import numpy as np
import pytest

from conftest import load_toy

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (3, 8), (5, 9), (13, 5), (2, 311), (2, 312), (2, 313), (3, 625), (350, 10), (1000, 313),
          (4096, 255), (20000, 256)]
POSITIONS = [624, 0, 1, 311, 312, 313, 622, 623]


def _state_at(pos):
    """The global generator's state with the given position: 624 = right after seed(), else a key taken after 1000 draws."""
    np.random.seed(20240)
    if pos != 624:
        np.random.rand(1000)
        name, key, _, has_gauss, cached = np.random.get_state()
        np.random.set_state((name, key, pos, has_gauss, cached))
    return np.random.get_state()


def _device_draw(ctx, state, N, S, threshold):
    """dmf_mask_draw through the C-ABI -> (status, bits or None, n_kept, key, pos)."""
    key = np.array(state[1], dtype=np.uint32)
    pos, dev, kept = C.c_int(int(state[2])), C.c_void_p(), C.c_int64(-1)
    status = ctx._lib.dmf_mask_draw(ctx._h, key.ctypes.data_as(C.c_void_p), C.byref(pos), N, S, threshold, C.byref(dev),
                                    C.byref(kept))
    if status != 0:
        assert not dev.value  # nothing handed out
        return status, None, kept.value, key, pos.value
    bits = np.full((N, (S + 7) // 8), 0xA5, dtype=np.uint8)  # (a byte the kernel skipped would keep the pattern)
    try:
        assert ctx._lib.dmf_stage_download(ctx._h, dev, bits.nbytes, bits.ctypes.data_as(C.c_void_p)) == 0
    finally:
        assert ctx._lib.dmf_stage_free(ctx._h, dev) == 0
    return status, bits, kept.value, key, pos.value


def _check(ctx, state, N, S, fraction):
    from demethify_amd.device import mask_threshold, pack_mask

    np.random.set_state(state)
    mask = np.random.rand(N, S) < fraction
    after = np.random.get_state()
    next3 = [np.random.rand() for _ in range(3)]
    status, bits, kept, key, pos = _device_draw(ctx, state, N, S, mask_threshold(fraction))
    assert status == 0
    want = pack_mask(mask)
    assert bits.shape == want.shape and np.array_equal(bits, want)
    assert kept == int(mask.sum())
    assert np.array_equal(key, after[1]) and pos == after[2]
    np.random.set_state((state[0], key, pos, state[3], state[4]))
    assert [np.random.rand() for _ in range(3)] == next3


# ---------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes(ctx, shape):
    _check(ctx, _state_at(624), *shape, 0.3)


# ---------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("shape", [(5, 9), (2, 313), (3, 625)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pos", POSITIONS)
def test_start_positions(ctx, pos, shape):
    _check(ctx, _state_at(pos), *shape, 0.3)


# ---------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("shape", [(350, 10), (2, 313)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fraction", [0.0, 1.0, 1.5, 2.0 ** -53, 1.0 / 3.0, 0.5])
def test_fractions(ctx, fraction, shape):
    _check(ctx, _state_at(624), *shape, fraction)


# ---------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("what", ["position_625", "no_rows", "threshold_above_2_53"])
def test_refusals_leave_nothing_behind(ctx, what):
    from demethify_amd import _lib as L
    from demethify_amd.device import mask_threshold

    state = _state_at(1)
    bad_state, N, T = state, 5, mask_threshold(0.3)
    if what == "position_625":
        bad_state = (state[0], state[1], 625, state[3], state[4])
    elif what == "no_rows":
        N = 0
    else:
        T = (1 << 53) + 1
    status, bits, _, key, pos = _device_draw(ctx, bad_state, N, 9, T)
    assert status == L.DMF_ERR_BAD_ARG and bits is None
    assert np.array_equal(key, state[1]) and pos == bad_state[2]  # untouched
    _check(ctx, state, 5, 9, 0.3)


# ---------------------------------------------------------------------------------------------- E
def test_staged_draw_keeps_the_gaussian_cache_and_feeds_problem_masked(ctx):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver
    from demethify_amd.staging import draw_mask
    from oracle import solver as osol

    V, D, Rt, _ = load_toy()
    V, D, Rt = np.ascontiguousarray(V), np.ascontiguousarray(D, dtype=np.int64), np.ascontiguousarray(Rt, dtype=np.float64)
    u0, _, a0 = osol.init_partial("uniform_", V, D, Rt, 1, seed=1)
    np.random.seed(3)
    np.random.randn()  # (leaves a cached Gaussian behind)
    state = np.random.get_state()
    assert state[3] == 1
    mask = np.random.rand(*V.shape) < 0.3
    after = np.random.get_state()
    np.random.set_state(state)
    bits, kept = draw_mask(V.shape, 0.3, ctx)
    got = np.random.get_state()
    assert kept == int(mask.sum()) and bits.packed_mask == (350, 2)
    assert np.array_equal(got[1], after[1]) and got[2:] == after[2:]
    assert np.array_equal(np.unpackbits(bits.to_host(np.uint8), axis=1, bitorder="little")[:, :10].astype(bool), mask)
    results = []
    with Problem(ctx, V, D, Rt) as parent:
        for m in (bits, mask):
            with parent.masked(m) as fold, Solver(fold, u0, a0, L.DMF_MODE_PARTIAL) as s:
                s.step(3, 20, 0.0)
                u, alpha, cost, _ = s.get()
                results.append((s.holdout_error(parent), u, alpha, cost))
    bits.close()
    (err_d, u_d, a_d, c_d), (err_h, u_h, a_h, c_h) = results
    assert err_d == err_h and err_d[1] == int((~mask).sum())
    assert np.array_equal(u_d, u_h) and np.array_equal(a_d, a_h) and c_d == c_h


@pytest.mark.parametrize("with_ref", [True, False], ids=["partial", "unsupervised"])
def test_bicross_validation_is_the_same_with_the_draw_on_either_side(ctx, with_ref, monkeypatch):
    from demethify_amd import ic, staging

    V, D, Rt, _ = load_toy()
    V, D = np.ascontiguousarray(V), np.ascontiguousarray(D, dtype=np.int64)
    ref = np.ascontiguousarray(Rt, dtype=np.float64) if with_ref else None
    calls = []
    real = staging.draw_mask
    monkeypatch.setattr(staging, "draw_mask", lambda *a: calls.append(a[0]) or real(*a))
    out = {}
    for gate in (0, V.size + 1):
        monkeypatch.setattr(ic, "DEVICE_MASK_MIN_ELEMENTS", gate)
        before = len(calls)
        total, u, alpha = ic.bicross_validation(V, 2, D, 5, 20, 1e-3, n_folds=4, seed=1, ref=ref, init_option="uniform_")
        out[gate] = (total, u, alpha, np.random.get_state(), len(calls) - before)
    (t_d, u_d, a_d, s_d, n_d), (t_h, u_h, a_h, s_h, n_h) = out[0], out[V.size + 1]
    assert n_d == 4 and n_h == 0  # the device drew every fold's mask / none
    assert t_d == t_h and np.isfinite(t_d)
    assert u_d.tobytes() == u_h.tobytes() and a_d.tobytes() == a_h.tobytes()
    assert np.array_equal(s_d[1], s_h[1]) and s_d[2:] == s_h[2:]
