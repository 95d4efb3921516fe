"""The hold-out mask drawn by one workgroup per segment of numpy's MT19937 stream (dmf_mask_draw_segments): the segments'
keys come from the caller's by polynomial jump-ahead on the device, and every byte of the mask is written by exactly one
workgroup.  numpy on the host is the oracle and every comparison is for equality, as in test_gpu_mask_draw.py: the packed
bits (downloaded into a buffer pre-filled with 0xA5, so that an unwritten byte shows), the count of ones, the key and position
afterwards, and three further ``np.random.rand()`` values after ``set_state``.

A  seams: segments of 1, 2, 3 and 5 blocks over shapes whose rows end inside bytes, are longer than a block or than several
   segments, with segment ends inside bytes
B  start positions: the odd ones make a double straddle a segment seam
C  fractions at and beyond both ends
D  many segments, not a power of two
E  the plan's own choice through dmf_mask_draw, against the one-workgroup kernel
F  refusals leave nothing behind
G  through staging.draw_mask and ic.bicross_validation
"""
import ctypes as C

import numpy as np
import pytest

from conftest import load_toy

pytestmark = pytest.mark.gpu

SEAM_SHAPES = [(1, 1), (5, 9), (13, 5), (40, 100), (2, 313), (3, 625), (1, 5000), (350, 10), (257, 77)]
POSITIONS = [624, 0, 1, 311, 312, 313, 622, 623]


def _state_at(pos):
    """The global generator's state with the given position: 624 = right after seed(), else a key taken after 1000 draws."""
    np.random.seed(20240)
    if pos != 624:
        np.random.rand(1000)
        name, key, _, has_gauss, cached = np.random.get_state()
        np.random.set_state((name, key, pos, has_gauss, cached))
    return np.random.get_state()


_oracle_cache = {}


def _oracle(state, N, S, fraction):
    """numpy's draw from ``state``: (packed bits, ones, state after, next three doubles); computed once per case."""
    from demethify_amd.device import pack_mask

    k = (int(state[2]), N, S, fraction)
    if k not in _oracle_cache:
        np.random.set_state(state)
        mask = np.random.rand(N, S) < fraction
        after = np.random.get_state()
        next3 = [np.random.rand() for _ in range(3)]
        want = pack_mask(mask)
        want.setflags(write=False)
        _oracle_cache[k] = (want, int(mask.sum()), after, next3)
    return _oracle_cache[k]


def _device_draw(ctx, state, N, S, threshold, blocks_per_segment, plain=False):
    """dmf_mask_draw_segments (plain: dmf_mask_draw) through the C-ABI -> (status, bits or None, n_kept, key, pos)."""
    key = np.array(state[1], dtype=np.uint32)
    pos, dev, kept = C.c_int(int(state[2])), C.c_void_p(), C.c_int64(-1)
    if plain:
        status = ctx._lib.dmf_mask_draw(ctx._h, key.ctypes.data_as(C.c_void_p), C.byref(pos), N, S, threshold, C.byref(dev),
                                        C.byref(kept))
    else:
        status = ctx._lib.dmf_mask_draw_segments(ctx._h, key.ctypes.data_as(C.c_void_p), C.byref(pos), N, S, threshold,
                                                 blocks_per_segment, C.byref(dev), C.byref(kept))
    if status != 0:
        assert not dev.value  # nothing handed out
        return status, None, kept.value, key, pos.value
    bits = np.full((N, (S + 7) // 8), 0xA5, dtype=np.uint8)  # (a byte the kernel skipped would keep the pattern)
    try:
        assert ctx._lib.dmf_stage_download(ctx._h, dev, bits.nbytes, bits.ctypes.data_as(C.c_void_p)) == 0
    finally:
        assert ctx._lib.dmf_stage_free(ctx._h, dev) == 0
    return status, bits, kept.value, key, pos.value


def _check(ctx, state, N, S, fraction, blocks_per_segment, plain=False):
    from demethify_amd.device import mask_threshold

    want, ones, after, next3 = _oracle(state, N, S, fraction)
    status, bits, kept, key, pos = _device_draw(ctx, state, N, S, mask_threshold(fraction), blocks_per_segment, plain)
    assert status == 0
    assert bits.shape == want.shape and np.array_equal(bits, want)
    assert kept == ones
    assert np.array_equal(key, after[1]) and pos == after[2]
    np.random.set_state((state[0], key, pos, state[3], state[4]))
    assert [np.random.rand() for _ in range(3)] == next3


def _segments(N, S, blocks_per_segment):
    blocks = (2 * N * S + 624 + 623) // 624
    return (blocks + blocks_per_segment - 1) // blocks_per_segment


# ---------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("shape", SEAM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("blocks_per_segment", [1, 2, 3, 5])
def test_seams(ctx, blocks_per_segment, shape):
    _check(ctx, _state_at(624), *shape, 0.3, blocks_per_segment)


# ---------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("shape", [(5, 9), (2, 313), (3, 625), (40, 100)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("blocks_per_segment", [1, 2])
@pytest.mark.parametrize("pos", POSITIONS)
def test_start_positions(ctx, pos, blocks_per_segment, shape):
    _check(ctx, _state_at(pos), *shape, 0.3, blocks_per_segment)


# ---------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("fraction", [0.0, 1.0, 1.5, 2.0 ** -53, 1.0 / 3.0, 0.5])
def test_fractions(ctx, fraction):
    _check(ctx, _state_at(624), 350, 10, fraction, 1)


# ---------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("shape, blocks_per_segment, segments", [((1000, 313), 3, 335), ((4096, 255), 7, 479)],
                         ids=["1000x313_by_3", "4096x255_by_7"])
def test_many_segments(ctx, shape, blocks_per_segment, segments):
    from demethify_amd import _lib as L

    assert _segments(*shape, blocks_per_segment) == segments <= L.MASK_DRAW_MAX_SEGMENTS
    _check(ctx, _state_at(624), *shape, 0.3, blocks_per_segment)
    _check(ctx, _state_at(313), *shape, 0.3, blocks_per_segment)


# ---------------------------------------------------------------------------------------------- E
def _smallest_planned_shape(lib):
    for k in range(0, 26):
        segments, blocks = C.c_int64(), C.c_int64()
        assert lib.dmf_mask_draw_plan(1 << k, 256, C.byref(segments), C.byref(blocks)) == 0
        if segments.value >= 2:
            return (1 << k, 256), segments.value, blocks.value
    return None, 0, 0


def test_the_plans_own_choice(ctx):
    shape, segments, blocks = _smallest_planned_shape(ctx._lib)
    assert shape is not None and shape[0] * shape[1] <= 1 << 25  # a draw of seconds would mean the plan is wrong
    assert segments >= 2
    for pos in (624, 311):
        state = _state_at(pos)
        _check(ctx, state, *shape, 0.3, 0, plain=True)  # dmf_mask_draw: the plan's segments
        _check(ctx, state, *shape, 0.3, 0)              # ... and the same asked for by 0
        _check(ctx, state, *shape, 0.3, -1)             # the one-workgroup kernel


# ---------------------------------------------------------------------------------------------- F
@pytest.mark.parametrize("what", ["too_many_segments", "position_625", "no_rows", "below_minus_one"])
def test_refusals_leave_nothing_behind(ctx, what):
    from demethify_amd import _lib as L
    from demethify_amd.device import mask_threshold

    state = _state_at(1)
    bad_state, N, S, c = state, 5, 9, 1
    if what == "too_many_segments":
        N, S, c = 4096, 255, 3  # 1117 segments
        assert _segments(N, S, c) > L.MASK_DRAW_MAX_SEGMENTS >= _segments(N, S, c + 1)
    elif what == "position_625":
        bad_state = (state[0], state[1], 625, state[3], state[4])
    elif what == "no_rows":
        N = 0
    else:
        c = -2
    status, bits, _, key, pos = _device_draw(ctx, bad_state, N, S, mask_threshold(0.3), c)
    assert status == L.DMF_ERR_BAD_ARG and bits is None
    assert np.array_equal(key, state[1]) and pos == bad_state[2]  # untouched
    _check(ctx, state, 5, 9, 0.3, 1)
    if what == "too_many_segments":
        _check(ctx, _state_at(624), N, S, 0.3, c + 1)  # the smallest length that fits


# ---------------------------------------------------------------------------------------------- G
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
    bits, kept = draw_mask(V.shape, 0.3, ctx, blocks_per_segment=1)
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
def test_bicross_validation_is_the_same_with_the_segmented_draw(ctx, with_ref, monkeypatch):
    from demethify_amd import ic, staging

    V, D, Rt, _ = load_toy()
    V, D = np.ascontiguousarray(V), np.ascontiguousarray(D, dtype=np.int64)
    ref = np.ascontiguousarray(Rt, dtype=np.float64) if with_ref else None
    calls = []
    real = staging.draw_mask
    monkeypatch.setattr(staging, "draw_mask", lambda *a: calls.append(a[0]) or real(*a, blocks_per_segment=1))
    out = {}
    for gate in (0, V.size + 1):
        monkeypatch.setattr(ic, "DEVICE_MASK_MIN_ELEMENTS", gate)
        before = len(calls)
        total, u, alpha = ic.bicross_validation(V, 2, D, 5, 20, 1e-3, n_folds=4, seed=1, ref=ref, init_option="uniform_")
        out[gate] = (total, u, alpha, np.random.get_state(), len(calls) - before)
    (t_d, u_d, a_d, s_d, n_d), (t_h, u_h, a_h, s_h, n_h) = out[0], out[V.size + 1]
    assert n_d == 4 and n_h == 0  # the segmented draw made every fold's mask / none
    assert t_d == t_h and np.isfinite(t_d)
    assert u_d.tobytes() == u_h.tobytes() and a_d.tobytes() == a_h.tobytes()
    assert np.array_equal(s_d[1], s_h[1]) and s_d[2:] == s_h[2:]
