"""CPU-only tests of the jump-ahead for numpy's legacy generator (dmf_mt_jump) and of the plan of the segmented mask draw
(dmf_mask_draw_plan).  numpy on the host is the oracle and every comparison is for equality: ``np.random.bytes(4 n)`` consumes
n 32-bit words (confirmed below by the position it leaves), so the key, the position and the next three doubles after a jump
of n words must be those of the generator that walked there.  Beyond what numpy can walk, jumps must compose."""
import ctypes as C

import numpy as np
import pytest

WORDS = [0, 1, 2, 623, 624, 625, 1247, 1248, 19937, 19938, 624 * 40, 10 ** 6 + 3, 2 * 10 ** 7]


def _start(which):
    """A legacy state: a fresh seed (position 624), positions inside a key taken after 1000 draws, or an arbitrary key of
    624 random words -- the low bits of word 0, which are no part of the generator's state, random too -- at position 5."""
    if which == "fresh":
        np.random.seed(20240)
        return np.random.get_state()
    if which == "arbitrary":
        key = np.random.RandomState(99).randint(0, 1 << 32, size=624, dtype=np.uint64).astype(np.uint32)
        assert key[0] & 0x7FFFFFFF not in (0, 0x7FFFFFFF)
        return ("MT19937", key, 5, 0, 0.0)
    np.random.seed(20240)
    np.random.rand(1000)
    name, key, _, has_gauss, cached = np.random.get_state()
    return (name, key, int(which), has_gauss, cached)


STARTS = ["fresh", 0, 1, 311, 623, "arbitrary"]


def _walk(state, n):
    """numpy's own state and next three doubles after n words from ``state`` (n = 0: nothing is drawn)."""
    np.random.set_state(state)
    if n:
        np.random.bytes(4 * n)
    after = np.random.get_state()
    return after, [np.random.rand() for _ in range(3)]


def test_bytes_consumes_one_word_per_four_bytes():
    np.random.seed(5)
    np.random.rand(50)  # position 100
    for n in (1, 3, 17):
        before = np.random.get_state()
        np.random.bytes(4 * n)
        after = np.random.get_state()
        assert after[2] == before[2] + n and np.array_equal(after[1], before[1])


@pytest.mark.parametrize("start", STARTS, ids=str)
def test_jump_is_numpys_walk(start):
    from demethify_amd.device import mt_jump

    state = _start(start)
    for n in WORDS:
        want, next3 = _walk(state, n)
        got = mt_jump(state, n)
        assert np.array_equal(got[1], want[1]) and got[2] == want[2], n
        assert got[0] == "MT19937" and tuple(got[3:]) == tuple(state[3:])
        np.random.set_state(got)
        assert [np.random.rand() for _ in range(3)] == next3, n
    # n = 0 leaves both untouched
    same = mt_jump(state, 0)
    assert np.array_equal(same[1], state[1]) and same[2] == state[2]


@pytest.mark.parametrize("a, b", [(2 ** 33 + 1, 2 ** 20), (2 ** 45, 2 ** 45 + 7), (624 * 2 ** 30, 311)])
@pytest.mark.parametrize("start", ["fresh", 311, "arbitrary"], ids=str)
def test_jumps_compose(start, a, b):
    from demethify_amd.device import mt_jump

    state = _start(start)
    two, one = mt_jump(mt_jump(state, a), b), mt_jump(state, a + b)
    assert np.array_equal(two[1], one[1]) and two[2] == one[2]
    assert not np.array_equal(one[1], state[1])


def test_jump_refuses_and_leaves_the_state():
    from demethify_amd import _lib as L

    lib = L.load()
    state = _start(311)
    key = np.array(state[1], dtype=np.uint32)
    for bad in (-1, 625):
        pos = C.c_int(bad)
        assert lib.dmf_mt_jump(key.ctypes.data_as(C.c_void_p), C.byref(pos), 1000) == L.DMF_ERR_BAD_ARG
        assert pos.value == bad and np.array_equal(key, state[1])
    pos = C.c_int(311)
    assert lib.dmf_mt_jump(None, C.byref(pos), 1000) == L.DMF_ERR_BAD_ARG
    assert lib.dmf_mt_jump(key.ctypes.data_as(C.c_void_p), None, 1000) == L.DMF_ERR_BAD_ARG
    assert pos.value == 311 and np.array_equal(key, state[1])


def test_entry_points_are_declared_and_bound():
    import re

    from conftest import ROOT
    from demethify_amd import _lib

    header = (ROOT / "include" / "demethify_hip.h").read_text()
    for name, n_args in (("dmf_mt_jump", 3), ("dmf_mask_draw_plan", 4), ("dmf_mask_draw_segments", 9)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert len(_lib.SIGNATURES[name][1]) == n_args
    m = re.search(r"#define\s+DMF_MASK_DRAW_MAX_SEGMENTS\s+(\d+)", header)
    assert m and int(m.group(1)) == _lib.MASK_DRAW_MAX_SEGMENTS


def _plan(lib, N, S):
    segments, blocks = C.c_int64(-1), C.c_int64(-1)
    status = lib.dmf_mask_draw_plan(N, S, C.byref(segments), C.byref(blocks))
    return status, segments.value, blocks.value


def test_plan():
    from demethify_amd import _lib as L

    lib = L.load()
    shapes = [(1, 1), (5, 9), (350, 10), (512, 256), (1024, 256), (10_000, 64), (100_000, 64), (1_000_000, 256),
              (3, 2 ** 31 - 1), (2 ** 40, 2 ** 20)]
    for N, S in shapes:
        status, segments, blocks = _plan(lib, N, S)
        assert status == 0 and (status, segments, blocks) == _plan(lib, N, S)  # deterministic
        assert 1 <= segments <= L.MASK_DRAW_MAX_SEGMENTS and blocks >= 1
        assert segments * blocks * 624 >= 2 * N * S + 624
    assert _plan(lib, 1, 1)[1] == 1
    assert _plan(lib, 1_000_000, 256)[1] > 1
    for N, S in [(0, 5), (5, 0), (-1, 5), (5, -3)]:
        assert _plan(lib, N, S)[0] == L.DMF_ERR_BAD_ARG
    assert lib.dmf_mask_draw_plan(5, 9, None, None) == L.DMF_ERR_BAD_ARG
