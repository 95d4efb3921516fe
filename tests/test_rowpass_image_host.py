"""The index map of the row pass's byte images (csrc/dmf_rowpass_image.h, dmf_rowpass_image_offset) -- no GPU involved.

One image holds the 16 rows x 64 samples of a 16-row block and a 64-sample column group in 1024 bytes.  The kernel keeps x in
that order in its ring slot and the counts in its byte count tile, and reads them with three patterns; the LDS has 64 banks of
four bytes, so a wave-wide read of one dword per lane is free of conflicts when its 64 dwords fall into 64 different banks.
A 16-byte read is served in four groups of 16 lanes ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32, as the
comment on the tile swizzle in dmf_kernels_rowpass2.hip records), and each group must touch 64 different banks."""
import numpy as np


def _offsets():
    from demethify_amd import _lib as L

    lib = L.load()
    return np.array([[lib.dmf_rowpass_image_offset(r, s) for s in range(64)] for r in range(16)])


def test_every_row_and_sample_has_a_byte_of_its_own():
    off = _offsets()
    assert sorted(off.ravel().tolist()) == list(range(1024))
    # four consecutive samples are one little-endian dword
    assert (off % 4 == np.arange(64) % 4).all() and (off[:, 0::4] // 4 == off[:, 3::4] // 4).all()
    # ... as the layout is described: rows in the order (row & 3, row >> 2), row r's dwords rotated by 4 (r & 3)
    row, sample = np.meshgrid(np.arange(16), np.arange(64), indexing="ij")
    want = ((4 * (row & 3) + (row >> 2)) * 16 + (((sample >> 2) + 4 * (row & 3)) & 15)) * 4 + (sample & 3)
    assert np.array_equal(off, want)


def test_outside_the_image():
    from demethify_amd import _lib as L

    lib = L.load()
    for row, sample in ((-1, 0), (16, 0), (0, -1), (0, 64)):
        assert lib.dmf_rowpass_image_offset(row, sample) == -1


def test_phase_a_strip_read_touches_64_banks():
    """lane (row m16 = lane & 15, q = lane >> 4) reads the dword of samples 16 t + 4 q .. + 3 of row m16, t = 0..3."""
    dword = _offsets()[:, 0::4] // 4   # [row][dword of the row]
    for t in range(4):
        banks = {int(dword[lane & 15, 4 * t + (lane >> 4)]) % 64 for lane in range(64)}
        assert len(banks) == 64, t


def test_phase_c_read_touches_64_banks():
    """lane (q = lane >> 4, m16 = lane & 15) reads dword m16 of row R + 8 (q & 1) + 4 (q >> 1), R = 0..3: the four rows
    R, R + 4, R + 8, R + 12 are 64 consecutive dwords."""
    dword = _offsets()[:, 0::4] // 4
    for R in range(4):
        got = sorted(int(dword[R + 8 * ((lane >> 4) & 1) + 4 * (lane >> 5), lane & 15]) for lane in range(64))
        assert got == list(range(got[0], got[0] + 64)) and got[0] % 64 == 0, R


def test_integer_product_read_is_one_piece_per_lane_without_conflicts():
    """lane (row m16, q) reads samples 16 q .. 16 q + 15 of row m16 as ONE aligned 16-byte piece; the 16 lanes that a 16-byte
    read serves together touch 16 different pieces modulo 256 bytes (64 banks)."""
    off = _offsets()
    piece = np.empty(64, dtype=int)
    for lane in range(64):
        o = off[lane & 15, 16 * (lane >> 4):16 * (lane >> 4) + 16]
        assert o[0] % 16 == 0 and (o == o[0] + np.arange(16)).all(), lane
        piece[lane] = o[0] // 16
    assert sorted(piece.tolist()) == list(range(64))
    base = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
    for group in base + [[l + 32 for l in g] for g in base]:
        assert len({int(piece[l]) % 16 for l in group}) == 16, group
