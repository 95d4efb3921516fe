"""The byte form of the row pass's deferred-C schedule (dmf_context_set_rowpass_bytes) against the u16 form it replaces.

A problem that can run the deferred-C schedule at all (X16, every count <= 255, 193 <= S <= 256) carries byte images X8 / D8 of
its X16 / D16, laid out per 16-row block and 64-sample column group in the order the kernel's LDS holds them
(csrc/dmf_rowpass_image.h).  With the switch on, k_rowpass_v2<.., BYTES> streams one byte per element of x and of the counts
instead of two.  Every sum stays on its wave and in its order, so the results must agree bit for bit.

Each case creates the same problem and solver twice in one process, with the switch on and off, on the seeded inputs and the
shapes of tests/test_gpu_rowpass_defer_c.py (the smallest that reach a lone block, a pair and a lone block, the ring's wrap-around
and the drain with one and with two pairs pending), and runs two outer iterations.  The launch counter must show the byte form
for every deferred launch with the switch on, and for none with it off or where the problem has no images.

The images themselves are read back and compared byte for byte, padding included, with a numpy re-layout of the X16 / D16 read
back from the same problem: created, masked (the images must carry the masked counts) and gathered."""
import numpy as np
import pytest

import rowpass_schedule_model as model
from test_gpu_rowpass_defer_c import K_ITERS, _gather_idx, _inputs, _mask, _rows

pytestmark = pytest.mark.gpu


def _run(ctx, V, D, Rt, u0, a0, n_iter2, rowpass_bytes, x16=True, derive=None):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem, Solver

    mode = L.DMF_MODE_PARTIAL if Rt is not None else L.DMF_MODE_UNSUPERVISED
    ctx.set_x16(x16)
    ctx.set_rowpass_bytes(rowpass_bytes)
    try:
        with Problem(ctx, V, D, Rt) as full:
            p = derive(full) if derive is not None else full
            try:
                with Solver(p, u0, a0, mode) as s:
                    desc = s.describe(n_iter2)
                    word = model.schedule_in_text(s.u_phase_describe(n_iter2))  # the plan's schedule, before any launch
                    s.step(K_ITERS, n_iter2, 0.0)
                    u, alpha = s.get()[:2]
                    mom = s.momentum_state()
                    gram = s.gram("last")[0]
                    out = {"u": u, "alpha": alpha, "u_prev": mom["u_prev"], "alpha_prev": mom["alpha_prev"], "gram": gram,
                           "direct_cost": np.float64(s.direct_cost())}
                    counts = s.rowpass_schedule_counts() + (s.rowpass_byte_launches(),)
                    assert counts == model.expected_counts(word, counts[0]), (word, counts)  # ... is what the launches ran
                    return out, desc, counts[:3], counts[3], p.has_byte_images()
            finally:
                if p is not full:
                    p.close()
    finally:
        ctx.set_rowpass_bytes(True)
        ctx.set_x16(True)


# (blocks, off, (nk lo, nk hi), S, n_c, n_u, n_iter2, (lo, hi, n_top), set-up, takes the byte form, why)
CASES = [
    (812, 5, (1, 2), 256, 12, 4, 20, (1, 255, 64), None, True, "lone block / one pair; x = 255; two digit planes"),
    (1224, 3, (2, 3), 193, 0, 1, 3, (1, 100, 8), None, True, "ragged fourth wave; unsupervised"),
    (1636, 7, (3, 4), 255, 1, 2, 7, (128, 255, 64), None, True, "odd S, odd step count, counts in 128..255"),
    (2125, 1, (4, 5), 256, 16, 2, 20, (1, 120, 8), None, True, "ring wrap; drain with one and two pairs; one plane"),
    (3322, 9, (6, 7), 256, 12, 4, 20, (1, 200, 64), None, True, "six and seven blocks; the bench's kernel instance"),
    (300, 11, (1, 1), 256, 0, 4, 20, (1, 60, 8), None, True, "every workgroup a lone block; unsupervised, 4 unknowns"),
    (1224, 3, (2, 3), 256, 12, 4, 20, (1, 256, 64), None, False, "largest count 256: the pair schedule, no images"),
    (1224, 3, (2, 3), 192, 12, 4, 20, (1, 100, 8), None, False, "S = 192, three waves: the pair schedule, no images"),
    (1224, 3, (2, 3), 256, 12, 4, 20, (1, 100, 8), "no_x16", False, "no X16: the V form, no images"),
    (1636, 7, (3, 4), 256, 12, 4, 20, (1, 255, 64), "masked", True, "a masked problem"),
    (1636, 7, (3, 4), 256, 12, 2, 20, (1, 255, 64), "gathered", True, "a gathered problem"),
]


@pytest.mark.parametrize("blocks,off,nk,S,n_c,n_u,n_iter2,counts,setup,takes,why", CASES)
def test_byte_form_is_bit_identical(ctx, blocks, off, nk, S, n_c, n_u, n_iter2, counts, setup, takes, why):
    N = _rows(blocks, off)
    assert N % 16 != 0
    V, D, Rt, u0, a0 = _inputs(N, S, n_c, n_u, counts, seed=blocks + S)
    derive, x16, n_rows = None, True, N
    if setup == "masked":
        derive = lambda p: p.masked(_mask(N, S))
    elif setup == "gathered":
        idx = _gather_idx(N)
        derive, n_rows = (lambda p: p.gather(idx)), idx.size
        u0 = u0[:n_rows].copy()
    elif setup == "no_x16":
        x16 = False
    assert model.blocks_per_workgroup(n_rows, S) == nk, (why, model.blocks_per_workgroup(n_rows, S))
    # the byte form runs exactly where the deferred-C schedule does
    assert model.runs_deferred(S, n_c, n_u, n_iter2, counts[1], x16=x16) == takes, why

    on, d_on, c_on, b_on, img_on = _run(ctx, V, D, Rt, u0, a0, n_iter2, True, x16, derive)
    off_, d_off, c_off, b_off, img_off = _run(ctx, V, D, Rt, u0, a0, n_iter2, False, x16, derive)
    assert "k_rowpass_v2" in d_on and d_on == d_off, (d_on, d_off)
    assert c_on[0] >= K_ITERS and c_on == c_off, (why, c_on, c_off)   # the same schedule either way
    assert c_on[2] == (c_on[0] if takes else 0), (why, c_on)
    assert b_on == c_on[2], (why, b_on, c_on)                         # every deferred launch read the images
    assert b_off == 0, (why, b_off)
    assert img_on == img_off == takes, (why, img_on, img_off)         # the images belong to the problem, not to the switch
    for name in ("u", "u_prev", "alpha_prev", "alpha", "gram", "direct_cost"):
        assert np.array_equal(on[name], off_[name]), (why, name)
    assert np.isfinite(on["u"]).all() and np.isfinite(on["gram"]).all() and np.isfinite(on["direct_cost"])


# ------------------------------------------------------------------------------------------------- the images, read back
def _image_offsets():
    """[row, sample] -> byte within a 1024-byte image, written from the layout's description alone (csrc/dmf_rowpass_image.h):
    rows in the order (row & 3, row >> 2), row r's 16 dwords of four samples rotated by 4 (r & 3)."""
    row, sample = np.meshgrid(np.arange(16), np.arange(64), indexing="ij")
    dword = ((sample >> 2) + 4 * (row & 3)) & 15
    return ((4 * (row & 3) + (row >> 2)) * 16 + dword) * 4 + (sample & 3)


def _relayout(a16):
    """The byte image of a (N16, SD) u16 array with every element <= 255."""
    n16, sd = a16.shape
    assert a16.max() <= 255
    blocks = a16.astype(np.uint8).reshape(n16 // 16, 16, sd // 64, 64).transpose(0, 2, 1, 3)  # [block, group, row, sample]
    out = np.empty((n16 // 16, sd // 64, 1024), dtype=np.uint8)
    out[:, :, _image_offsets()] = blocks
    return out


IMAGE_N, IMAGE_S = 16 * 9 - 5, 201   # nine blocks with a ragged last one; a ragged fourth column group


@pytest.mark.parametrize("setup", ["created", "masked", "gathered"])
def test_images_are_the_relayout_of_the_u16_copies(ctx, setup):
    from demethify_amd.device import Problem

    V, D, Rt, _, _ = _inputs(IMAGE_N, IMAGE_S, 3, 2, (1, 255, 16), seed=77)
    with Problem(ctx, V, D, Rt) as full:
        if setup == "masked":
            p = full.masked(_mask(IMAGE_N, IMAGE_S))
        elif setup == "gathered":
            p = full.gather(_gather_idx(IMAGE_N))
        else:
            p = full
        try:
            rep = p.report()
            assert rep["has_X16"] and rep["has_D16"] and p.has_byte_images()
            x16, d16 = p.copy_out("X16", rep), p.copy_out("D16", rep)
            x8, d8 = p.copy_out_image("X8", rep), p.copy_out_image("D8", rep)
        finally:
            if p is not full:
                p.close()
    assert x8.shape == d8.shape == (rep["N16"] // 16, 4, 1024)
    assert np.array_equal(x8, _relayout(x16)) and np.array_equal(d8, _relayout(d16))
    assert d16[: rep["N"], :IMAGE_S].max() > 127 and x16.max() > 127   # (both halves of the byte range are there)
    if setup == "masked":   # the masked counts, not the source's
        kept = _mask(IMAGE_N, IMAGE_S)
        assert (d16[:IMAGE_N, :IMAGE_S][~kept] == 0).all() and (d16[:IMAGE_N, :IMAGE_S][kept] > 0).all()


@pytest.mark.parametrize("S,hi,x16", [(192, 100, True), (200, 256, True), (257, 100, True), (200, 100, False)])
def test_no_images_where_the_schedule_cannot_run(ctx, S, hi, x16):
    from demethify_amd import _lib as L
    from demethify_amd.device import Problem

    V, D, Rt, _, _ = _inputs(IMAGE_N, S, 3, 2, (1, hi, 16), seed=78)
    ctx.set_x16(x16)
    try:
        with Problem(ctx, V, D, Rt) as p:
            assert not p.has_byte_images()
            for name in L.PROBLEM_BYTE_IMAGES:
                with pytest.raises(L.DemethifyHipError) as e:
                    p.copy_out_image(name)
                assert e.value.status == L.DMF_ERR_BAD_ARG, (name, e.value.status)
    finally:
        ctx.set_x16(True)
