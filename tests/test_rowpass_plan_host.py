"""The row pass's launch plan (rowpass_v2_plan: the one plan launch_rowpass_v2 dispatches on) against the rule written down in
tests/rowpass_schedule_model.py, through the pure dmf_u_phase_describe: no GPU.

Whole-string equality over a grid of keys, so wave count, grid, blocks per workgroup, LDS bytes, the raise flag and the
schedule all have to agree; then that every schedule and both MAXW are reached, that the byte images are built exactly
where some plan reads them, that the plan stands exactly where the selection table names the kernel, and that the case
tables of the four GPU files name the schedule the plan gives them."""
import ctypes as C
import itertools

import pytest

import rowpass_schedule_model as model
from demethify_amd import _lib as L

F32 = L.DMF_SELECT_COUNTS_F32_EXACT
SWITCHES = (L.DMF_SELECT_NO_ROWPASS_PAIR, L.DMF_SELECT_NO_ROWPASS_DEFER_C, L.DMF_SELECT_NO_ROWPASS_BYTES)

# every wave count 1..8 and both sides of every 64 k; 192 / 193 and 256 / 257 are the deferred-C schedule's and MAXW's edges
SAMPLES = [2, 63] + [64 * k + d for k in range(1, 8) for d in (0, 1, 63)] + [512]
STEPS = (1, 20, 50)


def _flags(x16, byte_counts, off):
    """DMF_SELECT_* of a problem (off: which of the three context switches are off, as a 3-bit number)."""
    return (F32 | (L.DMF_SELECT_X16 if x16 else 0) | (L.DMF_SELECT_COUNTS_BYTE if byte_counts else 0) |
            sum(bit for i, bit in enumerate(SWITCHES) if off >> i & 1))


def _model_kw(x16, byte_counts, off):
    return dict(x16=x16, max_count=255 if byte_counts else 256, pair=not off & 1, defer_c=not off & 2, bytes_=not off & 4)


def _rows(S):
    """15 rows, one block short of the full grid, a few blocks past it with a ragged last one, and the headline's million."""
    full = model.plan(10 ** 7, S, 0, 1)["grid"]
    return (15, 16 * (full - 1), 16 * (full + 3) + 5, 1_000_000)


class _Lib:
    def __init__(self):
        self.lib, self.buf = L.load(), C.create_string_buffer(2048)

    def _text(self, fn, args):
        st = fn(*args, self.buf, len(self.buf))
        if st == L.DMF_ERR_UNSUPPORTED:
            return None
        assert st == L.DMF_OK, (st, args)
        return self.buf.value.decode()

    def u_phase(self, N, S, n_c, n_u, nd, n_iter2, flags):
        return self._text(self.lib.dmf_u_phase_describe, (N, S, n_c, n_u, nd, 0, n_iter2, flags, L.DMF_ROUTE_SOLVER))

    def select(self, N, S, n_c, n_u, nd, n_iter2, flags):
        return self._text(self.lib.dmf_select_describe, (N, S, n_c, n_u, nd, 0, n_iter2, flags))


@pytest.fixture(scope="module")
def lib():
    return _Lib()


def test_plan_text_equals_the_library_over_the_grid(lib):
    """dmf_u_phase_describe == model.plan_text, whole strings; every schedule and both MAXW occur; the images are wanted
    exactly where some plan of the problem has `bytes`."""
    seen, reads_images = set(), {}
    for S in SAMPLES:
        rows = _rows(S)
        for n_c, n_u, n_iter2, x16, byte_counts, off in itertools.product(range(17), range(1, 5), STEPS, (False, True),
                                                                         (False, True), range(8)):
            nd = 1 if byte_counts and n_c % 2 else 2  # (the plan does not read the digit count: both values, no third axis)
            flags, kw = _flags(x16, byte_counts, off), _model_kw(x16, byte_counts, off)
            for N in rows:
                want = model.plan_text(N, S, n_c, n_u, n_iter2, **kw)
                got = lib.u_phase(N, S, n_c, n_u, nd, n_iter2, flags)
                assert got == want, (N, S, n_c, n_u, n_iter2, kw)
            word = model.schedule_in_text(got)
            seen.add((word, int(got.split(" maxw=")[1].split()[0])))
            problem = (S, x16, byte_counts)
            reads_images[problem] = reads_images.get(problem, False) or word == "bytes"
    assert seen == {("one", 4), ("pair", 4), ("deferred", 4), ("bytes", 4), ("one", 8)}, seen
    for (S, x16, byte_counts), some_plan_reads in reads_images.items():
        for max_count in ((0, 255) if byte_counts else (256, 32639)):
            assert model.byte_images_wanted(S, x16, max_count) == some_plan_reads, (S, x16, max_count)


def test_images_wanted_rule_at_its_edges():
    assert model.byte_images_wanted(193, True, 255) and model.byte_images_wanted(256, True, 0)
    assert not model.byte_images_wanted(192, True, 255) and not model.byte_images_wanted(257, True, 255)
    assert not model.byte_images_wanted(256, True, 256) and not model.byte_images_wanted(256, False, 255)
    assert not model.byte_images_wanted(256, True, float("inf"))


def test_plan_stands_exactly_where_the_selection_names_the_kernel(lib):
    """Inside the kernel's range and outside it (513 samples and more, 17 known types, 5 unknowns, no integer copies, more
    than 50 inner steps, none): the accessor answers a plan iff dmf_select_describe names k_rowpass_v2, and then the
    selection's rowpass= text is the head of the accessor's."""
    n = 0
    for S, n_c, n_u, nd, n_iter2, x16 in itertools.product((1, 2, 200, 512, 513, 576, 640), (0, 12, 16, 17), (1, 4, 5), (0, 1, 2),
                                                           (0, 1, 50, 51), (False, True)):
        for N in (15, 5000):
            flags = _flags(x16, True, 0)
            sel, text = lib.select(N, S, n_c, n_u, nd, n_iter2, flags), lib.u_phase(N, S, n_c, n_u, nd, n_iter2, flags)
            named = sel is not None and "k_rowpass_v2" in sel
            in_range = nd > 0 and 1 <= n_iter2 <= 50
            want = model.plan_text(N, S, n_c, n_u, n_iter2, x16=x16 and nd > 0) if in_range else None
            assert named == (want is not None), (N, S, n_c, n_u, nd, n_iter2, sel)
            assert (text == want) if named else (text is None or not text.startswith("k_rowpass_v2")), (text, want)
            if named:
                assert ("rowpass=" + text).startswith(sel.split(" gram=")[0] + " maxw="), (sel, text)
                n += 1
    assert n > 100


def test_model_spot_values():
    """A few values by hand, so that the model is not only held to the library: the headline shape's three X16 schedules
    (70 848 B deferred on u16 counts) and the grid rule."""
    head = dict(N=1_000_000, S=256, n_c=12, n_u=4, n_iter2=20)
    assert model.plan(**head)["lds"] == 60608 and model.plan(**head)["schedule"] == "bytes"
    assert model.plan(**head, bytes_=False)["lds"] == 70848 and model.plan(**head, defer_c=False)["lds"] == 62656
    assert model.plan(**head, x16=False)["lds"] == 56000 and model.plan(**head, x16=False)["schedule"] == "one"
    assert model.plan(**head)["grid"] == 512 and model.plan(**head)["blocks"] == (122, 123)
    assert model.plan(1000, 65, 16, 4)["schedule"] == "one" and model.plan(1000, 65, 16, 3)["schedule"] == "pair"  # 44 KB x 4
    assert model.plan(1000, 512, 16, 4)["maxw"] == 8 and model.plan(1000, 513, 0, 1) is None


def test_gpu_case_tables_name_the_plans_schedule():
    """The hand-written columns of the four GPU files equal the model, which the grid above holds to the library."""
    import test_gpu_rowpass_bytes as tb
    import test_gpu_rowpass_defer_c as td
    import test_gpu_rowpass_forms as tf
    import test_gpu_rowpass_pair as tp

    for N, S, n_c, n_u, n_iter2, depth, paired, why in tp.CASES:
        for max_count in (255, 256):  # (whatever the counts: a deferred launch is a paired one)
            assert (model.schedule(S, n_c, n_u, n_iter2, max_count=max_count) != "one") == paired, why
        assert model.schedule(S, n_c, n_u, n_iter2, pair=False) == "one", why
    for blocks, off, nk, S, n_c, n_u, n_iter2, counts, setup, deferred, paired, why in td.CASES:
        kw = dict(x16=setup != "no_x16", max_count=counts[1])
        assert model.schedule(S, n_c, n_u, n_iter2, **kw) == ("bytes" if deferred else "pair" if paired else "one"), why
        assert model.schedule(S, n_c, n_u, n_iter2, defer_c=False, **kw) == ("pair" if paired else "one"), why
    for blocks, off, nk, S, n_c, n_u, n_iter2, counts, setup, takes, why in tb.CASES:
        kw = dict(x16=setup != "no_x16", max_count=counts[1])
        assert (model.schedule(S, n_c, n_u, n_iter2, **kw) == "bytes") == takes, why
        assert (model.schedule(S, n_c, n_u, n_iter2, bytes_=False, **kw) == "deferred") == takes, why
        assert model.byte_images_wanted(S, kw["x16"], counts[1]) == takes, why  # (no case keeps images it cannot read)
    for cid, c in tf.MATRIX + tf.LOOPS:
        for leg in tf._legs(c.S):
            sched = tf._instance(c.S, c.n_c, c.n_u, leg, n_iter2=c.n_iter2)[4]
            for max_count in (255, 256):
                word = model.schedule(c.S, c.n_c, c.n_u, c.n_iter2, x16=leg[1], pair=leg[2], max_count=max_count)
                assert (word != "one") == (sched == "pair"), (cid, leg)
