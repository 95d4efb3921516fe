"""Kernel selection with DMF_SELECT_X16 (the problem carries its methylated read counts as u16): the rows of the checked-in
grid describe as without the flag, with one more token on k_rowpass_v2 -- no GPU involved."""
import importlib.util
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _grid_module():
    spec = importlib.util.spec_from_file_location("make_kernel_selection", ROOT / "tests" / "golden" / "make_kernel_selection.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _with_flags(row, flags):
    return (*row[:7], flags)


def test_x16_rows_append_one_token_to_the_row_pass():
    from demethify_amd import _lib as L

    mod = _grid_module()
    lib = L.load()
    X16, UNAL = L.DMF_SELECT_X16, L.DMF_SELECT_V_UNALIGNED
    n_v2 = 0
    for row in mod.grid():
        flags = int(row[7])
        base = mod.describe(lib, row)
        got = mod.describe(lib, _with_flags(row, flags | X16))
        if flags & UNAL:
            # the X16 row pass does not read V: its alignment no longer decides anything
            assert got == mod.describe(lib, _with_flags(row, (flags & ~UNAL) | X16)), row
            continue
        if "k_rowpass_v2" in base:
            n_v2 += 1
            want = re.sub(r"(rowpass=k_rowpass_v2<\d+,\d+> nw=\d+ grid=\d+ tail=\d+)", r"\1 x16", base)
            assert want != base
            assert got == want, row
        else:
            assert got == base, row
    assert n_v2 > 0


def test_x16_flag_needs_integer_copies():
    from demethify_amd import _lib as L

    mod = _grid_module()
    lib = L.load()
    f32 = L.DMF_SELECT_COUNTS_F32_EXACT
    on = mod.describe(lib, (1000000, 256, 12, 4, 1, 0, 20, f32 | L.DMF_SELECT_X16))
    assert on.startswith("rowpass=k_rowpass_v2<3,4> nw=4 grid=512 tail=0 x16 gram=")
    # no integer copies (nd = 0): no X16 either
    off = mod.describe(lib, (1000000, 256, 12, 4, 0, 0, 20, f32 | L.DMF_SELECT_X16))
    assert "x16" not in off and off == mod.describe(lib, (1000000, 256, 12, 4, 0, 0, 20, f32))
    # an unaligned V keeps the X16 row pass
    unal = mod.describe(lib, (1000000, 256, 12, 4, 1, 0, 20, f32 | L.DMF_SELECT_X16 | L.DMF_SELECT_V_UNALIGNED))
    assert unal == on
