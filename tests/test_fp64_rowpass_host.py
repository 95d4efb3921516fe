"""The case tables of tests/test_gpu_fp64_rowpass.py (tests/fp64_rowpass.py) against the launch plans of the first-generation
FP64 row kernels, through the pure dmf_u_phase_describe and dmf_select_describe: every case runs the instance, mode, wave
count and blocks per workgroup it claims, the tables reach every template instance that ANY key reaches (the unreachable
ones are listed by name with the rule that excludes them), and the supported boundaries answer as the rules say.  No GPU."""
import ctypes as C
import itertools

import pytest

import fp64_rowpass as fr

from demethify_amd import _lib as L
from demethify_amd.device import u_phase_describe

F32 = L.DMF_SELECT_COUNTS_F32_EXACT
AOUT = L.DMF_SELECT_ALPHA_OUTSIDE_UNIT


def _select(N, S, n_c, n_u, nd, level, n_iter2, flags):
    buf = C.create_string_buffer(512)
    st = L.load().dmf_select_describe(N, S, n_c, n_u, nd, level, n_iter2, flags, buf, len(buf))
    return st, buf.value.decode()


# ------------------------------------------------------------------------------------------------ the cases are what they claim
def test_stand_alone_cases_describe_as_their_plan():
    """Every stand-alone case: dmf_u_phase_describe (route update_u) answers the plan written down in fr.expected_text --
    template arguments, mode, waves, grid, LDS bytes, the raise and the blocks per workgroup."""
    for c in fr.instance_cases() + fr.subset_cases():
        assert fr.describe(c) == fr.expected_text(c), fr.uid(c)
        assert fr.instance_of(fr.describe(c))[0] == c.kernel, fr.uid(c)


def test_fused_cases_describe_as_their_plan():
    for c in fr.fused_cases():
        text = fr.fused_describe(c)
        assert text == fr.fused_text(c.N, c.S, c.n_c, c.n_u, c.n_iter2), fr.fid(c)
        # ... and the loop's own description names the same kernel, with the fused Gram behind it
        st, sel = _select(c.N, c.S, c.n_c, c.n_u, 0, 0 if c.big else 4, c.n_iter2, F32)
        assert st == L.DMF_OK and sel.startswith(f"rowpass=k_rowpass_fused<{(c.n_c + 3) // 4},{c.n_u}> nw={(c.S + 63) // 64} "), sel
        assert " gram=fused " in sel and f"grid={fr.field(text, 'grid')} tail={c.N % 16} " in sel
    for g in fr.FUSED_GRAM:
        text = u_phase_describe(g.N, g.S, g.n_c, g.n_u, 0, 4, g.n_iter2, F32, "solver")
        assert text == fr.fused_text(g.N, g.S, g.n_c, g.n_u, g.n_iter2), fr.gid(g)


def test_wrapping_cases_take_one_two_and_three_blocks():
    """N = block rows x (2 grid + 1) + a ragged tail, the grid at its cap: workgroup 0 takes a third full block, workgroup 1
    the ragged one, the others two."""
    for c in fr.wrap_cases():
        text = fr.describe(c)
        block = {"mfma": 16, "big": 16, "direct": 4}[c.kernel]
        grid = fr.field(text, "grid")
        assert fr.field(text, "blocks/wg") == 3 and c.N // block == 2 * grid + 1 and c.N % block != 0, fr.uid(c)
    assert {fr.field(fr.describe(c), "nw") for c in fr.wrap_cases() if c.kernel == "mfma"} == {1, 2, 3, 8}
    assert {fr.instance_of(fr.describe(c))[3:] for c in fr.wrap_cases() if c.kernel == "mfma"} == set(
        itertools.product(fr.FORMS, fr.MODES))
    assert {fr.instance_of(fr.describe(c))[2] for c in fr.wrap_cases() if c.kernel == "big"} == {16, 32}
    assert {fr.field(fr.describe(c), "grid") for c in fr.wrap_cases() if c.kernel == "big"} == {512, 256}
    for c in fr.fused_wrap_cases():
        text = fr.fused_describe(c)
        assert fr.field(text, "blocks/wg") == 3 and c.N // 16 == 2 * fr.field(text, "grid") + 1, fr.fid(c)
    assert {fr.field(fr.fused_describe(c), "nw") for c in fr.fused_wrap_cases()} == {1, 2, 3, 4}
    assert {c.N % 16 for c in fr.fused_wrap_cases()} == {0, 5}


def test_lds_raise_cases():
    """The launchers that raise the dynamic-LDS limit do so in some case: k_u_phase_big by its momentum table and by its
    alpha copy, k_u_phase_mfma by the partial sums of eight waves in both modes (its momentum table never gets there: more
    than 50 inner steps take the split mode, which keeps none).  k_u_step_direct's largest S asks for 60 KB and its
    launcher raises nothing."""
    raised = [c for c in fr.subset_cases() if " raise=1 " in fr.describe(c)]
    assert {(c.kernel, c.n_iter2 == fr.LDS_STEPS) for c in raised} == {("mfma", False), ("big", True), ("big", False)}
    assert {fr.instance_of(fr.describe(c))[4] for c in raised if c.kernel == "mfma"} == set(fr.MODES)
    assert all(" split " in u_phase_describe(53, 8, n_c, n_u, 0, 3, 51, 0, "update_u") for n_c in (0, 2) for n_u in range(1, 9))
    top = [c for c in fr.subset_cases() if c.kernel == "direct" and c.S == 1792]
    assert len(top) == 1 and " lds=61440 raise=0 " in fr.describe(top[0])


# ------------------------------------------------------------------------------------------------ reachability
S_GRID = (2, 6, 8, 68, 132, 196, 256, 260, 512, 516, 1537, 1792, 1796)
NC_GRID = (0, 1, 5, 12, 16, 17)
NU_GRID = tuple(range(1, 28)) + (32,)
STEPS = (0, 1, 2, 20, 50, 51)


def _reachable():
    """Every first-generation instance that some key reaches: a grid of shapes x levels 0..4 x count digit planes 0 / 1 / 2
    (integer copies exist at level 0 only) x alpha inside / outside [0, 1] x counts exact in f32 or not x inner steps x
    both entry points, as tests/golden/make_kernel_selection.py enumerates."""
    seen = set()
    keys = [(level, nd) for level in range(5) for nd in ((0, 1, 2) if level == 0 else (0,))]
    for S, n_c, n_u in itertools.product(S_GRID, NC_GRID, NU_GRID):
        if n_c + n_u > L.MAX_K:
            continue
        for (level, nd), aout, f32, n_iter2, route in itertools.product(keys, (0, AOUT), (0, F32), STEPS, ("solver", "update_u")):
            for N in (48, 53) if route == "solver" else (53,):
                text = u_phase_describe(N, S, n_c, n_u, nd, level, n_iter2, aout | f32, route)
                if text is not None and fr.instance_of(text) is not None:
                    seen.add(fr.instance_of(text))
    return seen


@pytest.fixture(scope="module")
def reachable():
    return _reachable()


def _covered():
    got = {fr.instance_of(fr.describe(c)) for c in fr.instance_cases()}
    got |= {fr.instance_of(fr.fused_describe(c)) for c in fr.fused_cases()}
    return got


def test_tables_cover_every_reachable_instance(reachable):
    """The instance tables name exactly the instances the enumeration reaches (k_u_phase_gram with alpha in LDS and in
    global memory counted apart; k_u_phase_mfma per form and mode; k_rowpass_fused per column-group count where the table
    claims it): removing a case, or a selection rule that moves one, fails here."""
    covered = _covered()
    assert covered - reachable == set(), sorted(covered - reachable)
    # k_rowpass_fused at nw 2..4 is sampled (five instances each), everything else is complete
    missing = {i for i in reachable - covered if not (i[0] == "fused" and i[3] > 1)}
    assert missing == set(), sorted(missing)
    mfma = {i for i in covered if i[0] == "mfma"}
    assert {(i[3], i[4]) for i in mfma} == set(itertools.product(fr.FORMS, fr.MODES))
    assert {i[1:4] for i in mfma} == set(itertools.product(range(5), range(1, 9), fr.FORMS))   # all 120 instances
    assert len(mfma) == 120 + 66 and len(fr.mfma_instance_cases()) == 186
    assert {i for i in covered if i[0] == "big"} == {("big", nkc, gs) for nkc in range(5) for gs in (16, 32)}
    assert {c.n_u for c in fr.big_instance_cases()} == set(range(9, 27))
    assert {i for i in covered if i[0] == "gram"} == {("gram", n_u, a) for n_u in range(1, 17) for a in ("lds", "global")}
    assert ("direct",) in covered
    fused = {i for i in covered if i[0] == "fused"}
    assert {i[1:3] for i in fused if i[3] == 1} == set(itertools.product(range(5), range(1, 5)))   # all 20 at nw = 1
    for nw in (2, 3, 4):
        assert len({i for i in fused if i[3] == nw}) >= 4, nw
    assert {c.n_iter2 for c in fr.fused_cases()} >= {0, 1, 20, 50} and {c.N % 16 for c in fr.fused_cases()} == {0, 5}
    assert {c.N for c in fr.fused_cases()} >= {16, 32}


def test_unreachable_instances_are_listed_by_name(reachable):
    """What no key reaches, with the rule: one-launch k_u_phase_mfma at 7 and 8 unknowns, and at 5 and 6 with known types
    (54 instance x mode pairs; each of those kernels still runs in split mode).  Everything else of the five kernels is
    reached."""
    listed = fr.mfma_unreachable()
    assert len(listed) == 54 and all(rule for _, rule in listed)
    everything = {("mfma", nkc, n_u, form, mode) for nkc in range(5) for n_u in range(1, 9) for form in fr.FORMS for mode in fr.MODES}
    assert everything - {i for i in reachable if i[0] == "mfma"} == {i for i, _ in listed}
    assert {i[1:3] for i in reachable if i[0] == "fused"} == set(itertools.product(range(5), range(1, 5)))
    assert {i[3] for i in reachable if i[0] == "fused"} == {1, 2, 3, 4}


# ------------------------------------------------------------------------------------------------ supported boundaries
def _row(N, S, n_c, n_u, nd, level, n_iter2, flags=F32):
    st, text = _select(N, S, n_c, n_u, nd, level, n_iter2, flags)
    return text.split(" gram=")[0] if st == L.DMF_OK else st


def test_supported_boundaries():
    # k_u_phase_mfma: S 512 / 513 and n_c 16 / 17 (level 3: no integer copies; beyond: k_u_phase_gram)
    assert _row(1000, 512, 16, 2, 0, 3, 20) == "rowpass=k_u_phase_mfma"
    assert _row(1000, 513, 16, 2, 0, 3, 20) == "rowpass=k_u_phase_gram"
    assert _row(1000, 512, 17, 2, 0, 3, 20) == "rowpass=k_u_phase_gram"
    assert u_phase_describe(1000, 512, 16, 2, 0, 3, 20, F32).startswith("k_u_phase_mfma<4,2,vec> one-launch nw=8 ")
    assert u_phase_describe(1000, 513, 16, 2, 0, 3, 20, F32).startswith("k_u_phase_gram<2> ")
    # k_rowpass_fused: S % 4, S 256 / 260, N >= 16, counts exact in f32; the accumulator limit of 80 admits all 20 instances
    assert _row(1000, 256, 12, 4, 0, 4, 20).startswith("rowpass=k_rowpass_fused<3,4> nw=4 ")
    assert _row(1000, 260, 12, 4, 0, 4, 20) == "rowpass=k_u_phase_mfma"
    assert _row(1000, 254, 12, 4, 0, 4, 20) == "rowpass=k_u_phase_mfma"
    assert _row(15, 256, 12, 4, 0, 4, 20) == "rowpass=k_u_phase_mfma"
    assert _row(1000, 256, 12, 4, 0, 4, 20, flags=0) == "rowpass=k_u_phase_mfma"
    assert _row(1000, 256, 12, 4, 0, 4, 51) == "rowpass=k_u_phase_mfma(split)+k_u_inner_rows"
    assert max(4 * nkc * n_u + n_u * (n_u + 1) // 2 + n_u for nkc in range(5) for n_u in range(1, 5)) == 78 <= 80
    assert _row(1000, 256, 16, 4, 0, 4, 20).startswith("rowpass=k_rowpass_fused<4,4> ")
    assert _row(1000, 256, 16, 5, 0, 4, 20) == "rowpass=k_u_phase_mfma(split)+k_u_inner_rows"   # (five unknowns: not fused)
    # k_u_phase_big: n_u 8 / 9 and 26 / 27
    assert _row(1000, 64, 4, 8, 0, 3, 20) == "rowpass=k_u_phase_mfma(split)+k_u_inner_rows"
    assert _row(1000, 64, 4, 9, 0, 3, 20) == "rowpass=k_u_phase_big"
    assert _row(1000, 64, 4, 26, 0, 3, 20) == "rowpass=k_u_phase_big"
    assert _row(1000, 64, 4, 27, 0, 3, 20) == "rowpass=k_u_step_direct"
    assert u_phase_describe(1000, 64, 4, 26, 0, 3, 20, F32).startswith("k_u_phase_big<1,32> n_u=26 nw=8 ")
    # k_u_phase_gram: n_u 16 / 17
    assert _row(1000, 64, 4, 16, 0, 1, 20) == "rowpass=k_u_phase_gram"
    assert _row(1000, 64, 4, 17, 0, 1, 20) == "rowpass=k_u_step_direct"
    # k_u_step_direct: S 1792 / 1793 -- beyond, no kernel takes the shape and nothing is launched
    assert _row(1000, 1792, 4, 3, 0, 2, 20) == "rowpass=k_u_step_direct"
    assert _row(1000, 1793, 4, 3, 0, 2, 20) == L.DMF_ERR_UNSUPPORTED
    assert _row(1000, 1793, 4, 17, 0, 1, 20) == L.DMF_ERR_UNSUPPORTED
    assert u_phase_describe(1000, 1793, 4, 3, 0, 2, 20, F32) is None
    assert u_phase_describe(1000, 1793, 4, 3, 0, 2, 20, F32, "update_u") is None
    assert u_phase_describe(1000, 1793, 4, 3, 0, 1, 20, F32).startswith("k_u_phase_gram<3> alpha=global ")


def test_second_generation_kernels_keep_their_row_text():
    """For a u phase that is not one of the five kernels the accessor answers the rowpass= part of dmf_select_describe --
    followed by the launch plan of the kernel it names: the integer producer k_cm_i8's (tests/cm_exact.py writes it down) or
    the one-launch row pass k_rowpass_v2's (tests/rowpass_schedule_model.py; the flags do not say that every count fits a byte)."""
    import cm_exact as cm
    import rowpass_schedule_model as rp

    flags = F32 | L.DMF_SELECT_X16
    for key, producer in (((1000, 64, 6, 2, 1, 0, 20), False), ((1000, 640, 6, 2, 1, 0, 20), True), ((1000, 64, 0, 12, 1, 0, 20), True),
                          ((5000, 256, 12, 4, 1, 0, 20), False)):
        st, sel = _select(*key, flags)
        assert st == L.DMF_OK
        N, S, n_c, n_u, nd = key[:5]
        plan = cm.plan_text(N, S, n_c, n_u, nd) if producer else rp.plan_text(N, S, n_c, n_u, 20, max_count=256).split(" x16 ")[1]
        assert ("k_cm_i8<" in sel) == producer and ("k_rowpass_v2<" in sel) == (not producer)
        assert plan.startswith("panels=" if producer else "maxw=4 one nw=1 " if S == 64 else "maxw=4 pair nw=4 ")
        assert "rowpass=" + u_phase_describe(*key, flags) == sel.split(" gram=")[0] + " " + plan


def test_describe_argument_checks():
    lib, buf = L.load(), C.create_string_buffer(256)
    ok = (100, 8, 2, 3, 0, 0, 5, 0, 0)
    assert lib.dmf_u_phase_describe(*ok, buf, len(buf)) == L.DMF_OK
    for i, bad in ((0, 0), (1, 0), (2, -1), (3, 0), (4, 3), (6, -1), (8, 2), (8, -1)):
        args = list(ok)
        args[i] = bad
        assert lib.dmf_u_phase_describe(*args, buf, len(buf)) == L.DMF_ERR_BAD_ARG, (i, bad)
    assert lib.dmf_u_phase_describe(*ok, None, 0) == L.DMF_ERR_BAD_ARG
    assert lib.dmf_solver_u_phase_describe(None, 5, 0, buf, len(buf)) == L.DMF_ERR_BAD_ARG
    with pytest.raises(ValueError):
        u_phase_describe(100, 8, 2, 3, route="loop")
