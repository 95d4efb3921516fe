"""The deferred-C schedule of the row pass, walked on the host (tests/rowpass_schedule_model.py): no GPU."""
import pytest

import rowpass_schedule_model as model


@pytest.mark.parametrize("nk", list(range(0, 10)) + [16, 17, 121, 122])
def test_schedule_holds(nk):
    n_bar = model.check(nk)
    assert n_bar == 2 * ((nk + 1) // 2)  # barriers X and Y per cycle, nothing else


def test_drain_shapes():
    # one pair pending on the waves that ran phase C in the last cycle, two on the waves that ran its phase B
    assert [model.pending_at_drain(1, w) for w in range(4)] == [[0]] * 4
    assert [model.pending_at_drain(2, w) for w in range(4)] == [[0, 1]] * 4
    assert [model.pending_at_drain(3, w) for w in range(4)] == [[2], [2], [0, 1, 2], [0, 1, 2]]
    assert [model.pending_at_drain(4, w) for w in range(4)] == [[2, 3], [2, 3], [0, 1, 2, 3], [0, 1, 2, 3]]
    assert [model.pending_at_drain(5, w) for w in range(4)] == [[2, 3, 4], [2, 3, 4], [4], [4]]
    assert [model.pending_at_drain(7, w) for w in range(4)] == [[6], [6], [4, 5, 6], [4, 5, 6]]


def test_model_sees_a_broken_hand_over(monkeypatch):
    # a ring or ubuf sets of two pairs would be overwritten before their last reader: the walk must say so
    real = model.wave_program

    def short_ring(nk, wave):
        fix = lambda blk: 2 * ((blk >> 1) % 2) + (blk & 1)
        return [(op[0], op[1], fix(op[1]), op[3]) if op[0] == "C" else
                ((op[0], op[1], fix(op[3]), op[3]) if op[0] == "store" else
                 ((op[0], op[1], op[2], fix(op[1])) if op[0] == "A" else op)) for op in real(nk, wave)]

    def two_ubuf_pairs(nk, wave):
        fix = lambda blk: 2 * ((blk >> 1) % 2) + (blk & 1)
        return [(op[0], op[1], op[2], fix(op[1])) if op[0] == "C" else ((op[0], op[1], fix(op[1])) if op[0] == "B" else op)
                for op in real(nk, wave)]

    for broken in (short_ring, two_ubuf_pairs):
        monkeypatch.setattr(model, "wave_program", broken)
        with pytest.raises(AssertionError):
            model.check(8)


def test_grid_rule():
    assert model.blocks_per_workgroup(1_000_000, 256) == (122, 123)
    assert model.blocks_per_workgroup(16 * 300 - 5, 256) == (1, 1)
    assert model.blocks_per_workgroup(16 * 812, 256) == (1, 2)
    assert model.blocks_per_workgroup(16 * 2100 + 3, 96) == (2, 3)


def test_lds_rule():
    assert model.runs_deferred(256, 12, 4, 20, 255) and model.runs_deferred(193, 0, 1, 3, 0)
    assert model.runs_deferred(256, 16, 2, 20, 255) and not model.runs_deferred(256, 16, 3, 20, 255)
    assert not model.runs_deferred(256, 12, 4, 20, 256) and not model.runs_deferred(192, 12, 4, 20, 50)
    assert not model.runs_deferred(256, 12, 4, 20, 50, x16=False) and not model.runs_deferred(256, 12, 4, 20, 50, defer_c=False)
