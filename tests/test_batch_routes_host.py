"""The batch routes against recordings of what they did before the routing was gathered into demethify_amd/batch.py (no
GPU): tests/golden/batch_routes.json and batch_calls.json, written by tools/record_batch_routes.py on the commit before; the
harness is tests/batch_route_cases.py."""
import json

import pytest

import batch_route_cases as cases
from conftest import GOLDEN


@pytest.fixture(scope="module", autouse=True)
def _library():
    from demethify_amd import _build

    _build.build()


def test_every_command_line_route_is_the_recorded_one(tmp_path):
    """About a hundred command lines on the toy -- --restart and --confidence under every subset of DEMETHIFY_BATCH, _MID and
    _MID_PURITY, with and without --purity, --ic CCC and AIC under every subset of DEMETHIFY_BATCH, _MID and _MID_IC, each with
    every size gate open around the toy and shut, each range gate closed, and the --init uniform and the aligning refusals:
    the sink reached, the batch size and purity vector it saw, the batch keywords of bt_ci / evaluate_best_ic and the Note
    lines, verbatim and in order."""
    recorded = json.loads((GOLDEN / "batch_routes.json").read_text())
    grid = cases.route_cases()
    assert sorted(case[0] for case in grid) == sorted(recorded)
    for case in grid:
        got = json.loads(json.dumps(cases.run_route_case(case, tmp_path / "out")))
        assert got == recorded[case[0]], case[0]


def test_every_entry_point_gets_the_recorded_argument_list():
    """dmf_solve_{small,mid}{,_purity,_masked} through solve_many, solve_many_mid, solve_many_masked and
    solve_many_mid_masked with distinct values everywhere: the function, every scalar by position and value, every pointer by
    position, null or not, and the dtype and shape of the array behind it."""
    recorded = json.loads((GOLDEN / "batch_calls.json").read_text())
    got = json.loads(json.dumps(cases.entry_point_calls()))
    assert sorted(got) == sorted(recorded)
    assert sorted({call["function"] for call in recorded.values()}) == [
        "dmf_solve_mid", "dmf_solve_mid_masked", "dmf_solve_mid_purity", "dmf_solve_small", "dmf_solve_small_masked",
        "dmf_solve_small_purity"]
    for label, call in recorded.items():
        assert got[label] == call, label
