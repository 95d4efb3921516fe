"""Records what the batch routes do on this checkout into tests/golden/batch_routes.json and batch_calls.json (the harness
is tests/batch_route_cases.py; no GPU).  Run once on the commit whose behaviour is to be kept:

    python tools/record_batch_routes.py

tests/test_batch_routes_host.py then holds every later commit to the two files."""
import json
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import batch_route_cases as cases  # noqa: E402


def main():
    from demethify_amd import _build

    _build.build()
    golden = ROOT / "tests" / "golden"
    with tempfile.TemporaryDirectory() as tmp:
        routes = cases.route_matrix(Path(tmp) / "out")
    for name, content in (("batch_routes.json", routes), ("batch_calls.json", cases.entry_point_calls())):
        (golden / name).write_text(json.dumps(content, indent=1, sort_keys=True) + "\n")
        print(f"{name}: {len(content)} cases")


if __name__ == "__main__":
    main()
