"""The Poisson stage gives the bytes that tests/golden/poisson_bits.json records (scripts/record_poisson_bits.py: the cases, and how to
re-record after a deliberate change of the solver's arithmetic).  The restatements solve directly and the other tests hold chi to a
bound; a changed order of the solver's fp64 operations shows here only."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_poisson_bits", os.path.join(ROOT, "scripts", "record_poisson_bits.py"))
REC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REC)

with open(os.path.join(ROOT, "tests", "golden", "poisson_bits.json")) as _fh:
    GOLDEN = json.load(_fh)


def test_the_recording_holds_every_case():
    assert sorted(GOLDEN["cases"]) == sorted(REC.CASES) and GOLDEN["solve_tol"] == REC.TOL and len(GOLDEN["parent"]) == 40


@pytest.mark.parametrize("case", REC.CASES)
def test_the_bytes_are_the_recorded_ones(case):
    got, want = REC.record(case), GOLDEN["cases"][case]
    for part in sorted(set(got) | set(want)):
        assert got.get(part) == want.get(part), f"{case}: {part} (recorded at {GOLDEN['parent']})"
