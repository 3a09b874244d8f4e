"""The association gives the bytes that tests/golden/assoc_bits.json records (scripts/record_assoc_bits.py: the cases, and how to
re-record after a deliberate change of the association's arithmetic).  The other tests hold the node targets to 1e-12 of the oracle's;
a changed order of the fp64 operations in the keys, the sorted lists or the means shows here only."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_assoc_bits", os.path.join(ROOT, "scripts", "record_assoc_bits.py"))
REC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REC)

with open(os.path.join(ROOT, "tests", "golden", "assoc_bits.json")) as _fh:
    GOLDEN = json.load(_fh)


def test_the_recording_holds_every_case():
    assert sorted(GOLDEN["cases"]) == sorted(REC.CASES) and len(GOLDEN["parent"]) == 40


@pytest.mark.parametrize("case", REC.CASES)
def test_the_bytes_are_the_recorded_ones(case):
    from multiviewstitch_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    got, want = REC.record(case), GOLDEN["cases"][case]
    for part in sorted(set(got) | set(want)):
        assert got.get(part) == want.get(part), f"{case}: {part} (recorded at {GOLDEN['parent']})"
