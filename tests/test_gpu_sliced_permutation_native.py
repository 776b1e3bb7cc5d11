"""The stable split of fadtk_amd/csrc/sliced_split.h below the public entry: a gfx950 executable built from
tests/native/sliced_split_check.hip by `python -m fadtk_amd.build` (the header of that file says what is compared: both groups of every
(direction, labelling) pair bit for bit against std::stable_partition, at the lane, wave, row and workgroup boundaries, with guard words
around every buffer and after every pair's segments).  tests/test_gpu_sliced_permutation.py has the public entry."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
EXE = Path(__file__).resolve().parent / "native" / "sliced_split_check"


def test_split_against_stable_partition():
    if not EXE.exists():
        from fadtk_amd.build import build_native_tests
        build_native_tests()
    r = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
