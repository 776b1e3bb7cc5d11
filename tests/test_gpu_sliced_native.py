"""The segmented radix sort of fadtk_amd/csrc/sliced_sort.h below the public entry: a gfx950 executable built from
tests/native/sliced_sort_check.hip by `python -m fadtk_amd.build` (the header of that file says what is compared: bit for bit against
std::sort of the mapped keys, over denormals, both zeros, +-FLT_MAX, keys sharing three of four bytes, at 1, 3 and 65 segments).
tests/test_gpu_sliced.py has the public entry."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
EXE = Path(__file__).resolve().parent / "native" / "sliced_sort_check"


def test_segmented_sort_against_std_sort():
    if not EXE.exists():
        from fadtk_amd.build import build_native_tests
        build_native_tests()
    r = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
