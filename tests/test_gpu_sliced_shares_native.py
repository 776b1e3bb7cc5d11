"""The key-index segmented sort of fadtk_amd/csrc/sliced_sort_pairs.h below the public entry: a gfx950 executable built from
tests/native/sliced_sort_pairs_check.hip by `python -m fadtk_amd.build` (the header of that file says what is compared: keys and indices
bit for bit against std::stable_sort of (mapped key, position), over denormals, both zeros, +-FLT_MAX, infinities, keys sharing three of
four bytes, all-equal, sorted, reversed and two-valued keys, at 1, 3 and 65 segments, with guard words around every buffer).
tests/test_gpu_sliced_shares.py has the public entry."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
EXE = Path(__file__).resolve().parent / "native" / "sliced_sort_pairs_check"


def test_segmented_pair_sort_against_std_stable_sort():
    if not EXE.exists():
        from fadtk_amd.build import build_native_tests
        build_native_tests()
    r = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
