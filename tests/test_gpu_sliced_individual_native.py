"""The resident song sort of fadtk_amd/csrc/sliced_song_sort.h below the public entry: a gfx950 executable built from
tests/native/sliced_song_sort_check.hip by `python -m fadtk_amd.build` (the header of that file says what is compared: every song's range
of every direction bit for bit against std::sort of the mapped keys, over the key sets of sliced_sort_check with NaN patterns added, over
song lengths on every edge of the unit table, at 1, 3 and 65 directions).  tests/test_gpu_sliced_individual.py has the public entry."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
EXE = Path(__file__).resolve().parent / "native" / "sliced_song_sort_check"


def test_resident_song_sort_against_std_sort():
    if not EXE.exists():
        from fadtk_amd.build import build_native_tests
        build_native_tests()
    r = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
