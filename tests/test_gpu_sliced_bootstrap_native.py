"""The stable expansion of fadtk_amd/csrc/sliced_expand.h below the public entry: a gfx950 executable built from
tests/native/sliced_expand_check.hip by `python -m fadtk_amd.build` (the header of that file says what is compared: the output of every
(direction, replicate) pair bit for bit against a host loop, at the lane, wave, row and workgroup boundaries, with guard words around
every buffer and after every pair's segment).  tests/test_gpu_sliced_bootstrap.py has the public entry."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
EXE = Path(__file__).resolve().parent / "native" / "sliced_expand_check"


def test_expansion_against_a_host_loop():
    if not EXE.exists():
        from fadtk_amd.build import build_native_tests
        build_native_tests()
    r = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
