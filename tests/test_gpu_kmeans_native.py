"""The centroid update of fadtk_amd/csrc/kmeans_update.h below the public entry: a gfx950 executable built from
tests/native/kmeans_update_check.hip by `python -m fadtk_amd.build` (the header of that file says what is compared: kmeans::update
against host long double on label sets fad_kmeans cannot easily produce -- all rows in one cluster, every cluster one row, empty
clusters interleaved, clusters of chunk - 1 / chunk / chunk + 1 rows -- for float32, float16 and bfloat16 rows, with the planes, h,
the untouched empty clusters, a second run and guard words behind every buffer).  tests/test_gpu_kmeans.py has the public entry."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
EXE = Path(__file__).resolve().parent / "native" / "kmeans_update_check"


def test_centroid_update_against_host_long_double():
    if not EXE.exists():
        from fadtk_amd.build import build_native_tests
        build_native_tests()
    r = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
