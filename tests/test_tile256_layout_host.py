"""fadtk_amd/csrc/tile256_layout.h -- the maps the 256-column-slab moments kernel, its epilogue and moments_reduce256 share -- checked
on the CPU (tests/native_cpu/tile256_layout_check.cpp, plain C++ built with g++): the slot's element map is a bijection and is the
accumulator layout of the 16x16x32 MFMA, the guard's pick-up names the diagonal, the part of a diagonal block the reduce reads is
issued, the LDS-DMA side and the transposed reads agree on the stage image, and every transposed read puts the two 16-lane groups of
each 32-lane half on 64 distinct banks.  No GPU."""
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_tile256_layout_maps_and_banks(tmp_path):
    exe = tmp_path / "tile256_layout_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe), str(ROOT / "tests" / "native_cpu" / "tile256_layout_check.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    assert "MFMAs per stage: 33 33 35 35 32" in r.stdout
    assert "64 transposed reads on 64 banks per half" in r.stdout
    assert "tile256 layout ok" in r.stdout
