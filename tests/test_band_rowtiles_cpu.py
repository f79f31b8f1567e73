"""The host arithmetic of the banded products' row-tile extents (csrc/band_plan.h): which K tiles of a band are interior,
which MFMAs an edge tile issues, and how many MFMAs a launch issues, against a brute-force scan of small operands and
the closed forms of the triangular ones -- n = 200 (362 per 16-column strip forward), n = 5000 (196 562 forward of the
whole tiles' 202 200; 195 938 backward).  A stand-alone driver under AddressSanitizer + UBSan, no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_row_tile_extents_under_asan_ubsan(tmp_path):
    csrc = os.path.join(ROOT, "glmmrmcml_amd", "csrc")
    exe = str(tmp_path / "host_band_rowtiles_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + csrc,
           "-I" + os.path.join(ROOT, "include"),
           "-x", "c++", os.path.join(csrc, "common.hip"), "-x", "c++", os.path.join(ROOT, "tests", "host_band_rowtiles_driver.cpp"),
           "-o", exe, "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "fails=0" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
