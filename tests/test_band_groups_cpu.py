"""The whole-band form of the banded HMC products' work decomposition (csrc/band_plan.h) deals whole bands into
balanced groups, one group per workgroup.  Host logic: a stand-alone driver under AddressSanitizer + UBSan checks the
largest group of the triangular shapes the sampler runs, the invariants of every whole-band shape in a sweep, and
that the streamed shapes come out byte for byte as before the grouping (tests/host_bandgroups_driver.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_band_groups_under_asan_ubsan(tmp_path):
    csrc = os.path.join(ROOT, "glmmrmcml_amd", "csrc")
    exe = str(tmp_path / "host_bandgroups_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + csrc,
           "-I" + os.path.join(ROOT, "include"),
           "-x", "c++", os.path.join(csrc, "common.hip"), "-x", "c++", os.path.join(ROOT, "tests", "host_bandgroups_driver.cpp"),
           "-o", exe, "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "fails=0" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
