"""The sampler's step-count read-ahead (csrc/step_ahead.h: when hmc_sample launches the cap of leapfrog steps without
waiting for the device's count) as plain C++ under AddressSanitizer + UBSan: tests/host_step_ahead_driver.cpp simulates
the ring of eight slots and the clock, with cap = 10.  No GPU, no HIP: the header makes no HIP call."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCENARIOS = {
    "warm_up": "all counts at the cap: eight synchronous proposals, then the cap without waiting; never with the switch off",
    "below_cap": "a count of 9 ends the speculation at the next decision; eight more at the cap before it resumes",
    "look_ahead": "at most four unobserved proposals behind a decision; 2000 ms without an arrival: synchronise",
    "foreign_token": "another sequence number in the slot: not arrived for harvest, hmc_sample's errors after a synchronise",
    "two_calls": "sequence numbers continue over two calls that share a ring, and across the wrap of the counter",
}


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ not found: the read-ahead logic cannot be checked")
    csrc = os.path.join(ROOT, "glmmrmcml_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("step_ahead") / "host_step_ahead_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + csrc,
           os.path.join(ROOT, "tests", "host_step_ahead_driver.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_read_ahead(report, name):
    lines = [ln for ln in report.splitlines() if ln.startswith("scenario %s " % name)]
    assert lines == ["scenario %s fails=0" % name], report


def test_header_is_host_only():
    """the read-ahead header includes nothing and calls nothing of HIP (the driver above is compiled by g++ without it)"""
    text = open(os.path.join(ROOT, "glmmrmcml_amd", "csrc", "step_ahead.h")).read()
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    assert "#include" not in code and "hip" not in code
