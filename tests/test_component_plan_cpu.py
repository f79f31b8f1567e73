"""The host plan of the component-local trajectory kernel (csrc/component_plan.h) as plain C++ under AddressSanitizer +
UBSan, the way test_host_sanitizers.py builds the band-plan driver: tests/host_component_plan_driver.cpp reads the ELL
rows of ZL of a design, builds the plan, checks its invariants (the components partition 0 .. Q-1; every observation
lies in exactly one component with all its columns; bijective local indices; records hold every entry once, in order;
work items cover every component once) and prints the counts, which are compared here with the connected components
of the designs as counted by hand (scipy.sparse.csgraph.connected_components gives the same)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from glmmrmcml_amd import synth
from test_gpu_sparse_products import DROP, RAGGED, design

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 32                                    # CP_MAX_VARS


def _dims(cov):
    dims, seen = [], set()
    for r in cov:
        if int(r[0]) not in seen:
            seen.add(int(r[0])); dims.append(int(r[1]))
    return dims


def ell_rows(Z, dims):
    """the ELL rows of ZL as sparse_zl_setup (csrc/model.hip) builds them: a nonzero Z[i, j] brings the columns
    start(j) .. j of j's covariance block"""
    n, Q = Z.shape
    assert sum(dims) == Q
    start = np.repeat(np.cumsum([0] + dims[:-1]), dims)
    rows = [[t for j in np.nonzero(Z[i])[0] for t in range(start[j], j + 1)] for i in range(n)]
    width = np.array([len(r) for r in rows])
    W = int(width.max())
    col = np.zeros((n, W), dtype=int)
    for i, r in enumerate(rows):
        col[i, :len(r)] = r
    return n, Q, W, width, col


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ not found: the host plan cannot be checked")
    csrc = os.path.join(ROOT, "glmmrmcml_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("cp") / "host_component_plan_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + csrc, os.path.join(ROOT, "tests", "host_component_plan_driver.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    return exe


def run_plan(driver, tmp_path, Z, dims):
    n, Q, W, width, col = ell_rows(np.asarray(Z), dims)
    path = str(tmp_path / "ell.txt")
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (n, Q, W))
        f.write(" ".join(map(str, width)) + "\n")
        f.write(" ".join(map(str, col.ravel(order="F"))) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([driver, path], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "fails=0" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("ncomp="))
    return {k: int(v) for k, v in (kv.split("=") for kv in line.split())}


def _synth(gen, *a):
    s = gen(*a)
    return s["Z"], _dims(s["cov"])


def _kind(kind, **opts):
    d = design(kind, "poisson", "log", **opts)
    return d["Z"], d["dims"]


# name -> (Z and block sizes, components, most variables, most observations, components without an observation)
TABLE = {
    "cluster_rct_10_5_10": (lambda: _synth(synth.cluster_rct, 10, 5, 10), 10, 6, 50, 0),
    "stepped_wedge_40_8_50": (lambda: _synth(synth.stepped_wedge, 40, 8, 50), 40, 8, 400, 0),
    "longitudinal_37_10": (lambda: _synth(synth.longitudinal, 37, 10), 37, 11, 10, 0),
    "rct": (lambda: _kind("rct"), 7, 6, 15, 0),
    "sw_short_drop": (lambda: _kind("sw_short", drop=DROP["sw_short"]), 7, 5, 15, 1),
    "sw_long_ragged": (lambda: _kind("sw_long", ragged=RAGGED), 7, 5, 200, 0),
    "sw_blk17": (lambda: _kind("sw_blk17"), 5, 17, 34, 0),
    "tiny": (lambda: _kind("tiny"), 3, 3, 6, 0),
}


@pytest.mark.parametrize("name", list(TABLE))
def test_components_of_the_block_designs(driver, tmp_path, name):
    make, ncomp, max_vars, max_rows, empty = TABLE[name]
    Z, dims = make()
    p = run_plan(driver, tmp_path, Z, dims)
    assert (p["ncomp"], p["max_vars"], p["max_rows"], p["empty_comps"]) == (ncomp, max_vars, max_rows, empty), p
    assert p["feasible"] == 1 and p["cap"] == CAP and 16 <= CAP < 48
    assert 1 <= p["nitems"] <= ncomp
    assert p["waves"] == (4 if max_rows >= 128 else 1), p          # CP_WAVES4_ROWS


def test_one_dense_block_is_one_component(driver, tmp_path):
    """geospatial(n): Z = I and one dense block, row i of ZL = columns 0 .. i: one component of n variables, n observations"""
    n = 40
    p = run_plan(driver, tmp_path, np.eye(n), [n])
    assert (p["ncomp"], p["max_vars"], p["max_rows"], p["empty_comps"]) == (1, n, n, 0), p
    assert p["feasible"] == 0 and n > CAP
    n = 20
    p = run_plan(driver, tmp_path, np.eye(n), [n])
    assert (p["ncomp"], p["max_vars"], p["max_rows"], p["feasible"], p["nitems"]) == (1, n, n, 1, 1), p


def test_blocks_above_the_cap_are_infeasible(driver, tmp_path):
    """stepped_wedge(3, 48, 2): one block of 48 per cluster; a row of ZL is at most 48 <= 64 wide, so the sparse operator
    stays possible, but a component of 48 variables is above the kernel's cap: the whole model keeps the per-step path"""
    Z, dims = _synth(synth.stepped_wedge, 3, 48, 2)
    n, Q, W, width, col = ell_rows(np.asarray(Z), dims)
    assert W == 48 and W <= 64
    p = run_plan(driver, tmp_path, Z, dims)
    assert (p["ncomp"], p["max_vars"], p["max_rows"], p["empty_comps"]) == (3, 48, 96, 0), p
    assert p["feasible"] == 0 and p["nitems"] == 0


def test_an_observation_without_entries_goes_to_component_zero(driver, tmp_path):
    """a row of Z that is all zero has no ELL entry: it joins no variables, and component 0 carries its log f"""
    Z, dims = _kind("rct")
    Z = np.array(Z); Z[100] = 0.0                       # an observation of the last cluster
    p = run_plan(driver, tmp_path, Z, dims)
    assert (p["ncomp"], p["max_vars"], p["max_rows"], p["empty_comps"]) == (7, 6, 16, 0), p
