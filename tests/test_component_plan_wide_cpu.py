"""The host component plan (csrc/component_plan.h) above the trajectory kernel's cap, as plain C++ under AddressSanitizer +
UBSan: tests/host_component_plan_wide_driver.cpp.  Up to CP_WIDE_MAX_VARS = 128 variables per component the plan has the
record arrays the Laplace kernels read (`records`), though no work items for the trajectory kernel (`feasible` keeps its
meaning, max_vars <= 32).  For plans at or below 32 variables the wide constant changes nothing: the counts equal those
host_component_plan_driver.cpp prints, and every array equals a restatement of the layout written here from its
description (compared through an FNV-1a hash of the int32 values)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from glmmrmcml_amd import synth
from test_component_plan_cpu import _dims, _kind, _synth, ell_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP, WIDE_CAP, SLOT, TARGET_ITEMS = 32, 128, 4, 1024          # CP_MAX_VARS, CP_WIDE_MAX_VARS, CP_SLOT, CP_TARGET_ITEMS


def _build(tmp_path_factory, name):
    if shutil.which("g++") is None:
        pytest.fail("g++ not found: the host plan cannot be checked")
    csrc = os.path.join(ROOT, "glmmrmcml_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("cpw") / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + csrc, os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    return exe


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return _build(tmp_path_factory, "host_component_plan_wide_driver"), _build(tmp_path_factory, "host_component_plan_driver")


def run(exe, tmp_path, Z, dims):
    """-> ({field: value} of the "ncomp=" line, the same of the "wide" line or None, the ELL rows)"""
    ell = ell_rows(np.asarray(Z), dims)
    n, Q, W, width, col = ell
    path = str(tmp_path / "ell.txt")
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (n, Q, W))
        f.write(" ".join(map(str, width)) + "\n")
        f.write(" ".join(map(str, col.ravel(order="F"))) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "fails=0" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    out = []
    for key in ("ncomp=", "wide "):
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith(key)), None)
        out.append(None if line is None else {k: int(v) for k, v in (kv.split("=") for kv in line.split() if "=" in kv)})
    return out[0], out[1], ell


def rct(nt):
    s = synth.cluster_rct(2, nt, 2)
    return s["Z"], _dims(s["cov"])


@pytest.mark.parametrize("nt,records", [(32, 1), (127, 1), (128, 0)])
def test_records_above_the_trajectory_cap(drivers, tmp_path, nt, records):
    """components of 33, 128 and 129 variables: never feasible for the trajectory kernel, records up to 128"""
    Z, dims = rct(nt)
    p, w, (n, Q, W, width, col) = run(drivers[0], tmp_path, Z, dims)
    assert (p["ncomp"], p["max_vars"], p["max_rows"], p["empty_comps"]) == (2, nt + 1, 2 * nt, 0), p
    assert p["feasible"] == 0 and p["nitems"] == 0 and p["waves"] == 0 and p["cap"] == CAP, p
    assert w["records"] == records and w["wide_cap"] == WIDE_CAP, w
    assert w["nslots"] == (n if records else 0), w             # rows of ZL two wide: a record each
    old, _, _ = run(drivers[1], tmp_path, Z, dims)             # the existing driver's line is the same
    assert old == p


def fnv(values):
    h = 1469598103934665603
    for b in np.asarray(values, dtype="<i4").tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def expected_arrays(n, Q, W, width, col):
    """the record arrays and work items as component_plan.h describes them, written from that description: components in
    the order of their smallest variable, local indices ascending, observations ascending, records of CP_SLOT entries"""
    parent = list(range(Q))

    def find(q):
        while parent[q] != q:
            q = parent[q]
        return q

    for i in range(n):
        for k in range(1, width[i]):
            a, b = find(col[i, 0]), find(col[i, k])
            parent[max(a, b)] = min(a, b)
    root = [find(q) for q in range(Q)]
    comp_of_root = {r: c for c, r in enumerate(sorted(set(root)))}
    comp = [comp_of_root[r] for r in root]
    ncomp = len(comp_of_root)
    local, cnt = [0] * Q, [0] * ncomp
    for q in range(Q):
        local[q] = cnt[comp[q]]; cnt[comp[q]] += 1
    rows = [[] for _ in range(ncomp)]
    for i in range(n):
        rows[comp[col[i, 0]] if width[i] > 0 else 0].append(i)
    slot_ptr, slot_i, slot_src, slot_quarter = [], [], [], []
    for c in range(ncomp):
        slot_ptr.append(len(slot_i) // 8)
        first = []
        for i in rows[c]:
            first.append(len(slot_i) // 8)
            nrec = max(1, -(-width[i] // SLOT))
            for s in range(nrec):
                ks = list(range(s * SLOT, min(width[i], (s + 1) * SLOT)))
                slot_i += [local[col[i, k]] for k in ks] + [0] * (SLOT - len(ks)) + [len(ks), int(s + 1 == nrec), i, 0]
                slot_src += [i + k * n for k in ks] + [-1] * (SLOT - len(ks))
        first.append(len(slot_i) // 8)
        nr = len(rows[c]); per = (nr + 3) // 4
        slot_quarter += [first[min(w * per, nr)] for w in range(5)]
    slot_ptr.append(len(slot_i) // 8)
    cost = [slot_ptr[c + 1] - slot_ptr[c] + 2 * cnt[c] for c in range(ncomp)]
    target = max(max(cost), -(-sum(cost) // TARGET_ITEMS))
    item_ptr, acc = [0], 0
    for c in range(ncomp):
        if acc > 0 and acc + cost[c] > target:
            item_ptr.append(c); acc = 0
        acc += cost[c]
    item_ptr.append(ncomp)
    return dict(nslots=slot_ptr[-1], h_slot_ptr=fnv(slot_ptr), h_slot_i=fnv(slot_i), h_slot_src=fnv(slot_src),
                h_slot_quarter=fnv(slot_quarter), h_item_ptr=fnv(item_ptr)), max(cnt)


SMALL = {"sw_blk17": lambda: _kind("sw_blk17"),                                # rows of ZL up to 17 wide: five records
         "stepped_wedge_6_8_5": lambda: _synth(synth.stepped_wedge, 6, 8, 5),
         "rct31": lambda: rct(31)}                                              # 32 variables: the last plan with work items


@pytest.mark.parametrize("name", list(SMALL))
def test_plans_up_to_the_trajectory_cap_are_unchanged(drivers, tmp_path, name):
    Z, dims = SMALL[name]()
    p, w, ell = run(drivers[0], tmp_path, Z, dims)
    old, _, _ = run(drivers[1], tmp_path, Z, dims)
    assert old == p and p["feasible"] == 1 and p["nitems"] >= 1, (old, p)
    want, max_vars = expected_arrays(*ell)
    assert max_vars == p["max_vars"] <= CAP
    assert w["records"] == 1
    assert {k: w[k] for k in want} == want


@pytest.mark.parametrize("nt", [32, 127])
def test_records_above_the_cap_follow_the_same_layout(drivers, tmp_path, nt):
    """the record arrays of a plan above 32 variables are the ones the description gives; it has no work items"""
    Z, dims = rct(nt)
    p, w, ell = run(drivers[0], tmp_path, Z, dims)
    want, max_vars = expected_arrays(*ell)
    assert max_vars == nt + 1
    want["h_item_ptr"] = fnv([])
    assert {k: w[k] for k in want} == want
