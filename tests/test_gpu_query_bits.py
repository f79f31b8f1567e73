"""The bits of the queries on the component operator, pinned where their copied code was given one home: the substitution
kernels, the CSR right-hand side and the factor scratch (csrc/component.hip), the Gram reduction, the flagged tail and the row
sum x_i' beta (csrc/info.hip, csrc/glm.h), which the information query, the sandwich and the component-wise exact draws share.
The reference tests judge each result within a bound; they cannot see a last digit that moves when two kernels become one, a
group of staged components changes its size or a sum is regrouped.  Here the SHA-256 of what a call returns is compared with
tests/golden/query_bits.json, recorded from the library of the commit named there (tests/golden/make_query_bits.py: never
from the code under test).

  info_<key>      Context.information_matrix on a fresh context, theta given:
                  family-*              6 components of 4 variables, one per family / link: the twelve branches of the weights
                  longitudinal_70x3     70 components: more than 64 (component, column) pairs in a group, several groups
                  stepped_wedge_7x8x3   8 variables: stride 37, P = 9
                  wide_41, wide_41_p71  one component per wave; P = 71 runs a second chunk of columns
                  geo150_p1, densez_poisson_log   the dense operator: the Gram reduction and the tail alone, P = 1 and P = 3
  sand_<name>     Context.sandwich(scores=True): information, meat and scores.  The same component and wide names (the back
                  sweep of the lane-per-component form and of the cooperative one-wave form) and densez_poisson_log.  Every case
                  has fewer than 2048 clusters: the meat's ONE-CHUNK path is what is pinned, the sum over several chunks is
                  test_gpu_sandwich's meat bound's
  exact_<design>  Context.exact_sample(operator="component") at a fixed seed, 80 columns: rct (staged) and rct32 (33 variables,
                  one component per wave): the factor scratch the draws share with the queries
The input hashes are asserted first: a changed numpy stream fails there instead of comparing different problems."""
import hashlib
import json
import os

import numpy as np
import pytest

import information_reference as ir
import sandwich_reference as sr
from test_gpu_la_component_wide import wide_design
from test_gpu_sparse_products import context as sparse_context

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "query_bits.json")
ENV = ("GLMMR_MCML_LA_WAVES", "GLMMR_MCML_SAND_SCORES", "GLMMR_MCML_GEMM", "GLMMR_MCML_ZL")
COMPONENT_NAMES = ir.FAMILY_KEYS + ir.COMPONENT_KEYS + ir.WIDE_KEYS
EXACT_SEED, EXACT_SIGMA = 20240601, 0.8


def sha256(*arrays):
    """of the arrays' values as float64 in column-major order, one after the other"""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.asarray(a, dtype=np.float64).tobytes(order="F"))
    return h.hexdigest()


def _inputs(c, *more):
    return sha256(c["Z"], c["X"], c["y"], c["cov"], c["data"], c["eff_range"], c["beta"], c["theta"], *more)


def _context(c):
    from glmmrmcml_amd import api
    return api.Context(c["cov"], c["data"], c["eff_range"], c["Z"], c["X"], c["y"], c["family"], c["link"])


def info(key):
    def run(mp):
        c = ir.case(key)
        with _context(c) as ctx:
            got = ctx.information_matrix(c["beta"], c["var_par"], theta=c["theta"])
            assert ctx.information_plan()["op"] == c["op"]
        return dict(inputs=_inputs(c, [c["var_par"]]), information=sha256(got))
    return run


def sand(name, op):
    def run(mp):
        c = sr.case(name)
        with _context(c) as ctx:
            r = ctx.sandwich(c["beta"], c["var_par"], theta=c["theta"], cluster=c["cluster"], scores=True)
            assert ctx.sandwich_plan()["op"] == op and r["ncluster"] < 2048
        cluster = [] if c["cluster"] is None else c["cluster"]
        return dict(inputs=_inputs(c, [c["var_par"]], cluster), information=sha256(r["information"]), meat=sha256(r["meat"]),
                    scores=sha256(r["scores"]))
    return run


def exact(design, staged):
    def run(mp):
        d, counts = wide_design(design, "gaussian", "identity")
        assert (counts[1] <= 32) == staged, counts
        with sparse_context(d, mp, None) as ctx:
            p = ctx.exact_component_plan()
            assert p["applicable"] and (p["ncomp"], p["max_vars"], p["max_rows"]) == tuple(counts), p
            ctx.exact_sample(d["beta"], EXACT_SIGMA, 80, EXACT_SEED, chains=40, chain_offset=3, iter_idx=2, operator="component")
            assert ctx.last_kernels() == ("exact_component", "exact_component")
            u = ctx.get_u()
        assert u.shape == (d["Q"], 80)
        return dict(inputs=_inputs(d), samples=sha256(u))
    return run


CASES = {"info_" + k: info(k) for k in COMPONENT_NAMES + ["geo150_p1", "densez_poisson_log"]}
CASES.update({"sand_" + k: sand(k, ir.case(k)["op"]) for k in COMPONENT_NAMES + ["densez_poisson_log"]})
CASES.update({"exact_rct": exact("rct", True), "exact_rct32": exact("rct32", False)})


def digests(name, mp):
    """{"inputs": .., ...} of a case through the library that is loaded; mp: a pytest.MonkeyPatch"""
    for k in ENV:
        mp.delenv(k, raising=False)
    return CASES[name](mp)


@pytest.mark.parametrize("name", list(CASES))
def test_query_bits_are_the_recorded_ones(name, monkeypatch):
    with open(FIXTURE) as f:
        want = json.load(f)["cases"][name]
    got = digests(name, monkeypatch)
    assert got["inputs"] == want["inputs"], "the seeded inputs are not the recorded ones (numpy stream changed?)"
    for key in sorted(want):
        print(name, key, got[key])
    for key in sorted(want):
        assert got[key] == want[key], "%s: %s differs from the bits recorded in %s" % (name, key, FIXTURE)
    assert set(got) == set(want)
