"""The "component_wide" operator of the Laplace fits (csrc/component.hip k_lac_factor_wg; Context.set_la_operator(
"component_wide")): the component operator of test_gpu_la_component.py for components of up to 128 variables, a wave
(k_lac_factor) or a workgroup of four waves (k_lac_factor_wg) per component.

Tolerances are those of test_gpu_la_component.py: functor values 1e-9 relative to oracle/la.py, the Newton step rtol 1e-8 /
atol 1e-10, sigma 1e-10, against another operator 2e-9 (each is within 1e-9 of the oracle), the drivers through the final
functor 1e-6 with beta atol 2e-3, theta and u atol 5e-3; fallbacks, the untouched "component" mode and repeated runs
bit for bit.  Every positive case asserts la_plan()["operator"] == "component_wide", its waves, the plan's counts and
dense_bytes == 0.  The designs of sections 1 and 2 are checked on the CPU by test_la_component_wide_designs_cpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from glmmrmcml_amd import api, synth
from oracle import la as ola
from test_gpu_component_traj import _blk48, _rct41
from test_gpu_la import CASES as LA_CASES
from test_gpu_la_component import (POINTS, _args, _check_driver, _oracle, _probes, component_context, functor_points, la_design,
                                   with_start)
from test_gpu_sparse_products import _centre, _y, design

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = "component_wide"


# ---------------------------------------------------------------- designs above the old cap
def rct_wide(nt, family, link, ncl=2, nind=2):
    """cluster_rct(ncl, nt, nind): diagonal blocks, components of 1 + nt variables and nt * nind observations; the mean
    replaced by X = 1 and y drawn for the family, as test_gpu_sparse_products.design does it"""
    s = synth.cluster_rct(ncl, nt, nind)
    n, centre = s["n"], _centre(family, link)
    y = _y(family, link, np.full(n, centre), np.random.default_rng(1000 + nt))
    d = dict(cov=s["cov"], data=s["data"], eff_range=s["eff_range"], Z=s["Z"], X=np.ones((n, 1), order="F"), y=y, family=family,
             link=link, beta=np.array([centre]), theta=np.array((0.1, 0.07)), n=n, Q=s["Q"])
    return with_start(d), (ncl, nt + 1, nt * nind)


def rct41(family, link):
    """test_gpu_component_traj._rct41 (3 components of 41 variables, 80 observations each) with y drawn for the family"""
    d = _rct41()
    centre = _centre(family, link)
    y = _y(family, link, np.full(d["n"], centre), np.random.default_rng(1041))
    return with_start(dict(d, y=y, family=family, link=link, beta=np.array([centre]), theta=np.array((0.1, 0.07)))), (3, 41, 80)


def paired_ar1(family, link):
    """stepped_wedge(4, 24, 2): four gr x ar1 blocks of 24 (a non-diagonal L).  Every observation also loads, with weight
    0.6, on a period of the partner cluster (0 <-> 1, 2 <-> 3): the observations couple two covariance blocks into one
    component of 48 variables.  A row of ZL is at most 24 + 24 = 48 wide"""
    blk = 24
    s = synth.stepped_wedge(ncl=4, nt=blk, nind=2)
    Z = np.array(s["Z"], order="F")
    n = s["n"]
    for i in range(n):
        j = int(np.nonzero(Z[i])[0][0])
        b, t = divmod(j, blk)
        Z[i, (b ^ 1) * blk + (t + 5) % blk] = 0.6
    assert (np.count_nonzero(Z, axis=1) == 2).all()
    centre = _centre(family, link)
    y = _y(family, link, np.full(n, centre), np.random.default_rng(1048))
    d = dict(cov=s["cov"], data=s["data"], eff_range=s["eff_range"], Z=Z, X=np.ones((n, 1), order="F"), y=y, family=family,
             link=link, beta=np.array([centre]), theta=np.array((0.1, 0.8)), n=n, Q=s["Q"])
    return with_start(d), (2, 48, 96)


# components of 33 (the first above the old cap), 64, 65 (a lane's second entry starts), 128 (the cap) and 41 variables
ABOVE = [("rct%d" % nt, f, l) for nt in (32, 63, 64, 127) for f, l in (("poisson", "log"), ("binomial", "logit"))] + \
        [("rct64", "gaussian", "identity"), ("rct41", "poisson", "log"), ("rct41", "binomial", "logit")]
ABOVE_IDS = ["%s-%s-%s" % p for p in ABOVE]


def wide_design(name, family, link):
    if name == "rct41":
        return rct41(family, link)
    if name == "paired_ar1":
        return paired_ar1(family, link)
    if name.startswith("rct") and name[3:].isdigit():
        return rct_wide(int(name[3:]), family, link)
    return la_design(name, family, link)


def assert_wide(ctx, counts, waves, launches=None):
    p = ctx.la_plan()
    assert p["requested"] == WIDE and p["operator"] == WIDE, p
    assert p["waves"] == waves, p
    assert (p["ncomp"], p["max_vars"], p["max_rows"]) == tuple(counts), p
    assert p["dense_bytes"] == 0, p
    if launches is not None:
        assert p["launches"] == launches, p
    return p


def check_against_oracle(ctx, d, counts, waves, trials=2):
    """the three functors and the Newton step at the points of test_gpu_la_component.py"""
    gauss = d["family"] == "gaussian"
    rng = np.random.default_rng(11)
    for trial in range(trials):
        v, beta, theta, vp = functor_points(d, rng, trial)
        m = _oracle(d); m.var_par = vp
        want = m.la_objective(np.r_[beta, v])
        got = ctx.la_probe(d["start"], 0, var_par=vp, par=np.r_[beta, v])
        assert_wide(ctx, counts, waves, launches=0)
        print("bv", trial, got, want, abs(got - want) / abs(want))
        assert got == pytest.approx(want, rel=1e-9), ("bv", trial)
        m = _oracle(d); m.var_par = vp; m.v = v.copy(); m.update_W(False)
        par = np.r_[theta, vp] if gauss else theta
        want = m.la_cov_objective(par)
        got = ctx.la_probe(d["start"], 1, v=v, var_par=vp, par=par)
        assert_wide(ctx, counts, waves, launches=1)
        print("cov", trial, got, want, abs(got - want) / abs(want))
        assert got == pytest.approx(want, rel=1e-9), ("cov", trial)
        m = _oracle(d); m.var_par = vp; m.v = v.copy()
        par = np.r_[beta, theta, vp] if gauss else np.r_[beta, theta]
        want = m.la_btheta_objective(par)
        got = ctx.la_probe(d["start"], 2, v=v, var_par=vp, par=par)
        assert_wide(ctx, counts, waves, launches=1)
        print("btheta", trial, got, want, abs(got - want) / abs(want))
        assert got == pytest.approx(want, rel=1e-9), ("btheta", trial)
    rng = np.random.default_rng(5)
    for trial in range(trials):
        v = rng.normal(size=d["Q"]) * 0.2
        vp = 0.7 + 0.2 * trial if gauss else 1.0
        m = _oracle(d)
        m.v = v.copy(); m.var_par = vp
        m.update_W(True)
        m.mcnr_b()
        got = ctx.la_probe(d["start"], 3, v=v, var_par=vp)
        assert_wide(ctx, counts, waves, launches=1)
        print("newton", trial, np.abs(got["v"] - m.v).max(), np.abs(got["beta"] - m.beta).max(), got["sigma"], m.sigma)
        assert np.allclose(got["v"], m.v, rtol=1e-8, atol=1e-10), trial
        assert np.allclose(got["beta"], m.beta, rtol=1e-8, atol=1e-10), trial
        assert got["sigma"] == pytest.approx(m.sigma, rel=1e-10), trial


def wide_context(d, monkeypatch, waves=None):
    """waves: "1" / "4" forces a kernel form (GLMMR_MCML_LA_WAVES, read per call), None leaves the rule"""
    if waves is None:
        monkeypatch.delenv("GLMMR_MCML_LA_WAVES", raising=False)
    else:
        monkeypatch.setenv("GLMMR_MCML_LA_WAVES", waves)
    return component_context(d, monkeypatch, mode=WIDE)


def assert_close(a, b, tol=2e-9):
    (fa, sa), (fb, sb) = a, b
    assert np.abs(fa - fb).max() <= tol * np.abs(fa).max(), (fa, fb)
    for k in ("v", "beta"):
        assert np.abs(sa[k] - sb[k]).max() <= tol * max(1.0, np.abs(sa[k]).max()), k
    assert sb["sigma"] == pytest.approx(sa["sigma"], rel=tol)


def assert_same(a, b):
    (fa, sa), (fb, sb) = a, b
    assert np.array_equal(fa, fb)
    for k in ("v", "beta"):
        assert np.array_equal(sa[k], sb[k]), k
    assert sa["sigma"] == sb["sigma"]


# ---------------------------------------------------------------- 1) above the old cap, against the oracle
@pytest.mark.parametrize("name,family,link", ABOVE, ids=ABOVE_IDS)
def test_above_the_old_cap_matches_oracle(orc, name, family, link, monkeypatch):
    d, counts = wide_design(name, family, link)
    assert 32 < counts[1] <= 128 and d["Q"] <= 256 and d["n"] <= 508
    with wide_context(d, monkeypatch) as ctx:
        check_against_oracle(ctx, d, counts, 4)


def test_forcing_one_wave_above_the_old_cap_is_ignored(monkeypatch):
    d, counts = wide_design("rct32", "poisson", "log")
    with wide_context(d, monkeypatch, waves="1") as ctx:
        a = _probes(ctx, d, np.random.default_rng(23))
        assert_wide(ctx, counts, 4)
    with wide_context(d, monkeypatch) as ctx:
        b = _probes(ctx, d, np.random.default_rng(23))
    assert_same(a, b)


# ---------------------------------------------------------------- 2) a component above 32 with a non-diagonal L
@pytest.mark.parametrize("family,link", [("poisson", "log"), ("binomial", "logit")])
def test_two_coupled_ar1_blocks(orc, family, link, monkeypatch):
    d, counts = wide_design("paired_ar1", family, link)
    with wide_context(d, monkeypatch) as ctx:
        check_against_oracle(ctx, d, counts, 4)
        wide = _probes(ctx, d, np.random.default_rng(23))
        assert_wide(ctx, counts, 4)
        ctx.set_la_operator("dense")
        dense = _probes(ctx, d, np.random.default_rng(23))
        p = ctx.la_plan()
        assert p["operator"] == "dense" and p["waves"] == 0 and p["launches"] == 0, p
    assert_close(dense, wide)


# ---------------------------------------------------------------- 3) the rule and both forms
@pytest.mark.parametrize("name,waves", [("sw_long_ragged", 4), ("rct", 1)])
def test_the_rule(orc, name, waves, monkeypatch):
    """200 observations in the largest component: a workgroup each; 15: a wave each"""
    d, counts = la_design(name, "binomial", "logit")
    with wide_context(d, monkeypatch) as ctx:
        check_against_oracle(ctx, d, counts, waves, trials=1)


# rct: 15 observations, a partial batch and idle waves; sw_short_drop: a component without observations; dup: a local
# column twice in a row of ZL; empty_row: an observation without entries; cap32: one component of 32
FORCED = [p for p in POINTS if p[0] in ("rct", "sw_short_drop", "dup", "empty_row", "cap32")] + [("sw_blk16", "gaussian", "identity")]


@pytest.mark.parametrize("name,family,link", FORCED, ids=["%s-%s-%s" % p for p in FORCED])
def test_the_workgroup_form_on_small_components(orc, name, family, link, monkeypatch):
    d, counts = la_design(name, family, link)
    with wide_context(d, monkeypatch, waves="4") as ctx:
        check_against_oracle(ctx, d, counts, 4)


def test_more_components_than_partial_sums(monkeypatch):
    """longitudinal(1200, 2), a workgroup per component: 1200 of them, more than the 1100 partial sums of the other
    reductions.  Against the dense operator"""
    d = synth.longitudinal(1200, 2)
    with wide_context(d, monkeypatch, waves="4") as ctx:
        wide = _probes(ctx, d, np.random.default_rng(23))
        assert_wide(ctx, (1200, 3, 2), 4)
        ctx.set_la_operator("dense")
        dense = _probes(ctx, d, np.random.default_rng(23))
        assert ctx.la_plan()["operator"] == "dense"
    assert_close(dense, wide)


# ---------------------------------------------------------------- 4) agreement between the operators, repeatability
@pytest.mark.parametrize("name,family,link", [("rct", "poisson", "log"), ("sw_long_ragged", "binomial", "logit"),
                                              ("sw_blk16", "gaussian", "identity")])
def test_both_forms_against_component(name, family, link, monkeypatch):
    d, counts = la_design(name, family, link)
    with component_context(d, monkeypatch, mode="component") as ctx:
        ref = _probes(ctx, d, np.random.default_rng(23))
        p = ctx.la_plan()
        assert p["operator"] == "component" and p["waves"] == 1, p
        ctx.set_la_operator(WIDE)
        for waves in (1, 4):
            monkeypatch.setenv("GLMMR_MCML_LA_WAVES", str(waves))
            got = _probes(ctx, d, np.random.default_rng(23))
            assert_wide(ctx, counts, waves, launches=1)
            assert_close(ref, got)
            if waves == 1:
                assert_same(ref, got)          # the same kernel


@pytest.mark.parametrize("name,waves", [("rct41", None), ("sw_long_ragged", None), ("rct", "4"), ("rct", None)])
def test_two_runs_are_bit_identical(name, waves, monkeypatch):
    d, counts = wide_design(name, "binomial", "logit")
    with wide_context(d, monkeypatch, waves=waves) as ctx:
        a = _probes(ctx, d, np.random.default_rng(23))
        ra = ctx.mcml_la(d["start"], nr=True, maxiter=2, maxfun=40)
        b = _probes(ctx, d, np.random.default_rng(23))
        rb = ctx.mcml_la(d["start"], nr=True, maxiter=2, maxfun=40)
        p = ctx.la_plan()
        assert p["operator"] == WIDE and p["launches"] > 0 and p["dense_bytes"] == 0, p
    assert_same(a, b)
    for k in ("beta", "theta", "u"):
        assert np.array_equal(ra[k], rb[k]), k


# ---------------------------------------------------------------- 5) fallbacks
def _fallback_cases():
    geo = synth.geospatial(40, seed=3)
    s = synth.cluster_rct(2, 128, 2)
    return {"above_128": (dict(s, beta=np.array([0.2]), X=np.ones((s["n"], 1), order="F")), None),
            "block_above_small": (_blk48(), None),
            "geospatial": (dict(geo, start=np.r_[geo["beta"], geo["theta"], 0.8]), None),
            "zl_dense": (design("rct", "poisson", "log"), "dense")}


@pytest.mark.parametrize("which", ["above_128", "block_above_small", "geospatial", "zl_dense"])
def test_fallbacks_run_the_dense_path_bit_for_bit(which, monkeypatch):
    """"component_wide" requested where it cannot run: cluster_rct(2, 128, 2) (components of 129 variables),
    stepped_wedge(3, 48, 2) (blocks above SMALL_BLOCK: no sparse operator), a geospatial model (a dense Z), and
    GLMMR_MCML_ZL=dense on a design that would otherwise qualify"""
    d, zl = _fallback_cases()[which]
    if "start" not in d or len(d["start"]) != d["beta"].size + d["theta"].size + (d["family"] == "gaussian"):
        d = with_start(d)
    monkeypatch.delenv("GLMMR_MCML_LA_WAVES", raising=False)
    if zl is None:
        monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    else:
        monkeypatch.setenv("GLMMR_MCML_ZL", zl)
    out = {}
    for mode in (None, WIDE):
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
            if mode is not None:
                ctx.set_la_operator(mode)
            f, st = _probes(ctx, d, np.random.default_rng(23))
            p = ctx.la_plan()
            assert p["requested"] == (mode or "dense") and p["operator"] == "dense" and p["launches"] == 0 and p["waves"] == 0, p
            fit = ctx.mcml_la(d["start"], nr=True, maxiter=2, maxfun=40)
            p = ctx.la_plan()
            assert p["operator"] == "dense" and p["launches"] == 0 and p["waves"] == 0 and p["dense_bytes"] > 0, p
            if which == "above_128" and mode is not None:
                assert p["ncomp"] == 2 and p["max_vars"] == 129, p
            out[mode] = (f, st, fit)
    (fa, sa, ra), (fb, sb, rb) = out[None], out[WIDE]
    assert_same((fa, sa), (fb, sb))
    for k in ("beta", "theta", "u"):
        assert np.array_equal(ra[k], rb[k]), k
    assert ra["sigma"] == rb["sigma"] and ra["iters"] == rb["iters"]


# ---------------------------------------------------------------- 6) "component" is unchanged
def test_component_keeps_its_cap(monkeypatch):
    """41 variables per component under "component": the dense path, bit for bit what an unset context runs"""
    monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    d = with_start(_rct41())
    out = {}
    for mode in (None, "component"):
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
            if mode is not None:
                ctx.set_la_operator(mode)
            out[mode] = _probes(ctx, d, np.random.default_rng(23))
            p = ctx.la_plan()
            assert p["requested"] == (mode or "dense") and p["operator"] == "dense" and p["launches"] == 0 and p["waves"] == 0, p
    assert_same(out[None], out["component"])


# ---------------------------------------------------------------- 7) drivers and interface
def _rct41_driver():
    """the one-shot exports size theta from a start that ends with the slot of sigma, as the reference's does"""
    d = _rct41()
    return dict(d, start=np.r_[d["beta"], d["theta"], 1.0])


def test_mcml_la_nr_matches_oracle_driver(monkeypatch):
    monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    monkeypatch.delenv("GLMMR_MCML_LA_WAVES", raising=False)
    d = _rct41_driver()
    want = ola.mcml_la_nr(*_args(d), maxiter=6)
    n0 = api.la_component_launches()
    got = api.mcml_la_nr(*_args(d), verbose=False, maxiter=6, operator=WIDE)      # the one-shot export
    assert api.la_component_launches() > n0 and api.get_default_la_operator() == "dense"
    assert got["u"].shape == (d["Q"], 1)
    _check_driver(d, got, want)
    with api.Context(*_args(d)[:-1]) as ctx:
        same = ctx.mcml_la(d["start"], nr=True, maxiter=6, operator=WIDE)
        p = ctx.la_plan()
        assert p["requested"] == "dense" and p["operator"] == WIDE and p["waves"] == 4 and p["launches"] > 0, p
        assert p["dense_bytes"] == 0 and (p["ncomp"], p["max_vars"], p["max_rows"]) == (3, 41, 80), p
    for k in ("beta", "theta"):
        assert np.array_equal(got[k], same[k]), k
    assert np.array_equal(got["u"].ravel(), same["u"])


_ENV_SCRIPT = """
import json, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from glmmrmcml_amd import api
from test_gpu_component_traj import _rct41
d = _rct41()
start = np.r_[d["beta"], d["theta"], 1.0]
args = (d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"])
default = api.get_default_la_operator()
n0 = api.la_component_launches()
r = api.mcml_la_nr(*args, start, verbose=False, maxiter=3)
with api.Context(*args) as ctx:
    requested = ctx.la_plan()["requested"]
print("RESULT " + json.dumps(dict(default=default, requested=requested, launches=api.la_component_launches() - n0,
                                  beta=r["beta"].tolist(), theta=r["theta"].tolist())))
"""


def test_one_shot_export_under_the_environment_variable(monkeypatch):
    """GLMMR_MCML_LA=component_wide is read once per process: a fresh interpreter"""
    monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    monkeypatch.delenv("GLMMR_MCML_LA_WAVES", raising=False)
    env = dict(os.environ, GLMMR_MCML_LA=WIDE)
    out = subprocess.run([sys.executable, "-c", _ENV_SCRIPT % (ROOT, os.path.join(ROOT, "tests"))], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(next(l for l in out.stdout.splitlines() if l.startswith("RESULT "))[7:])
    assert r["default"] == WIDE and r["requested"] == WIDE and r["launches"] > 0, r
    d = _rct41_driver()
    with api.Context(*_args(d)[:-1]) as ctx:
        same = ctx.mcml_la(d["start"], nr=True, maxiter=3, operator=WIDE)
    assert np.array_equal(np.array(r["beta"]), same["beta"]) and np.array_equal(np.array(r["theta"]), same["theta"])


def test_model_caller_passes_the_choice_and_restores_it(monkeypatch):
    """ModelMCML.LA(operator="component_wide") sets the backend default for the duration of the call"""
    from glmmrmcml_amd.model import ModelMCML
    monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    monkeypatch.delenv("GLMMR_MCML_LA_WAVES", raising=False)
    assert api.get_default_la_operator() == "dense"
    seen = []

    class Spy:
        def __getattr__(self, name):
            return getattr(api, name)

        def mcml_la_nr(self, *a, **k):
            n0 = api.la_component_launches()
            r = api.mcml_la_nr(*a, **k)
            seen.append((api.get_default_la_operator(), api.la_component_launches() > n0))
            return r

    d = synth.cluster_rct(ncl=8, nt=3, nind=8, seed=5, family="poisson")
    mod = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["family"], d["link"], d["beta"], d["theta"],
                    backend=Spy())
    fit = {}
    try:
        api.set_default_la_operator("component")
        for op in (WIDE, None):
            fit[op] = mod.LA(d["y"], method="nr", operator=op)
        assert seen == [(WIDE, True), ("component", True)] and api.get_default_la_operator() == "component"
    finally:
        api.set_default_la_operator("dense")
    assert np.abs(fit[WIDE].theta - fit[None].theta).max() <= 2e-9 * max(1.0, np.abs(fit[None].theta).max())


@pytest.mark.parametrize("traj", ["step", "component"])
def test_la_keeps_the_context_usable(traj, monkeypatch):
    """after a component_wide call on components of 41 variables the sampler's draws equal those of a context that never
    ran a Laplace fit, in both trajectory modes (the plan has records but no work items: "component" runs per step)"""
    monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    monkeypatch.delenv("GLMMR_MCML_LA_WAVES", raising=False)
    d = with_start(_rct41())
    out = {}
    for la in (False, True):
        with api.Context(*_args(d)[:-1]) as ctx:
            ctx.set_trajectory(traj)
            if la:
                r = ctx.mcml_la(d["start"], nr=True, maxiter=2, operator=WIDE)
                p = ctx.la_plan()
                assert np.all(np.isfinite(r["beta"])) and p["operator"] == WIDE and p["waves"] == 4, p
            ctx.update_L(d["theta"])
            dg = ctx.hmc_sample(d["beta"], 1.0, 5, 8, 0.05, 10, 0.9, seed=3, chains=8)
            assert dg["accept_rate"] > 0
            assert ctx.last_kernels() == ("sparse",) * 2
            out[la] = ctx.get_u()
    assert np.array_equal(out[False], out[True])
