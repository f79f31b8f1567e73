"""The component operator of the Laplace fits (csrc/component.hip; Context.set_la_operator("component")): on a
block-structured design M = ZL' W ZL + I is block diagonal over the connected components of ZL's coupling graph, and the
functors, the Newton step and the drivers run on the sparse ZL operator with M built, factorised and solved one component
at a time.

Checked against the oracle restatement (oracle/la.py) with the tolerances of test_gpu_la.py -- functor values 1e-9
relative, the Newton step rtol 1e-8 / atol 1e-10, sigma 1e-10, the drivers through the final functor 1e-6 with beta atol
2e-3, theta and u atol 5e-3 --, against the dense operator on the same context (2e-9 relative: each is within 1e-9 of
the oracle), for the fallbacks and the untouched default (bit for bit), for repeatability (bit for bit), through the
one-shot exports and ModelMCML.LA.  Every positive case asserts la_plan()["operator"] == "component" and the plan's counts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from glmmrmcml_amd import api, synth
from oracle import la as ola
from oracle import oracle as orc_mod
from test_gpu_component_traj import DESIGNS, _blk48, _rct41
from test_gpu_la import CASES as LA_CASES
from test_gpu_sparse_products import _last_effect_design, context, design

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = [("poisson", "log"), ("binomial", "logit")]


def with_start(d):
    start = np.r_[d["beta"], d["theta"]]
    if d["family"] == "gaussian":
        start = np.r_[start, 0.8]
    return dict(d, start=start)


def dup_design(family, link):
    """sw_short with a second nonzero of Z in the observation's own covariance block (two periods of its cluster, the
    second weighted 0.6): a row of ZL then holds the local columns of the shorter run twice"""
    d = design("sw_short", family, link)
    blk = max(d["dims"])
    Z = d["Z"].copy()
    for i in range(d["n"]):
        j = int(np.nonzero(Z[i])[0][0])
        b0 = blk * (j // blk)
        Z[i, b0 + (j - b0 + 2) % blk] = 0.6
    assert (np.count_nonzero(Z, axis=1) == 2).all()
    return dict(d, Z=np.asfortranarray(Z))


def empty_row_design(family, link):
    """test_gpu_component_traj.test_an_observation_without_entries: observation 4 loads on nothing"""
    d = design("rct", family, link)
    Z = d["Z"].copy(); Z[4] = 0.0
    return dict(d, Z=np.asfortranarray(Z))


def la_design(name, family, link):
    """-> (design with start, (components, most variables, most observations))"""
    if name == "cap32":                               # one block of 32, every observation on its last effect: one component at the cap
        return with_start(_last_effect_design(1, 32, family, link)), (1, 32, 40)
    if name == "dup":
        return with_start(dup_design(family, link)), (6, 5, 15)
    if name == "empty_row":
        return with_start(empty_row_design(family, link)), (7, 6, 15)
    kind, opts, ncomp, max_vars, max_rows, empty = DESIGNS[name]
    return with_start(design(kind, family, link, **opts)), (ncomp, max_vars, max_rows)


SMALL = ["tiny", "rct", "sw_short_drop", "sw_short_slope", "sw_long_ragged", "sw_blk8", "sw_blk12", "sw_blk16", "cap32", "dup",
         "empty_row"]
POINTS = [(name, f, l) for name in SMALL for f, l in FAMILIES] + \
         [("sw_blk16", "gaussian", "identity"), ("rct", "gaussian", "identity"), ("rct", "gamma", "log")]
IDS = ["%s-%s-%s" % p for p in POINTS]


def _oracle(d):
    return ola.LaModel(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"], d["start"])


def component_context(d, monkeypatch, mode="component"):
    ctx = context(d, monkeypatch, None)
    if mode is not None:
        ctx.set_la_operator(mode)
    return ctx


def assert_component(ctx, counts, launches=None):
    p = ctx.la_plan()
    assert p["requested"] == "component" and p["operator"] == "component", p
    assert (p["ncomp"], p["max_vars"], p["max_rows"]) == tuple(counts), p
    assert p["dense_bytes"] == 0, p
    if launches is not None:
        assert p["launches"] == launches, p
    return p


def functor_points(d, rng, trial):
    """as test_gpu_la.test_functors_match_oracle draws them"""
    gauss = d["family"] == "gaussian"
    v = rng.normal(size=d["Q"]) * 0.3
    beta = d["beta"] + rng.normal(size=d["beta"].size) * 0.1
    theta = d["theta"] * (1 + 0.3 * rng.random(d["theta"].size))
    vp = 0.7 + 0.2 * trial if gauss else 1.0
    return v, beta, theta, vp


# ---------------------------------------------------------------- 1) functors and the Newton step against the oracle
@pytest.mark.parametrize("name,family,link", POINTS, ids=IDS)
def test_functors_match_oracle(orc, name, family, link, monkeypatch):
    d, counts = la_design(name, family, link)
    gauss = family == "gaussian"
    rng = np.random.default_rng(11)
    with component_context(d, monkeypatch) as ctx:
        for trial in range(3):
            v, beta, theta, vp = functor_points(d, rng, trial)
            m = _oracle(d); m.var_par = vp
            want = m.la_objective(np.r_[beta, v])
            got = ctx.la_probe(d["start"], 0, var_par=vp, par=np.r_[beta, v])
            assert_component(ctx, counts, launches=0)
            assert got == pytest.approx(want, rel=1e-9), ("bv", trial)
            m = _oracle(d); m.var_par = vp; m.v = v.copy(); m.update_W(False)
            par = np.r_[theta, vp] if gauss else theta
            want = m.la_cov_objective(par)
            got = ctx.la_probe(d["start"], 1, v=v, var_par=vp, par=par)
            assert_component(ctx, counts, launches=1)
            assert got == pytest.approx(want, rel=1e-9), ("cov", trial)
            m = _oracle(d); m.var_par = vp; m.v = v.copy()
            par = np.r_[beta, theta, vp] if gauss else np.r_[beta, theta]
            want = m.la_btheta_objective(par)
            got = ctx.la_probe(d["start"], 2, v=v, var_par=vp, par=par)
            assert_component(ctx, counts, launches=1)
            assert got == pytest.approx(want, rel=1e-9), ("btheta", trial)


@pytest.mark.parametrize("name,family,link", POINTS, ids=IDS)
def test_mcnr_b_step_matches_oracle(orc, name, family, link, monkeypatch):
    d, counts = la_design(name, family, link)
    rng = np.random.default_rng(5)
    with component_context(d, monkeypatch) as ctx:
        for trial in range(3):
            v = rng.normal(size=d["Q"]) * 0.2
            vp = 0.7 + 0.2 * trial if family == "gaussian" else 1.0
            m = _oracle(d)
            m.v = v.copy(); m.var_par = vp
            m.update_W(True)
            m.mcnr_b()
            got = ctx.la_probe(d["start"], 3, v=v, var_par=vp)
            assert_component(ctx, counts, launches=1)
            assert np.allclose(got["v"], m.v, rtol=1e-8, atol=1e-10), trial
            assert np.allclose(got["beta"], m.beta, rtol=1e-8, atol=1e-10), trial
            assert got["sigma"] == pytest.approx(m.sigma, rel=1e-10), trial


def test_long_wide(orc, monkeypatch):
    """410 components (103 workgroups of k_lac_factor, the last one half empty), Q = 4100.  One functor (kind 1) and one
    Newton step.  D is diagonal, so the oracle's factor is sqrt(D) instead of a dense Cholesky of 4100 x 4100 (as
    test_gpu_component_traj does it)"""
    d, counts = la_design("long_wide", "poisson", "log")
    assert counts[0] % 4 != 0 and d["Q"] > 4096
    dense_gen_D = orc_mod.gen_D

    def diag_gen_D(cov, data, eff_range, theta, chol=False):
        D = dense_gen_D(cov, data, eff_range, theta, chol=False)
        assert np.count_nonzero(D) == D.shape[0]
        return np.sqrt(D) if chol else D

    monkeypatch.setattr(ola.orc, "gen_D", diag_gen_D)
    rng = np.random.default_rng(11)
    v, beta, theta, vp = functor_points(d, rng, 0)
    m = _oracle(d); m.v = v.copy(); m.update_W(False)
    want = m.la_cov_objective(theta)
    m.v = v.copy(); m.update_W(True); m.mcnr_b()
    with component_context(d, monkeypatch) as ctx:
        got = ctx.la_probe(d["start"], 1, v=v, par=theta)
        assert_component(ctx, counts, launches=1)
        st = ctx.la_probe(d["start"], 3, v=v)
        assert_component(ctx, counts, launches=1)
    assert got == pytest.approx(want, rel=1e-9)
    assert np.allclose(st["v"], m.v, rtol=1e-8, atol=1e-10)
    assert np.allclose(st["beta"], m.beta, rtol=1e-8, atol=1e-10)
    assert st["sigma"] == pytest.approx(m.sigma, rel=1e-10)


# ---------------------------------------------------------------- 2) component against dense on the same context
def _probes(ctx, d, rng):
    v, beta, theta, vp = functor_points(d, rng, 1)
    gauss = d["family"] == "gaussian"
    out = [ctx.la_probe(d["start"], 0, var_par=vp, par=np.r_[beta, v]),
           ctx.la_probe(d["start"], 1, v=v, var_par=vp, par=np.r_[theta, vp] if gauss else theta),
           ctx.la_probe(d["start"], 2, v=v, var_par=vp, par=np.r_[beta, theta, vp] if gauss else np.r_[beta, theta])]
    st = ctx.la_probe(d["start"], 3, v=v, var_par=vp)
    return np.array(out), st


@pytest.mark.parametrize("name,family,link", [("rct", "poisson", "log"), ("sw_short_drop", "binomial", "logit"),
                                              ("sw_blk16", "gaussian", "identity"), ("dup", "poisson", "log"),
                                              ("sw_long_ragged", "binomial", "logit")])
def test_component_against_dense(name, family, link, monkeypatch):
    d, counts = la_design(name, family, link)
    out = {}
    with component_context(d, monkeypatch, mode=None) as ctx:
        for mode in ("dense", "component"):
            ctx.set_la_operator(mode)
            out[mode] = _probes(ctx, d, np.random.default_rng(23))
            p = ctx.la_plan()
            assert p["operator"] == mode and (p["launches"] > 0) == (mode == "component"), p
    (fd, sd), (fc, sc) = out["dense"], out["component"]
    assert np.abs(fd - fc).max() <= 2e-9 * np.abs(fd).max(), (fd, fc)
    for k in ("v", "beta"):
        assert np.abs(sd[k] - sc[k]).max() <= 2e-9 * max(1.0, np.abs(sd[k]).max()), k
    assert sc["sigma"] == pytest.approx(sd["sigma"], rel=2e-9)


def test_more_components_than_partial_sums(monkeypatch):
    """longitudinal(1200, 2): 1200 components of 3 variables and 2 observations, more than the 1100 partial sums the other reductions of the
    Laplace path keep -- the per-component log-determinants have a buffer of their own.  Against the dense operator"""
    monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    d = synth.longitudinal(1200, 2)
    out = {}
    with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
        for mode in ("dense", "component"):
            ctx.set_la_operator(mode)
            out[mode] = _probes(ctx, d, np.random.default_rng(23))
            p = ctx.la_plan()
            assert p["operator"] == mode, p
        assert (p["ncomp"], p["max_vars"], p["max_rows"]) == (1200, 3, 2) and p["ncomp"] > 1100, p
    (fd, sd), (fc, sc) = out["dense"], out["component"]
    assert np.abs(fd - fc).max() <= 2e-9 * np.abs(fd).max(), (fd, fc)
    for k in ("v", "beta"):
        assert np.abs(sd[k] - sc[k]).max() <= 2e-9 * max(1.0, np.abs(sd[k]).max()), k


# ---------------------------------------------------------------- 3) fallbacks
def _fallback_cases():
    geo = synth.geospatial(40, seed=3)
    return {"above_cap": (_rct41(), None), "block_above_small": (_blk48(), None),
            "geospatial": (dict(geo, start=np.r_[geo["beta"], geo["theta"], 0.8]), None),
            "zl_dense": (design("rct", "poisson", "log"), "dense")}


@pytest.mark.parametrize("which", ["above_cap", "block_above_small", "geospatial", "zl_dense"])
def test_fallbacks_run_the_dense_path_bit_for_bit(which, monkeypatch):
    """"component" requested where it cannot run: cluster_rct(3, 40, 2) (the sparse operator possible, components of 41
    variables), stepped_wedge(3, 48, 2) (blocks above SMALL_BLOCK: no sparse operator), a geospatial model, and
    GLMMR_MCML_ZL=dense on a design that would otherwise qualify"""
    d, zl = _fallback_cases()[which]
    if "start" not in d or len(d["start"]) != d["beta"].size + d["theta"].size + (d["family"] == "gaussian"):
        d = with_start(d)
    if zl is None:
        monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    else:
        monkeypatch.setenv("GLMMR_MCML_ZL", zl)
    out = {}
    for mode in (None, "component"):
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
            if mode is not None:
                ctx.set_la_operator(mode)
            f, st = _probes(ctx, d, np.random.default_rng(23))
            p = ctx.la_plan()
            assert p["requested"] == (mode or "dense") and p["operator"] == "dense" and p["launches"] == 0, p
            fit = ctx.mcml_la(d["start"], nr=True, maxiter=2, maxfun=40)
            p = ctx.la_plan()
            assert p["operator"] == "dense" and p["launches"] == 0 and p["dense_bytes"] > 0, p
            if which == "above_cap" and mode is not None:
                assert p["ncomp"] == 3 and p["max_vars"] == 41, p
            out[mode] = (f, st, fit)
    (fa, sa, ra), (fb, sb, rb) = out[None], out["component"]
    assert np.array_equal(fa, fb)
    for k in ("v", "beta"):
        assert np.array_equal(sa[k], sb[k]), k
    assert sa["sigma"] == sb["sigma"]
    for k in ("beta", "theta", "u"):
        assert np.array_equal(ra[k], rb[k]), k
    assert ra["sigma"] == rb["sigma"] and ra["iters"] == rb["iters"]


# ---------------------------------------------------------------- 4) nothing set is the dense path
def test_nothing_set_is_the_dense_path(monkeypatch):
    monkeypatch.delenv("GLMMR_MCML_LA", raising=False)
    monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    assert api.get_default_la_operator() == "dense"

    def run():
        out = {}
        for name, d in LA_CASES.items():
            with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
                p = ctx.la_plan()
                assert p["requested"] == "dense" and p["operator"] == "dense" and p["launches"] == 0, p
                out[name] = _probes(ctx, d, np.random.default_rng(23))
                p = ctx.la_plan()
                assert p["operator"] == "dense" and p["launches"] == 0, p
        return out

    before = run()
    d = LA_CASES["poisson"]
    with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
        ctx.set_la_operator("component")
        ctx.mcml_la(d["start"], nr=True, maxiter=2)
        assert ctx.la_plan()["operator"] == "component"
    after = run()
    for name in LA_CASES:
        assert np.array_equal(before[name][0], after[name][0]), name
        for k in ("v", "beta"):
            assert np.array_equal(before[name][1][k], after[name][1][k]), (name, k)
        assert before[name][1]["sigma"] == after[name][1]["sigma"], name


# ---------------------------------------------------------------- 5) no dense allocation
@pytest.mark.parametrize("name", ["poisson", "binomial"])
def test_no_dense_matrix_is_allocated(name, monkeypatch):
    monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    d = LA_CASES[name]
    with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
        ctx.set_la_operator("component")
        r = ctx.mcml_la(d["start"], nr=True, maxiter=2)
        p = ctx.la_plan()
        assert p["operator"] == "component" and p["dense_bytes"] == 0 and p["launches"] > 0, p
        assert np.all(np.isfinite(r["beta"])) and np.all(np.isfinite(r["theta"]))
        ctx.set_la_operator("dense")
        ctx.mcml_la(d["start"], nr=True, maxiter=1, maxfun=20)
        p = ctx.la_plan()
        # M (Q x Q), ZLTW, ZL and ZLT (Q x n, n x Q, Q x n) of the dense path
        assert p["operator"] == "dense" and p["launches"] == 0 and p["dense_bytes"] >= 8 * d["Q"] * (d["Q"] + 3 * d["n"]), p


# ---------------------------------------------------------------- 6) drivers
def _check_driver(d, got, want):
    m = _oracle(d); m.v = want["v"].copy()
    f_want = m.la_btheta_objective(np.r_[want["beta"], want["theta"]])
    f_got = m.la_btheta_objective(np.r_[got["beta"], got["theta"]])
    assert f_got == pytest.approx(f_want, rel=1e-6)
    assert np.allclose(got["beta"], want["beta"], atol=2e-3)
    assert np.allclose(got["theta"], want["theta"], atol=5e-3)
    assert np.allclose(np.asarray(got["u"]).ravel(), want["u"], atol=5e-3)


@pytest.fixture(scope="module")
def nr_oracle():
    out = {}

    def get(name):
        if name not in out:
            d = LA_CASES[name]
            out[name] = ola.mcml_la_nr(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"],
                                       d["start"], maxiter=6)
        return out[name]
    return get


def _args(d):
    return (d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"], d["start"])


@pytest.mark.parametrize("name", ["poisson", "binomial"])
def test_mcml_la_nr_matches_oracle_driver(name, nr_oracle, monkeypatch):
    monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    d = LA_CASES[name]
    n0 = api.la_component_launches()
    got = api.mcml_la_nr(*_args(d), verbose=False, maxiter=6, operator="component")
    assert api.la_component_launches() > n0 and api.get_default_la_operator() == "dense"
    assert got["u"].shape == (d["Q"], 1)
    _check_driver(d, got, nr_oracle(name))
    with api.Context(*_args(d)[:-1]) as ctx:
        same = ctx.mcml_la(d["start"], nr=True, maxiter=6, operator="component")
        p = ctx.la_plan()
        assert p["requested"] == "dense" and p["operator"] == "component" and p["launches"] > 0 and p["dense_bytes"] == 0, p
    for k in ("beta", "theta"):
        assert np.array_equal(got[k], same[k]), k
    assert np.array_equal(got["u"].ravel(), same["u"])


def test_mcml_la_matches_golden_driver(monkeypatch):
    """test_gpu_la.test_mcml_la_matches_golden_driver on the component operator (its tolerances)"""
    monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    with open(os.path.join(ROOT, "tests", "golden", "la_golden.json")) as f:
        g = json.load(f)["crt_poisson"]
    d = getattr(synth, g["gen"])(**g["kw"])
    want = g["la"]
    n0 = api.la_component_launches()
    got = api.mcml_la(*_args(d), verbose=False, maxiter=want["maxiter"], usehess=True, operator="component")
    assert api.la_component_launches() > n0
    m = _oracle(d); m.v = np.array(want["v"])
    f_want = m.la_btheta_objective(np.r_[want["beta"], want["theta"]])
    f_got = m.la_btheta_objective(np.r_[got["beta"], got["theta"]])
    assert f_got == pytest.approx(f_want, rel=1e-5)
    assert np.allclose(got["beta"], want["beta"], atol=1e-2)
    assert np.allclose(got["theta"], want["theta"], atol=1e-2)
    assert np.allclose(got["u"].ravel(), want["u"], atol=1e-2)
    nv = d["P"] + 2
    assert np.all(np.isfinite(got["se"])) and np.all(got["se"][:nv] > 0)
    assert np.allclose(got["se"][:nv], np.array(want["se"])[:nv], rtol=5e-2)


def test_one_shot_exports_under_the_process_default(nr_oracle, monkeypatch):
    """api.mcml_la_nr creates its context itself: under set_default_la_operator("component") it launches k_lac_factor
    (it does not under the default) and its fit equals Context.mcml_la(operator="component") bit for bit"""
    monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    d = LA_CASES["poisson"]
    n0 = api.la_component_launches()
    dense = api.mcml_la_nr(*_args(d), verbose=False, maxiter=6)
    assert api.la_component_launches() == n0
    try:
        api.set_default_la_operator("component")
        assert api.get_default_la_operator() == "component"
        got = api.mcml_la_nr(*_args(d), verbose=False, maxiter=6)
        with api.Context(*_args(d)[:-1]) as ctx:
            assert ctx.la_plan()["requested"] == "component"
    finally:
        api.set_default_la_operator("dense")
    assert api.la_component_launches() > n0
    _check_driver(d, got, nr_oracle("poisson"))
    with api.Context(*_args(d)[:-1]) as ctx:
        assert ctx.la_plan()["requested"] == "dense"
        same = ctx.mcml_la(d["start"], nr=True, maxiter=6, operator="component")
    assert np.array_equal(got["beta"], same["beta"]) and np.array_equal(got["theta"], same["theta"])
    assert np.abs(got["beta"] - dense["beta"]).max() < 2e-3 and np.abs(got["theta"] - dense["theta"]).max() < 5e-3


_ENV_SCRIPT = """
import json, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from glmmrmcml_amd import api
from test_gpu_la import CASES
d = CASES["poisson"]
args = (d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"])
default = api.get_default_la_operator()
n0 = api.la_component_launches()
r = api.mcml_la_nr(*args, d["start"], verbose=False, maxiter=6)
with api.Context(*args) as ctx:
    requested = ctx.la_plan()["requested"]
print("RESULT " + json.dumps(dict(default=default, requested=requested, launches=api.la_component_launches() - n0,
                                  beta=r["beta"].tolist(), theta=r["theta"].tolist())))
"""


def test_one_shot_export_under_the_environment_variable(monkeypatch):
    """GLMMR_MCML_LA=component is read once per process: a fresh interpreter"""
    monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    env = dict(os.environ, GLMMR_MCML_LA="component")
    out = subprocess.run([sys.executable, "-c", _ENV_SCRIPT % (ROOT, os.path.join(ROOT, "tests"))], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(next(l for l in out.stdout.splitlines() if l.startswith("RESULT "))[7:])
    assert r["default"] == "component" and r["requested"] == "component" and r["launches"] > 0, r
    d = LA_CASES["poisson"]
    with api.Context(*_args(d)[:-1]) as ctx:
        same = ctx.mcml_la(d["start"], nr=True, maxiter=6, operator="component")
    assert np.array_equal(np.array(r["beta"]), same["beta"]) and np.array_equal(np.array(r["theta"]), same["theta"])


def test_model_caller_passes_the_choice_and_restores_it(monkeypatch):
    """ModelMCML.LA(operator=...) sets the backend default for the duration of the call"""
    from glmmrmcml_amd.model import ModelMCML
    monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
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
    for op in ("component", None):
        fit[op] = mod.LA(d["y"], method="nr", operator=op)
    assert seen == [("component", True), ("dense", False)] and api.get_default_la_operator() == "dense"
    assert np.abs(fit["component"].theta - fit[None].theta).max() < 5e-3


# ---------------------------------------------------------------- 7) repeatability
@pytest.mark.parametrize("name", ["sw_long_ragged", "rct"])
def test_two_runs_are_bit_identical(name, monkeypatch):
    d, counts = la_design(name, "binomial", "logit")
    with component_context(d, monkeypatch) as ctx:
        a = _probes(ctx, d, np.random.default_rng(23))
        ra = ctx.mcml_la(d["start"], nr=True, maxiter=2, maxfun=40)
        b = _probes(ctx, d, np.random.default_rng(23))
        rb = ctx.mcml_la(d["start"], nr=True, maxiter=2, maxfun=40)
        assert_component(ctx, counts)
    assert np.array_equal(a[0], b[0])
    for k in ("v", "beta"):
        assert np.array_equal(a[1][k], b[1][k]), k
    assert a[1]["sigma"] == b[1]["sigma"]
    for k in ("beta", "theta", "u"):
        assert np.array_equal(ra[k], rb[k]), k


# ---------------------------------------------------------------- 8) the context stays usable
@pytest.mark.parametrize("traj", ["step", "component"])
def test_la_keeps_the_context_usable(traj, monkeypatch):
    """test_gpu_la.test_la_keeps_the_context_usable after a component call, in both trajectory modes: the sampler's
    draws equal those of a context that never ran a Laplace fit"""
    monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    d = LA_CASES["poisson"]
    out = {}
    for la in (False, True):
        with api.Context(*_args(d)[:-1]) as ctx:
            ctx.set_trajectory(traj)
            if la:
                r = ctx.mcml_la(d["start"], nr=True, maxiter=2, operator="component")
                assert np.all(np.isfinite(r["beta"])) and ctx.la_plan()["operator"] == "component"
            ctx.update_L(d["theta"])
            dg = ctx.hmc_sample(d["beta"], 1.0, 5, 8, 0.05, 10, 0.9, seed=3, chains=8)
            assert dg["accept_rate"] > 0
            assert ctx.last_kernels() == ((traj,) * 2 if traj == "component" else ("sparse",) * 2)
            out[la] = ctx.get_u()
    assert np.array_equal(out[False], out[True])
