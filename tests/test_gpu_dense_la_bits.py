"""The bits of the dense linear-algebra layer, pinned where its code was moved and its duplicates merged: the blocked
Cholesky stack (csrc/chol.hip), the vector-sized kernels several modules share (csrc/vecops.hip) and the small host solves
(csrc/host_linalg.h).  The element-by-element and oracle tests judge each result within a bound; they cannot see a last
digit that moves when a kernel is replaced by its twin, a sum is regrouped or a launch changes its grid.  Here the SHA-256
of what a call returns is compared with tests/golden/dense_la_bits.json, recorded from the library of the commit named there
(tests/golden/make_dense_la_bits.py: never from the code under test).

  chol_*          glmmr_mcml_dbg_chol: the array as returned, the three solves, the inverted diagonal blocks -- one ragged
                  leaf (47), one panel plus a row on a single stream (129), three panels with the look-ahead (300)
  mvn_ll_graph    one dense block of 300, four calls on one context: eager, eager, capture, replay; the workspace after
  mvn_batch_*     mvn_ll_batch, 2 and 8 candidates at d = 300, 8 at d = 1153 (the first size with a super-panel regrouping)
  mixed_layout    diagonal rows, blocks up to 32 and one block above: mvn_ll (the accumulating sum) and gen_D(chol=True)
  la_dense_*      Laplace fits on the dense operator: the four probes, both drivers, the Hessian's inverse
  la_component_*  the probes on the component operators, a wave and a workgroup per component: rows of ZL two wide (rct), rows of
                  8 = two records per observation (sw_blk8), 65 variables = a lane's second entry of a row (rct64), and a
                  component of 48 variables over two covariance blocks, 12 records per observation (paired_ar1)
  beta_step       Context.mcnr: the Gauss-Jordan inverse at tolerance 0
  bobyqa          mcml_optim: the same elimination at 1e-14 inside the optimiser
The input hashes are asserted first: a changed numpy stream fails there instead of comparing different problems."""
import hashlib
import json
import os

import numpy as np
import pytest

import chol_reference as cr
import cov_layouts as cl
import family_designs as fd
import test_gpu_la_component as lc
import test_gpu_la_component_wide as lw
from test_gpu_la import CASES as LA_CASES
from test_gpu_sparse_products import context as sparse_context, design as sparse_design

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_la_bits.json")
ENV = ("GLMMR_MCML_LA_WAVES", "GLMMR_MCML_CHOL_GRAPH", "GLMMR_MCML_GEMM", "GLMMR_MCML_ZL")
WS_M = 5                 # sample columns of the mvn cases


def sha256(*arrays):
    """of the arrays' values as float64 in column-major order, one after the other"""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.asarray(a, dtype=np.float64).tobytes(order="F"))
    return h.hexdigest()


def _design_inputs(d):
    return sha256(d["Z"], d["X"], d["y"], d["cov"], d["data"], d["eff_range"], d["beta"], d["theta"], d.get("start", []))


def _model(d):
    from glmmrmcml_amd import api
    return api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"])


def _cov_context(blocks, u):
    from glmmrmcml_amd import api
    cov, data = cl.layout(blocks)
    ctx = api.Context(cov, data, np.zeros(cov.shape[0]))
    ctx.set_u(u)
    return ctx, sha256(cov, data, u)


# ---------------------------------------------------------------------------------------------- the Cholesky stack
def chol(n, m):
    def run(mp):
        A, B = cr.family_W(n), cr.rhs(n, m)
        ctx, _ = _cov_context([cr.block_S(40)], cr.samples(40, 1))
        with ctx:
            got = ctx.dbg_chol(A, B)
        return dict(inputs=sha256(A, B), **{k: sha256(got[k]) for k in ("A", "fwd", "trans", "potrs", "linv")})
    return run


def mvn_ll_graph(mp):
    d = 300
    block, theta, u = cr.block_S(d), cr.thetas_S(1)[0], cr.samples(d, WS_M)
    ctx, inputs = _cov_context([block], u)
    with ctx:
        values = [ctx.mvn_ll(theta) for call in range(4)]          # eager, eager, capture, replay
        L, X, dims = ctx.mvn_workspace()
    assert dims[:3] == (d, 304, WS_M), dims
    return dict(inputs=inputs, theta=sha256(theta), values=sha256(values), workspace=sha256(L, X))


def mvn_batch(k, d):
    def run(mp):
        block, th, u = cr.block_S(d), cr.thetas_S(k), cr.samples(d, WS_M)
        ctx, inputs = _cov_context([block], u)
        with ctx:
            values = ctx.mvn_ll_batch(th)
            L, X, dims = ctx.mvn_workspace(1)
        assert dims[:3] == (d, (d + 15) // 16 * 16, WS_M), dims
        return dict(inputs=inputs, thetas=sha256(th), values=sha256(values), workspace=sha256(L, X))
    return run


def mixed_layout(mp):
    """MIXED's diagonal rows (blocks of 1 and the all-gr block of 3), its blocks of 5, 7 and 32, and of its large blocks the
    150 alone; they use the first seven parameters"""
    blocks = [cl.MIXED[i] for i in (0, 1, 2, 4, 6, 7, 8, 3)]
    theta = cl.MIXED_THETA[:7]
    u = cl.samples(blocks, 20, seed=41)
    ctx, inputs = _cov_context(blocks, u)
    with ctx:
        assert ctx.npar() == 7
        ll = ctx.mvn_ll(theta)
        L = ctx.gen_D(theta, chol=True)
    return dict(inputs=inputs, theta=sha256(theta), mvn_ll=sha256([ll]), gen_D_chol=sha256(L))


# ---------------------------------------------------------------------------------------------- Laplace fits
def _probes(ctx, d):
    """the four probes at the points test_gpu_la draws: three functor values, then v, beta, sigma of the Newton step"""
    v, beta, theta, vp = lc.functor_points(d, np.random.default_rng(11), 1)
    gauss = d["family"] == "gaussian"
    f = [ctx.la_probe(d["start"], 0, var_par=vp, par=np.r_[beta, v]),
         ctx.la_probe(d["start"], 1, v=v, var_par=vp, par=np.r_[theta, vp] if gauss else theta),
         ctx.la_probe(d["start"], 2, v=v, var_par=vp, par=np.r_[beta, theta, vp] if gauss else np.r_[beta, theta])]
    st = ctx.la_probe(d["start"], 3, v=np.random.default_rng(5).normal(size=d["Q"]) * 0.2, var_par=1.0)
    return dict(functors=sha256(f), newton=sha256(st["v"], st["beta"], [st["sigma"]]))


def _fit(r):
    return sha256(r["beta"], r["theta"], [r["sigma"]], r["se"], r["u"])


def la_dense(name, usehess=False):
    def run(mp):
        d = LA_CASES[name]
        with _model(d) as ctx:
            out = _probes(ctx, d)
            assert ctx.la_plan()["operator"] == "dense"
            out["la"] = _fit(ctx.mcml_la(d["start"], nr=False, maxiter=2, maxfun=60))
            out["la_nr"] = _fit(ctx.mcml_la(d["start"], nr=True, maxiter=2, maxfun=60))
            if usehess:
                r = ctx.mcml_la(d["start"], nr=True, maxiter=2, maxfun=60, usehess=True)
                assert np.all(r["se"][:d["P"] + 2] > 0)
                out["la_nr_hess"] = _fit(r)
        return dict(out, inputs=_design_inputs(d))
    return run


def la_component(mode, waves=None, design=("rct", "poisson", "log"), counts=(7, 6, 15), want_waves=None):
    """counts: components, most variables and most observations of a component; want_waves: the form without a forced one"""
    def run(mp):
        if waves:
            mp.setenv("GLMMR_MCML_LA_WAVES", waves)
        d = lw.wide_design(*design)[0] if design[0] in ("rct64", "paired_ar1") else lc.with_start(sparse_design(*design))
        with sparse_context(d, mp, None) as ctx:
            ctx.set_la_operator(mode)
            out = _probes(ctx, d)
            p = ctx.la_plan()
            assert p["operator"] == mode and p["waves"] == int(waves or want_waves or 1) and p["launches"] == 1, p
            assert (p["ncomp"], p["max_vars"], p["max_rows"]) == counts and p["dense_bytes"] == 0, p
        return dict(out, inputs=_design_inputs(d))
    return run


# ---------------------------------------------------------------------------------------------- host solves
def beta_step(mp):
    d = fd.design("poisson", "log")
    assert d["P"] == 4
    u = np.asfortranarray(np.random.default_rng(31).normal(size=(d["Q"], 20)) * 0.2)
    with _model(d) as ctx:
        ctx.set_u(u)
        r = ctx.mcnr(d["beta"], 1.0)
    return dict(inputs=_design_inputs(d), u=sha256(u),
                mcnr=sha256(r["beta"], [r["sigma"]], r["XtWX"], r["XtWr"]))


def bobyqa(mp):
    d = LA_CASES["poisson"]
    u = np.asfortranarray(np.random.default_rng(37).normal(size=(d["Q"], 12)) * 0.2)
    with _model(d) as ctx:
        ctx.set_u(u)
        r = ctx.mcml_optim(d["start"], maxfun=40)
    return dict(inputs=_design_inputs(d), u=sha256(u), optim=sha256(r["beta"], r["theta"], [r["sigma"]]))


CASES = {
    "chol_47_ragged_leaf": chol(47, 3),
    "chol_129_panel_plus_row": chol(129, 3),
    "chol_300_lookahead": chol(300, 5),
    "mvn_ll_graph_300": mvn_ll_graph,
    "mvn_batch_2x300": mvn_batch(2, 300),
    "mvn_batch_8x300": mvn_batch(8, 300),
    "mvn_batch_8x1153": mvn_batch(8, 1153),
    "mixed_layout": mixed_layout,
    "la_dense_poisson": la_dense("poisson", usehess=True),
    "la_dense_gaussian": la_dense("gaussian"),
    "la_component_rct": la_component("component"),
    "la_component_wide_rct_waves1": la_component("component_wide", "1"),
    "la_component_wide_rct_waves4": la_component("component_wide", "4"),
    "la_component_sw_blk8": la_component("component", design=("sw_blk8", "poisson", "log"), counts=(5, 8, 24)),
    "la_component_wide_sw_blk8_waves4": la_component("component_wide", "4", design=("sw_blk8", "poisson", "log"), counts=(5, 8, 24)),
    "la_component_wide_rct64": la_component("component_wide", design=("rct64", "poisson", "log"), counts=(2, 65, 128), want_waves=4),
    "la_component_wide_paired_ar1": la_component("component_wide", design=("paired_ar1", "binomial", "logit"), counts=(2, 48, 96),
                                                 want_waves=4),
    "beta_step": beta_step,
    "bobyqa": bobyqa,
}


def digests(name, mp):
    """{"inputs": .., ...} of a case through the library that is loaded; mp: a pytest.MonkeyPatch"""
    for k in ENV:
        mp.delenv(k, raising=False)
    return CASES[name](mp)


@pytest.mark.parametrize("name", list(CASES))
def test_dense_la_bits_are_the_recorded_ones(name, monkeypatch):
    with open(FIXTURE) as f:
        want = json.load(f)["cases"][name]
    got = digests(name, monkeypatch)
    assert got["inputs"] == want["inputs"], "the seeded inputs are not the recorded ones (numpy stream changed?)"
    for key in sorted(want):
        print(name, key, got[key])
    for key in sorted(want):
        assert got[key] == want[key], "%s: %s differs from the bits recorded in %s" % (name, key, FIXTURE)
    assert set(got) == set(want)
