"""Exact conditional draws for gaussian / identity models (csrc/hmc_exact.h, Context.set_draws("exact") /
Context.exact_sample) on the GPU.

1. parity with the float64 twin (tests/exact_gaussian_twin.py, itself pinned to extended precision at 1e-12 by
   test_exact_gaussian_cpu.py) at 1e-10 max|want| -- the bound the project holds its factor to (test_gen_D_and_chol) --
   at the shapes where the 128-wide panel logic of the factorisation and of the two triangular solves can go wrong and at
   column counts below, at and past one 128-column tile;
2. the mean the path uses is the stationary point of the density the existing device code samples (log_prob_grad);
3. the dispatch: hmc_sample under set_draws("exact"), where it is honoured and where it is ignored;
4. the RNG addressing;
5. the full driver and the caller's keyword."""
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_gaussian_twin as tw
from glmmrmcml_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20240601
EXACT_DIAG = dict(accept_rate=1.0, mean_e=0.0, min_e=0.0, max_e=0.0, max_steps_used=0, leapfrog_total=0)


def _ctx(d, theta=None):
    from glmmrmcml_amd import api
    ctx = api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"])
    ctx.update_L(d["theta"] if theta is None else theta)
    return ctx


def _gaussian_cluster_design():
    """gaussian / identity on a design whose covariance blocks are all of size 1: the context runs the sparse ZL operator"""
    d = synth.cluster_rct(ncl=6, nt=4, nind=5, seed=8)
    rng = np.random.default_rng(8)
    u = np.concatenate([0.25 * rng.standard_normal(6), 0.1 * rng.standard_normal(24)])
    d["y"] = d["X"] @ d["beta"] + d["Z"] @ u + 0.7 * rng.standard_normal(d["n"])
    d["family"], d["link"], d["sigma"] = "gaussian", "identity", 0.7
    return d


# ---------------------------------------------------------------- 1. parity with the twin
@pytest.mark.parametrize("name", list(tw.SHAPES))
def test_exact_draws_match_the_twin(orc, name):
    d = tw.SHAPES[name]()
    Q = d["Q"]
    L = orc.gen_D(d["cov"], d["data"], d["eff_range"], d["theta"], chol=True)
    with _ctx(d) as ctx:
        assert ctx.draws_plan()["applicable"] and ctx.draws_plan()["Q"] == Q
        for chains, nsamp in tw.COLUMNS:
            diag = ctx.exact_sample(d["beta"], d["sigma"], nsamp, SEED, chains=chains, chain_offset=3, iter_idx=2)
            got = ctx.get_u()
            z = tw.normals(orc, Q, SEED, chains, nsamp, chain_offset=3, iter_idx=2)
            want, _ = tw.twin(d["Z"], L, d["X"], d["y"], d["beta"], d["sigma"], z)
            assert got.shape == want.shape == (Q, tw.layout(chains, nsamp)[2])
            err = np.abs(got - want).max() / np.abs(want).max()
            print("%s, %d columns: |got - want| / |want| = %.2e" % (name, want.shape[1], err))
            assert err <= 1e-10
            assert ctx.last_kernels() == ("exact", "exact")
            assert diag == EXACT_DIAG


# ---------------------------------------------------------------- 2. same target as the HMC path
@pytest.mark.parametrize("name", ["one panel plus one row (129)", "three panels, sigma 0.2 (300)", "dense Z 330 x 200"])
def test_mean_is_the_stationary_point_of_the_sampled_density(orc, name):
    """inj_z = 0: every column is L mu*; the device's own log_grad (what the HMC path integrates) vanishes there"""
    d = tw.SHAPES[name]()
    Q = d["Q"]
    L = orc.gen_D(d["cov"], d["data"], d["eff_range"], d["theta"], chol=True)
    b = (d["Z"] @ L).T @ (d["y"] - d["X"] @ d["beta"]) / d["sigma"] ** 2
    with _ctx(d) as ctx:
        ctx.exact_sample(d["beta"], d["sigma"], 3, SEED, inj_z=np.zeros((Q, 4)))
        u = ctx.get_u()
        assert u.shape == (Q, 4) and np.abs(u - u[:, :1]).max() <= 1e-12 * np.abs(u).max()
        v = np.linalg.solve(L, u)
        _, G = ctx.log_prob_grad(d["beta"], d["sigma"], v)
    print("%s: |grad| / |b| = %.2e" % (name, np.abs(G).max() / np.abs(b).max()))
    assert np.abs(G).max() <= 1e-10 * np.abs(b).max()


# ---------------------------------------------------------------- 3. dispatch
HMC_ARGS = dict(warmup=12, nsamp=40, lambda_=0.4, max_steps=6, target_accept=0.9)


def _hmc(ctx, d, seed=5, chains=20, iter_idx=1, sigma=None):
    return ctx.hmc_sample(d["beta"], d["sigma"] if sigma is None else sigma, HMC_ARGS["warmup"], HMC_ARGS["nsamp"],
                          HMC_ARGS["lambda_"], HMC_ARGS["max_steps"], HMC_ARGS["target_accept"], seed, chains=chains,
                          iter_idx=iter_idx, want_trace=True)


def test_hmc_sample_dispatches_to_the_exact_path_and_back():
    d = synth.geospatial(150)
    with _ctx(d) as plain:                               # a context that never heard of the switch
        diag0, flags0, probs0 = _hmc(plain, d)
        u0 = plain.get_u()
        assert "exact" not in plain.last_kernels() and plain.draws_plan()["requested"] == "hmc"
    with _ctx(d) as ctx:
        ctx.exact_sample(d["beta"], d["sigma"], 40, 5, chains=20, iter_idx=1)
        ue = ctx.get_u()
        ctx.set_draws("exact")
        assert ctx.draws_plan() == dict(requested="exact", applicable=True, Q=150, m_bytes=8 * 160 * 150)
        diag, flags, probs = _hmc(ctx, d)
        assert ctx.last_kernels() == ("exact", "exact")
        assert np.array_equal(ctx.get_u(), ue)
        assert flags.shape == (20, 12 + 2) and np.all(flags == 1) and np.all(probs == 1.0)
        assert diag == EXACT_DIAG
        assert not np.array_equal(ue, u0)
        ctx.set_draws("hmc")
        diag1, flags1, probs1 = _hmc(ctx, d)
        assert np.array_equal(ctx.get_u(), u0) and np.array_equal(flags1, flags0) and np.array_equal(probs1, probs0)
        assert diag1 == diag0 and "exact" not in ctx.last_kernels()


@pytest.mark.parametrize("which", ["binomial", "gaussian on the sparse operator"])
def test_request_is_ignored_where_the_path_does_not_apply(which):
    from glmmrmcml_amd import _lib
    d = synth.cluster_rct(ncl=6, nt=4, nind=5) if which == "binomial" else _gaussian_cluster_design()
    out = []
    for mode in ("hmc", "exact"):
        with _ctx(d) as ctx:
            ctx.set_draws(mode)
            if which != "binomial":
                assert ctx.sparse_plan(20)["active"]
            assert not ctx.draws_plan()["applicable"] and ctx.draws_plan()["requested"] == mode
            diag, flags, probs = _hmc(ctx, d)
            assert "exact" not in ctx.last_kernels()
            out.append((ctx.get_u(), flags, probs, diag))
            if mode == "exact":
                with pytest.raises(_lib.McmlError):
                    ctx.exact_sample(d["beta"], d["sigma"], 40, 5, chains=20)
                assert np.array_equal(ctx.get_u(), out[-1][0])          # the refused call left the samples alone
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][2], out[1][2]) and out[0][3] == out[1][3]


def test_environment_default_in_a_fresh_process():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from glmmrmcml_amd import api, synth\n"
            "d = synth.geospatial(40)\n"
            "print(api.get_default_draws())\n"
            "with api.Context(d['cov'], d['data'], d['eff_range'], d['Z'], d['X'], d['y'], d['family'], d['link']) as ctx:\n"
            "    ctx.update_L(d['theta'])\n"
            "    ctx.hmc_sample(d['beta'], d['sigma'], 5, 8, 0.4, 4, 0.9, 3, chains=8)\n"
            "    print(ctx.draws_plan()['requested'], *ctx.last_kernels())\n" % ROOT)
    for val, want in (("exact", ["exact", "exact exact exact"]), ("hmc", None)):
        r = subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, GLMMR_MCML_DRAWS=val),
                           capture_output=True, text=True, timeout=120)
        lines = r.stdout.strip().splitlines()[-2:]
        if want is not None:
            assert lines == want, r.stdout
        else:
            assert lines[0] == "hmc" and lines[1].startswith("hmc ") and "exact" not in lines[1], r.stdout


# ---------------------------------------------------------------- 4. RNG addressing
def test_rng_addressing():
    d = synth.geospatial(150)
    with _ctx(d) as ctx:
        ctx.exact_sample(d["beta"], d["sigma"], 40, 11, chains=40, iter_idx=1)
        a = ctx.get_u()
        ctx.exact_sample(d["beta"], d["sigma"], 40, 11, chains=40, iter_idx=1)
        assert np.array_equal(ctx.get_u(), a)                                    # the same seed reproduces bits
        ctx.exact_sample(d["beta"], d["sigma"], 40, 11, chains=40, iter_idx=2)
        b = ctx.get_u()
        assert a.shape == b.shape == (150, 40)
        assert all(not np.array_equal(a[:, j], b[:, j]) for j in range(40))      # another iteration: every column
        assert len({a[:, j].tobytes() for j in range(40)}) == 40                 # no two columns equal
        ctx.exact_sample(d["beta"], d["sigma"], 6, 11)                           # one chain: column 0 is a draw too
        one = ctx.get_u()
        assert one.shape == (150, 7) and len({one[:, j].tobytes() for j in range(7)}) == 7
    halves = []
    for off in (0, 20):
        with _ctx(d) as ctx:
            ctx.exact_sample(d["beta"], d["sigma"], 20, 11, chains=20, chain_offset=off, iter_idx=1)
            halves.append(ctx.get_u())
    assert np.abs(np.hstack(halves) - a).max() <= 1e-12 * np.abs(a).max()


# ---------------------------------------------------------------- 5. driver
def test_mcml_full_in_exact_mode_equals_the_hand_run_loop():
    d = synth.geospatial(150)
    start = d["start"]
    with _ctx(d) as ctx:
        ctx.set_draws("exact")
        got = ctx.mcml_full(start, mcnr=True, m=64, maxiter=2, chains=64, seed=7)
        gu = ctx.get_u()
        assert ctx.last_kernels() == ("exact", "exact")
    with _ctx(d) as ctx:
        ctx.set_draws("exact")
        beta, theta, sigma = start[:1].copy(), start[1:3].copy(), float(start[3])
        for it in (1, 2):
            ctx.update_L(theta)
            ctx.hmc_sample(beta, sigma, 500, 64, 0.05, 100, 0.9, seed=7, chains=64, iter_idx=it)
            u = ctx.get_u()
            r = ctx.mcml_optim(np.r_[beta, theta, sigma], mcnr=True)
            beta, theta, sigma = r["beta"], r["theta"], r["sigma"]

    def rel(a, b):
        return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())
    print("beta %.2e theta %.2e sigma %.2e u %.2e" % (rel(got["beta"], beta), rel(got["theta"], theta),
                                                      rel(got["sigma"], sigma), rel(gu, u)))
    assert got["iters"] == 2
    assert rel(got["beta"], beta) <= 1e-9 and rel(got["theta"], theta) <= 1e-9 and rel(got["sigma"], sigma) <= 1e-9
    assert rel(gu, u) <= 1e-9


def test_caller_keyword_sets_and_restores_the_process_default():
    from glmmrmcml_amd import api
    from glmmrmcml_amd.model import ModelMCML
    d = synth.geospatial(150)
    m = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["family"], d["link"], d["beta"], d["theta"],
                  var_par=d["sigma"])
    m.mcmc_options.update(warmup=20, samps=64, lambda_=0.5, maxsteps=8)
    assert api.get_default_draws() == "hmc"
    kw = dict(verbose=False, max_iter=2, seed=7, chains=64, se_method="none", options=dict(maxfun=40))
    fit = m.MCML(d["y"], draws="exact", **kw)
    assert api.get_default_draws() == "hmc"
    api.set_default_draws("exact")
    try:
        same = m.MCML(d["y"], **kw)                       # the default itself set to "exact": the same fit
        assert api.get_default_draws() == "exact"
        other = m.MCML(d["y"], draws="hmc", **kw)
        assert api.get_default_draws() == "exact"
    finally:
        api.set_default_draws("hmc")
    assert np.array_equal(fit["theta"], same["theta"]) and np.array_equal(fit["re_samps"], same["re_samps"])
    assert not np.array_equal(fit["re_samps"], other["re_samps"])
    with pytest.raises(KeyError):
        m.MCML(d["y"], draws="gibbs", **kw)
    assert api.get_default_draws() == "hmc"
