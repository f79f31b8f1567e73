"""The bits of the samplers' per-chain rules and sample layout, pinned in every back end.  The oracle comparisons check
each back end on its own and within a tolerance on the draws; they cannot see a rule (csrc/hmc_chain.h: the reset of a
chain, its step count, the Metropolis decision, dual averaging, the column a draw lands in) that drifts by a last digit in
one back end.  Here the SHA-256 of what a call returns -- get_u(), the accept flags, the probabilities and the diagnostics --
is compared with tests/golden/sampler_bits.json, recorded from the library of the commit named there
(tests/golden/make_sampler_bits.py: never from the code under test).

Sampler settings are test_gpu_dense_products' (a short adaptive warm-up: step size and step count differ per chain).  The
cases are the smallest that reach each copy of the rules the back ends once carried:
  dense_*       column-major state (k_hmc_init / k_hmc_propose / k_hmc_accept<3>, <7> and the run-time instance, epilogues <3>,
                <7>, run-time and <12>): Q = 150, 20 chains (past the 16-column stream), 3 chains (the stream), one chain with
                and without warm-up (column 0 is then the start value)
  step_*        chain-major state, a launch pair per leapfrog step (k_cm_init / k_cm_propose_fin / k_cm_accept_fin<false>):
                130 chains (two groups of 64 and one of 2), one chain, and 5 chains x 2 draws for 7 samples (10 columns)
  component_*   component trajectories (k_cm_traj, k_cm_accept_fin<true>), both forms of the kernel
  exact_*       exact conditional draws, dense and component-wise (factor kernel a wave / a workgroup per component); on rct64
                (components of 65 variables) the draw kernel reads the factors unstaged, 9 columns and 70 (a second block of 64)
  nuts_*        NUTS on a dense and a sparse design (sampler_init_state, store_columns, the shape), nsamp not a multiple of chains
The input hashes are asserted first: a changed numpy stream fails there instead of comparing different problems."""
import hashlib
import json
import os

import numpy as np
import pytest

import nuts_cases as nc
import test_gpu_dense_products as dp
import test_gpu_sparse_products as sp
from test_gpu_la_component_wide import wide_design
from test_gpu_dense_products import ADAPT, IT, LAM, MS, SEED, TA, WARM

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_bits.json")
DIAG_KEYS = ("accept_rate", "mean_e", "min_e", "max_e", "max_steps_used", "leapfrog_total")
NUTS_DIAG_KEYS = ("mean_e", "min_e", "max_e", "divergent", "treedepth_hits")
ENV = ("GLMMR_MCML_TRAJ_WAVES", "GLMMR_MCML_LA_WAVES", "GLMMR_MCML_SKINNY", "GLMMR_MCML_GEMM", "GLMMR_MCML_DRAWS")


def sha256(*arrays):
    """of the arrays' values in column-major order, one after the other: uint8 as bytes, everything else as float64"""
    h = hashlib.sha256()
    for a in arrays:
        a = np.asarray(a)
        h.update(a.tobytes(order="F") if a.dtype == np.uint8 else a.astype(np.float64).tobytes(order="F"))
    return h.hexdigest()


def _inputs(d):
    return sha256(d["Z"], d["X"], d["y"], d["cov"], d["data"], d["eff_range"], d["beta"], d["theta"])


def _hmc(ctx, d, chains, nsamp, warm):
    vp = sp._vp(d)
    diag, flags, probs = ctx.hmc_sample(d["beta"], vp, warm, nsamp, LAM, MS, TA, SEED, chains=chains, iter_idx=IT,
                                        adapt=ADAPT, want_trace=True)
    u = ctx.get_u()
    per = nsamp if chains == 1 else -(-nsamp // chains)
    assert u.shape == (d["Q"], nsamp + 1 if chains == 1 else chains * per) and flags.shape == (chains, warm + per)
    return dict(u=sha256(u), flags=sha256(flags), probs=sha256(probs), diag=sha256([diag[k] for k in DIAG_KEYS]),
                kernels=",".join(map(str, ctx.last_kernels())))          # recorded as text: the same path as the reference build


def dense(family, link, chains, nsamp, warm=WARM, draws=None):
    def run(mp):
        d = dp.design(family, link, 150)
        with dp.context(d) as ctx:
            if draws:
                ctx.set_draws(draws)
                assert ctx.draws_plan()["applicable"]
            out = _hmc(ctx, d, chains, nsamp, warm)
            assert ctx.last_kernels() == ("exact", "exact") if draws else not {"sparse", "exact"} & set(ctx.last_kernels())
        return dict(out, inputs=_inputs(d))
    return run


def sparse(kind, opts, chains, nsamp, warm=WARM, trajectory="step", traj_waves=None, family="binomial", link="logit",
           draws=None, la_waves=None):
    def run(mp):
        if traj_waves:
            mp.setenv("GLMMR_MCML_TRAJ_WAVES", traj_waves)
        if la_waves:
            mp.setenv("GLMMR_MCML_LA_WAVES", la_waves)
        d = sp.design(kind, family, link, **opts)
        with sp.context(d, mp, None) as ctx:
            ctx.set_trajectory(trajectory)
            if draws:
                ctx.set_draws(draws)
                p = ctx.exact_component_plan()
                assert p["applicable"] and p["requested"] == draws and p["factor_waves"] == int(la_waves), p
            out = _hmc(ctx, d, chains, nsamp, warm)
            want = draws or {"step": "sparse", "component": "component"}[trajectory]
            assert ctx.last_kernels() == (want, want), ctx.last_kernels()
            if trajectory == "component" and traj_waves:
                assert ctx.component_plan(chains)["waves_per_item"] == int(traj_waves)
        return dict(out, inputs=_inputs(d))
    return run


def exact_rct64(chains, nsamp):
    """cluster_rct(2, 64, 2), gaussian / identity: 2 components of 65 variables, above the staged draw kernel's cap"""
    def run(mp):
        d = wide_design("rct64", "gaussian", "identity")[0]
        with sp.context(d, mp, None) as ctx:
            ctx.set_draws("exact_component")
            p = ctx.exact_component_plan()
            assert p["applicable"] and (p["ncomp"], p["max_vars"], p["max_rows"]) == (2, 65, 128), p
            assert p["factor_waves"] == 4 and p["draw_lds_bytes"] == 8 * 64 * 65 and p["factor_bytes"] == 8 * 2 * 65 * 65, p
            out = _hmc(ctx, d, chains, nsamp, WARM)
            assert ctx.last_kernels() == ("exact_component",) * 2, ctx.last_kernels()
        return dict(out, inputs=_inputs(d))
    return run


def nuts(name):
    def run(mp):
        c = nc.CASES[name]
        C = min(v["C"] for v in nc.CASES.values() if v["cm"] == c["cm"])      # the smallest chain count of its operator
        assert C == c["C"]
        d = nc.design(name)
        from glmmrmcml_amd import api
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
            ctx.update_L(d["theta"])
            diag, tr = ctx.nuts_sample(d["beta"], c["vp"], c["warm"], 2 * C - 3, c.get("seed", nc.SEED), chains=C,
                                       iter_idx=nc.ITER_IDX, max_treedepth=nc.MAX_DEPTH, adapt_delta=c["adapt_delta"],
                                       want_trace=True, metric=c["metric"])
            u = ctx.get_u()
            assert ("sparse" in ctx.last_kernels()) == c["cm"], ctx.last_kernels()
        assert u.shape == (d["Q"], 2 * C)                 # ceil((2 C - 3) / C) = 2 draws per chain
        return dict(inputs=_inputs(d), u=sha256(u), depth=sha256(tr["depth"]), nleap=sha256(tr["nleap"]), eps=sha256(tr["eps"]),
                    accept=sha256(tr["accept"]), diag=sha256([diag[k] for k in NUTS_DIAG_KEYS]))
    return run


SW_SHORT = ("sw_short", dict(drop=sp.DROP["sw_short"]))
SW_LONG = ("sw_long", dict(ragged=sp.RAGGED))
GAUSS = dict(family="gaussian", link="identity")

CASES = {
    "dense_20_binomial_logit": dense("binomial", "logit", 20, 20),
    "dense_20_gaussian_identity": dense("gaussian", "identity", 20, 20),
    "dense_20_gamma_log": dense("gamma", "log", 20, 20),
    "dense_20_beta_logit": dense("beta", "logit", 20, 20),
    "dense_3_binomial_logit": dense("binomial", "logit", 3, 3),
    "dense_1x3_warm6": dense("binomial", "logit", 1, 3),
    "dense_1x3_warm0": dense("binomial", "logit", 1, 3, warm=0),
    "step_130": sparse(*SW_SHORT, 130, 130),
    "step_1x3_warm6": sparse(*SW_SHORT, 1, 3),
    "step_1x3_warm0": sparse(*SW_SHORT, 1, 3, warm=0),
    "step_5_chains_7_samples": sparse(*SW_SHORT, 5, 7),
    "component_sw_long_130_waves1": sparse(*SW_LONG, 130, 130, trajectory="component", traj_waves="1"),
    "component_sw_long_130_waves4": sparse(*SW_LONG, 130, 130, trajectory="component", traj_waves="4"),
    "component_rct_130": sparse("rct", {}, 130, 130, trajectory="component"),
    "exact_dense_1x4": dense("gaussian", "identity", 1, 4, draws="exact"),
    "exact_dense_3_chains_7_samples": dense("gaussian", "identity", 3, 7, draws="exact"),
    "exact_component_waves1_1x4": sparse(*SW_LONG, 1, 4, draws="exact_component", la_waves="1", **GAUSS),
    "exact_component_waves1_3_chains_7_samples": sparse(*SW_LONG, 3, 7, draws="exact_component", la_waves="1", **GAUSS),
    "exact_component_waves4_1x4": sparse(*SW_LONG, 1, 4, draws="exact_component", la_waves="4", **GAUSS),
    "exact_component_waves4_3_chains_7_samples": sparse(*SW_LONG, 3, 7, draws="exact_component", la_waves="4", **GAUSS),
    "exact_component_rct64_3_chains_7_samples": exact_rct64(3, 7),
    "exact_component_rct64_1x69": exact_rct64(1, 69),
    "nuts_dense_96x40": nuts("dense_96x40"),
    "nuts_sparse_repack_128": nuts("repack"),
}


def digests(name, mp):
    """{"inputs": .., "u": .., ...} of a case through the library that is loaded; mp: a pytest.MonkeyPatch"""
    for k in ENV:
        mp.delenv(k, raising=False)
    return CASES[name](mp)


@pytest.mark.parametrize("name", list(CASES))
def test_sampler_bits_are_the_recorded_ones(name, monkeypatch):
    with open(FIXTURE) as f:
        want = json.load(f)["cases"][name]
    got = digests(name, monkeypatch)
    assert got["inputs"] == want["inputs"], "the seeded design is not the recorded one (numpy stream changed?)"
    for key in sorted(want):
        print(name, key, got[key])
    for key in sorted(want):
        assert got[key] == want[key], "%s: %s differs from the bits recorded in %s" % (name, key, FIXTURE)
    assert set(got) == set(want)
