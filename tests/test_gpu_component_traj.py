"""Component-local HMC trajectories (csrc/hmc_traj.h, csrc/component_plan.h; Context.set_trajectory("component")): one
launch per proposal runs the whole leapfrog trajectory of every (connected component of ZL's coupling graph, chain).

Checked against the CPU oracle chain by chain on the designs of test_gpu_sparse_products (tolerances of that file and of
test_gpu_dense_products: identical accept flags -- the oracle's |u - prob| >= 1e-6 margin asserted --, probabilities within
1e-9, samples within 1e-8 relative), in both forms of the kernel (one wave / four waves per work item), against the
per-step path in the same process at the full size of configs 1, 4 and 5, in the single-chain layout, with injected
starts and momenta, as a shard of a larger run, for reproducibility, for the fallbacks (nothing requested; a component
above the cap; a dense operator; the No-U-Turn sampler), in whole fits and through the one-shot export.  Every positive
case asserts last_kernels() == ("component", "component"), component_plan()["used"] and the plan's counts."""
import numpy as np
import pytest

from glmmrmcml_amd import api, synth
from test_gpu_dense_products import ADAPT, CASES, CHAIN_CASES, IT, LAM, MS, SEED, TA, WARM, run_chains
from test_gpu_sparse_products import DROP, GROUP_EDGES, RAGGED, _vp, check_chains, context, design

pytestmark = pytest.mark.gpu

CAP = 32                                    # CP_MAX_VARS (csrc/component_plan.h)
WAVES4_ROWS = 128                           # CP_WAVES4_ROWS: the four-wave form from this many observations in a component

# name -> (kind, design options, components, most variables, most observations, components without an observation)
DESIGNS = {
    "rct": ("rct", {}, 7, 6, 15, 0),
    "sw_short_drop": ("sw_short", dict(drop=DROP["sw_short"]), 7, 5, 15, 1),
    "sw_long_ragged": ("sw_long", dict(ragged=RAGGED), 7, 5, 200, 0),
    "sw_blk8": ("sw_blk8", {}, 5, 8, 24, 0),
    "sw_blk12": ("sw_blk12", {}, 5, 12, 24, 0),
    "sw_blk16": ("sw_blk16", {}, 5, 16, 32, 0),
    "tiny": ("tiny", {}, 3, 3, 6, 0),
    "long_wide": ("long_wide", {}, 410, 10, 9, 0),
    "sw_short_slope": ("sw_short", dict(slope=True), 6, 5, 15, 0),
}


def component_context(d, monkeypatch, waves=None, mode="component"):
    """a context on the heuristic's form of the sparse operator with the trajectory mode set; waves: "1" / "4" forces
    that form of the kernel (GLMMR_MCML_TRAJ_WAVES, read per call)"""
    if waves is None:
        monkeypatch.delenv("GLMMR_MCML_TRAJ_WAVES", raising=False)
    else:
        monkeypatch.setenv("GLMMR_MCML_TRAJ_WAVES", waves)
    ctx = context(d, monkeypatch, None)
    if mode is not None:
        ctx.set_trajectory(mode)
    return ctx


def assert_component(ctx, C, ncomp, max_vars, max_rows, empty, waves=None):
    assert ctx.last_kernels() == ("component", "component"), ctx.last_kernels()
    p = ctx.component_plan(C)
    assert p["requested"] and p["feasible"] and p["used"], p
    assert (p["ncomp"], p["max_vars"], p["max_rows"], p["empty_comps"]) == (ncomp, max_vars, max_rows, empty), p
    assert p["cap_vars"] == CAP and 1 <= p["nitems"] <= ncomp, p
    want = waves if waves is not None else (4 if max_rows >= WAVES4_ROWS else 1)
    assert p["waves_per_item"] == want, p
    assert p["lds_bytes_per_workgroup"] == (max_vars * 512 * 6 + 8192 if want == 4 else max_vars * 512 * 3), p
    return p


# ---------------------------------------------------------------- 1) chains against the oracle, one by one
@pytest.mark.parametrize("name", list(DESIGNS))
@pytest.mark.parametrize("family,link,vp", CHAIN_CASES)
def test_chains_against_the_oracle(orc, family, link, vp, name, monkeypatch):
    """130 chains after a short adaptive warm-up (step size and step count differ per chain: lanes of one wave finish at
    different steps); the group edges 0, 63, 64, 127, 128, 129 against the oracle.  sw_long with RAGGED is the design the
    rule gives the four-wave form (200 observations in a component); the others take one wave per work item."""
    kind, opts, ncomp, max_vars, max_rows, empty = DESIGNS[name]
    d = design(kind, family, link, **opts)
    L = None
    if kind == "long_wide":               # L is diagonal: sqrt(D) instead of a dense Cholesky of 4100 x 4100
        D = orc.gen_D(d["cov"], d["data"], d["eff_range"], d["theta"], chol=False)
        assert np.count_nonzero(D) == d["Q"]
        L = np.sqrt(D)
    with component_context(d, monkeypatch) as ctx:
        u, flags, probs = run_chains(ctx, d, 130)
        p = assert_component(ctx, 130, ncomp, max_vars, max_rows, empty)
        assert p["waves_per_item"] == (4 if name == "sw_long_ragged" else 1)
    assert u.shape == (d["Q"], 130)
    check_chains(orc, d, u, flags, probs, GROUP_EDGES, L=L)


# ---------------------------------------------------------------- 2) both forms of the kernel, whatever the rule says
@pytest.mark.parametrize("name,waves", [("sw_long_ragged", "1"), ("sw_long_ragged", "4"), ("rct", "4"), ("rct", "1"),
                                        ("sw_short_drop", "4"), ("sw_blk16", "4")])
def test_both_kernel_forms(orc, name, waves, monkeypatch):
    """WAVES = 1 on the long-row design and WAVES = 4 on designs whose components have fewer observations than waves'
    quarters can all be non-empty for (15 observations; an isolated variable: four empty quarters), forced through
    GLMMR_MCML_TRAJ_WAVES; binomial-logit and gaussian-identity (post = 1 / vp^2)"""
    kind, opts, ncomp, max_vars, max_rows, empty = DESIGNS[name]
    for family, link, vp in (CASES[2], CASES[6]):
        d = design(kind, family, link, **opts)
        with component_context(d, monkeypatch, waves) as ctx:
            u, flags, probs = run_chains(ctx, d, 130)
            assert_component(ctx, 130, ncomp, max_vars, max_rows, empty, waves=int(waves))
        check_chains(orc, d, u, flags, probs, GROUP_EDGES)


def test_forms_agree_with_each_other(monkeypatch):
    """the two forms are the same sampler (the four-wave form adds the waves' sums in wave order): identical flags,
    probabilities within 1e-9, draws within 1e-8"""
    d = design("sw_long", "poisson", "log", ragged=RAGGED)
    out = {}
    for waves in ("1", "4"):
        with component_context(d, monkeypatch, waves) as ctx:
            out[waves] = run_chains(ctx, d, 130)
            assert_component(ctx, 130, 7, 5, 200, 0, waves=int(waves))
    assert np.array_equal(out["1"][1], out["4"][1])
    assert np.abs(out["1"][2] - out["4"][2]).max() < 1e-9
    assert np.abs(out["1"][0] - out["4"][0]).max() < 1e-8 * max(1.0, np.abs(out["1"][0]).max())


# ---------------------------------------------------------------- 3) against the per-step path at full size
def eps_trace(probs, warm, adapt, ta):
    """the step size every chain ran proposal `it` with, from the acceptance probabilities (mhmcmc.h:107-116 as
    k_cm_accept_fin evaluates it): (chains, proposals)"""
    C, total = probs.shape
    e = np.full(C, 0.001); ebar = np.ones(C); H = np.zeros(C)
    out = np.zeros((C, total))
    for it in range(total):
        out[:, it] = e
        if it < warm and it < adapt:
            k = it + 1
            f1 = 1.0 / (k + 10)
            H = (1 - f1) * H + f1 * (ta - probs[:, it])
            loge = -4.60517 - np.sqrt(k / 0.05) * H
            powm = k ** -0.75
            ebar = np.exp(powm * loge + (1 - powm) * np.log(ebar))
            e = np.exp(loge)
        else:
            e = ebar.copy()
    return out


FULL = {  # config -> (design, chains, warm-up, lambda, max_steps, seed, plan counts) as in test_gpu_configs_fullsize
    "config1": (lambda: synth.cluster_rct(10, 5, 10), 100, 30, 0.3, 10, 5, (10, 6, 50, 0)),
    "config4": (lambda: synth.stepped_wedge(40, 8, 50), 512, 40, 0.5, 10, 31, (40, 8, 400, 0)),
    "config5": (lambda: synth.longitudinal(2000, 10), 1024, 30, 0.5, 10, 31, (2000, 11, 10, 0)),
}


@pytest.mark.parametrize("config", list(FULL))
def test_against_the_per_step_path_at_full_size(config, monkeypatch):
    make, C, warm, lam, ms, seed, counts = FULL[config]
    d = make()
    monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    monkeypatch.delenv("GLMMR_MCML_TRAJ_WAVES", raising=False)
    out = {}
    with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
        ctx.update_L(d["theta"])
        for mode in ("step", "component"):
            ctx.set_trajectory(mode)
            diag, flags, probs = ctx.hmc_sample(d["beta"], 1.0, warm, C, lam, ms, 0.9, seed, chains=C, want_trace=True)
            if mode == "component":
                p = assert_component(ctx, C, *counts)
                assert p["waves_per_item"] == (4 if config == "config4" else 1)
            else:
                assert ctx.last_kernels() == ("sparse", "sparse") and not ctx.component_plan(C)["used"]
            out[mode] = (ctx.get_u(), flags.copy(), probs.copy(), diag)
    (us, fs, ps, ds), (uc, fc, pc, dc) = out["step"], out["component"]
    assert np.array_equal(fs, fc)
    assert np.abs(ps - pc).max() < 1e-9
    assert np.abs(us - uc).max() < 1e-8 * max(1.0, np.abs(us).max())
    assert ds["leapfrog_total"] == dc["leapfrog_total"] and ds["max_steps_used"] == dc["max_steps_used"]
    # the warm-up is long enough that chains of one wave take different numbers of steps in one proposal
    steps = np.clip(np.round(lam / eps_trace(pc, warm, 100, 0.9)), 1, ms).astype(int)
    # eps_trace restates the device's dual averaging: held to what the device ran through its own counters
    assert int(steps.sum()) == dc["leapfrog_total"] and int(steps[:, -1].max()) == dc["max_steps_used"]
    assert any(len(set(steps[g:g + 64, it])) > 1 for g in range(0, C, 64) for it in range(steps.shape[1])), steps[:64]


# ---------------------------------------------------------------- 4) other layouts and inputs
@pytest.mark.parametrize("warm", [WARM, 0])
def test_single_chain_reference_layout(orc, warm, monkeypatch):
    """chains = 1: the reference's Q x (nsamp + 1), also without a warm-up (column 0 is the start)"""
    d = design("sw_short", "binomial", "probit", drop=DROP["sw_short"])
    nsamp = 3
    with component_context(d, monkeypatch) as ctx:
        diag, flags, probs = ctx.hmc_sample(d["beta"], _vp(d), warm, nsamp, LAM, MS, TA, SEED, chains=1, iter_idx=IT,
                                            adapt=ADAPT, want_trace=True)
        u = ctx.get_u()
        assert_component(ctx, 1, 7, 5, 15, 1)
        ctx.set_trajectory("step")
        diag2, flags2, probs2 = ctx.hmc_sample(d["beta"], _vp(d), warm, nsamp, LAM, MS, TA, SEED, chains=1, iter_idx=IT,
                                               adapt=ADAPT, want_trace=True)
        u2 = ctx.get_u()
        assert ctx.last_kernels() == ("sparse", "sparse")
    assert u.shape == (d["Q"], nsamp + 1) and flags.shape == (1, warm + nsamp)
    assert np.array_equal(flags, flags2) and np.abs(probs - probs2).max() < 1e-9
    assert np.abs(u - u2).max() < 1e-8 * max(1.0, np.abs(u2).max())
    if warm == WARM:
        check_chains(orc, d, u, flags, probs, [0], nsamp=nsamp)


def test_injected_start_and_momenta(monkeypatch):
    """inj_init / inj_mom replace the generator's draws: the two paths read the same numbers"""
    d = design("rct", "poisson", "log")
    C, total = 70, WARM + 1
    rng = np.random.default_rng(12)
    init = np.asfortranarray(0.2 * rng.normal(size=(d["Q"], C)))
    mom = np.asfortranarray(rng.normal(size=(d["Q"], C * total)))
    out = {}
    with component_context(d, monkeypatch) as ctx:
        for mode in ("step", "component"):
            ctx.set_trajectory(mode)
            diag, flags, probs = ctx.hmc_sample(d["beta"], _vp(d), WARM, C, LAM, MS, TA, SEED, chains=C, iter_idx=IT,
                                                adapt=ADAPT, inj_init=init, inj_mom=mom, want_trace=True)
            out[mode] = (ctx.get_u(), flags.copy(), probs.copy())
        assert_component(ctx, C, 7, 6, 15, 0)
        ctx.set_trajectory("component")
        diag, flags, probs = ctx.hmc_sample(d["beta"], _vp(d), WARM, C, LAM, MS, TA, SEED, chains=C, iter_idx=IT,
                                            adapt=ADAPT, want_trace=True)
        free = ctx.get_u()
    assert np.array_equal(out["step"][1], out["component"][1])
    assert np.abs(out["step"][2] - out["component"][2]).max() < 1e-9
    assert np.abs(out["step"][0] - out["component"][0]).max() < 1e-8 * max(1.0, np.abs(out["step"][0]).max())
    assert np.abs(free - out["component"][0]).max() > 1e-3           # the injected numbers were used


def test_a_shard_equals_the_same_global_chains(monkeypatch):
    """chain_offset != 0: chains 40 .. 109 run alone equal chains 40 .. 109 of a run of 130"""
    d = design("sw_blk8", "gaussian", "identity")
    with component_context(d, monkeypatch) as ctx:
        u, flags, probs = run_chains(ctx, d, 130)
        diag, f2, p2 = ctx.hmc_sample(d["beta"], _vp(d), WARM, 70, LAM, MS, TA, SEED, chains=70, chain_offset=40,
                                      iter_idx=IT, adapt=ADAPT, want_trace=True)
        u2 = ctx.get_u()
        assert_component(ctx, 70, 5, 8, 24, 0)
    assert np.array_equal(u[:, 40:110], u2) and np.array_equal(flags[40:110], f2) and np.array_equal(probs[40:110], p2)


# ---------------------------------------------------------------- 5) reproducibility
@pytest.mark.parametrize("name", ["sw_long_ragged", "rct"])
def test_two_runs_are_bit_identical(name, monkeypatch):
    kind, opts, ncomp, max_vars, max_rows, empty = DESIGNS[name]
    d = design(kind, "binomial", "logit", **opts)
    with component_context(d, monkeypatch) as ctx:
        a = run_chains(ctx, d, 130)
        b = run_chains(ctx, d, 130)
        assert_component(ctx, 130, ncomp, max_vars, max_rows, empty)
    for k in range(3):
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------- 6) unchanged and fallback behaviour
def test_nothing_set_is_the_per_step_path(monkeypatch):
    monkeypatch.delenv("GLMMR_MCML_TRAJ", raising=False)
    d = design("rct", "binomial", "logit")
    with component_context(d, monkeypatch, mode=None) as ctx:
        p = ctx.component_plan(130)
        assert not p["requested"] and p["feasible"] and not p["used"], p
        a = run_chains(ctx, d, 130)
        assert ctx.last_kernels() == ("sparse", "sparse")
        ctx.set_trajectory("component")
        run_chains(ctx, d, 130)
        assert ctx.last_kernels() == ("component", "component")
        ctx.set_trajectory("step")
        b = run_chains(ctx, d, 130)
        assert ctx.last_kernels() == ("sparse", "sparse")
    for k in range(3):
        assert np.array_equal(a[k], b[k]), k


def _blk48():
    s = synth.stepped_wedge(3, 48, 2)
    d = dict(s, beta=np.array([0.2]), X=np.ones((s["n"], 1), order="F"), theta=np.array((0.1, 0.8)))
    d["y"] = (np.random.default_rng(97).random(d["n"]) < 0.55).astype(float)
    return d


def _rct41():
    """cluster_rct(3, 40, 2): diagonal blocks, a row of ZL two wide -- the sparse operator is active -- and components of
    1 + 40 variables, above the cap"""
    s = synth.cluster_rct(3, 40, 2)
    return dict(s, beta=np.array([0.2]), X=np.ones((s["n"], 1), order="F"))


def test_fallbacks_run_the_old_kernels_bit_for_bit(monkeypatch):
    """"component" requested where it cannot be used: stepped_wedge(3, 48, 2) (components of 48 variables; its blocks are
    above SMALL_BLOCK, so the operator is a dense one), cluster_rct(3, 40, 2) (the sparse operator active, components of
    41 variables: above the cap), a geospatial model (dense operator) and the No-U-Turn sampler -- the old kernels run
    and the results equal the per-step results bit for bit"""
    monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    old = {"skinny", "band", "dlds", "reg", "sparse"}
    for d, C, kernels in ((_blk48(), 70, old), (_rct41(), 70, {"sparse"}), (synth.geospatial(192, seed=7), 40, old - {"sparse"})):
        out = {}
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
            ctx.update_L(d["theta"])
            for mode in ("step", "component"):
                ctx.set_trajectory(mode)
                diag, flags, probs = ctx.hmc_sample(d["beta"], d.get("sigma", 1.0), WARM, C, LAM, MS, TA, SEED, chains=C,
                                                    want_trace=True)
                assert set(ctx.last_kernels()) <= kernels, ctx.last_kernels()
                p = ctx.component_plan(C)
                assert p["requested"] == (mode == "component") and not p["feasible"] and not p["used"], p
                if ctx.sparse_plan(C)["active"]:
                    assert p["ncomp"] == 3 and p["max_vars"] in (41, 48) and p["max_vars"] > CAP, p
                else:
                    assert kernels != {"sparse"}
                out[mode] = (ctx.get_u(), flags.copy(), probs.copy())
        for k in range(3):
            assert np.array_equal(out["step"][k], out["component"][k]), k
    d = design("rct", "poisson", "log")
    out = {}
    with component_context(d, monkeypatch, mode=None) as ctx:
        for mode in ("step", "component"):
            ctx.set_trajectory(mode)
            ctx.nuts_sample(d["beta"], 1.0, 20, 8, seed=3, chains=8)
            assert ctx.last_kernels() == ("sparse", "sparse")
            out[mode] = ctx.get_u()
    assert np.array_equal(out["step"], out["component"])


# ---------------------------------------------------------------- 7) whole fits
@pytest.mark.parametrize("config", ["config1", "config4"])
def test_whole_fits_agree(config):
    """two mcml_full iterations at small size, component against step: beta and theta to 2e-6 (the tolerance of
    test_gpu_drivers.test_mcml_full_iteration_by_iteration)"""
    d = synth.cluster_rct(8, 3, 6, seed=3) if config == "config1" else synth.stepped_wedge(7, 4, 5, seed=11)
    fit = {}
    for mode in ("step", "component"):
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
            ctx.set_trajectory(mode)
            fit[mode] = ctx.mcml_full(d["start"], mcnr=True, m=24, maxiter=2, warmup=20, tol=1e-12, lambda_=0.3, maxsteps=8,
                                      target_accept=0.9, seed=4242, chains=24)
            assert ctx.last_kernels() == (("component",) * 2 if mode == "component" else ("sparse",) * 2)
            assert ctx.component_plan(24)["used"] == (mode == "component")
    a, b = fit["step"], fit["component"]
    assert a["iters"] == b["iters"] == 2
    assert np.abs(a["beta"] - b["beta"]).max() < 2e-6 * max(1.0, np.abs(a["beta"]).max())
    assert np.abs(a["theta"] - b["theta"]).max() < 2e-6


def test_model_caller_passes_the_choice_and_restores_it():
    """ModelMCML.MCML(trajectory=...) sets the backend default for the duration of the call"""
    from glmmrmcml_amd.model import ModelMCML
    assert api.get_default_trajectory() == "step"
    seen = []

    class Spy:
        def __getattr__(self, name):
            return getattr(api, name)

        def mcml_full(self, *a, **k):
            seen.append(api.get_default_trajectory())
            return api.mcml_full(*a, **k)

    d = synth.cluster_rct(ncl=8, nt=3, nind=8, seed=5, family="poisson")
    mod = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["family"], d["link"], d["beta"], d["theta"],
                    backend=Spy())
    mod.mcmc_options.update(warmup=20, samps=24, lambda_=0.3, maxsteps=8)
    fit = {}
    for traj in ("component", None):
        fit[traj] = mod.MCML(d["y"], se_method="none", verbose=False, max_iter=2, tol=1e-12, seed=4242, chains=24,
                             trajectory=traj)
    assert seen == ["component", "step"] and api.get_default_trajectory() == "step"
    assert np.abs(fit["component"]["theta"] - fit[None]["theta"]).max() < 2e-6 * max(1.0, np.abs(fit[None]["theta"]).max())


# ---------------------------------------------------------------- 8) one-shot exports
def test_one_shot_export_under_the_process_default(monkeypatch):
    """api.mcmc_sample creates its context itself: under set_default_trajectory("component") it inherits the mode, and its
    u equals Context.hmc_sample's on a context given the same L (a caller's L keeps the dense operator: the old kernels)"""
    d = design("rct", "poisson", "log")
    with context(d, monkeypatch, None) as ctx:
        L = ctx.gen_D(d["theta"], chol=True)
    try:
        api.set_default_trajectory("component")
        assert api.get_default_trajectory() == "component"
        got = api.mcmc_sample(d["Z"], L, d["X"], d["y"], d["beta"], d["family"], d["link"], WARM, 40, LAM, var_par=1.0,
                              maxsteps=MS, target_accept=TA, seed=SEED, chains=40)
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
            assert ctx.component_plan(40)["requested"]
            ctx.set_L(L)
            ctx.hmc_sample(d["beta"], 1.0, WARM, 40, LAM, MS, TA, SEED, chains=40)
            want = ctx.get_u()
            ctx.update_L(d["theta"])
            ctx.hmc_sample(d["beta"], 1.0, WARM, 40, LAM, MS, TA, SEED, chains=40)
            assert ctx.last_kernels() == ("component", "component")
            comp = ctx.get_u()
    finally:
        api.set_default_trajectory("step")
    assert np.array_equal(got, want)                 # fallback against fallback: both ran the dense operator on the caller's L
    assert np.abs(got - comp).max() < 1e-8 * max(1.0, np.abs(comp).max())


def test_one_shot_fit_runs_the_component_kernel():
    """api.mcml_full creates its context itself (from cov: the sparse operator): under the process default "component" that
    context launches k_cm_traj (the process-wide launch count moves; it does not under "step") and its fit equals
    Context.mcml_full after set_trajectory("component") bit for bit"""
    d = synth.stepped_wedge(7, 4, 5, seed=11)
    args = (d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"])
    kw = dict(mcnr=True, m=24, maxiter=2, warmup=20, tol=1e-12, verbose=False, lambda_=0.3, maxsteps=8, target_accept=0.9,
              seed=4242, chains=24)
    n0 = api.traj_launches()
    api.mcml_full(*args, d["start"], **kw)
    assert api.traj_launches() == n0                                  # default "step": not one launch
    try:
        api.set_default_trajectory("component")
        got = api.mcml_full(*args, d["start"], **kw)
    finally:
        api.set_default_trajectory("step")
    assert api.traj_launches() >= n0 + 2 * (20 + 1)                   # a launch per proposal: two iterations of warm-up + draw
    with api.Context(*args) as ctx:
        ctx.set_trajectory("component")
        want = ctx.mcml_full(d["start"], **{k: v for k, v in kw.items() if k != "verbose"})
        assert ctx.last_kernels() == ("component", "component")
        u = ctx.get_u()
    assert np.array_equal(got["beta"], want["beta"]) and np.array_equal(got["theta"], want["theta"])
    assert np.array_equal(got["u"], u)


def test_an_observation_without_entries(monkeypatch):
    """a row of Z that is all zero couples nothing but still adds log f(y | xb) to the density: the plan hands it to
    component 0, and the two paths agree"""
    d = design("rct", "poisson", "log")
    Z = d["Z"].copy(); Z[4] = 0.0
    d = dict(d, Z=np.asfortranarray(Z))
    out = {}
    with component_context(d, monkeypatch) as ctx:
        for mode in ("step", "component"):
            ctx.set_trajectory(mode)
            out[mode] = run_chains(ctx, d, 70)
        assert_component(ctx, 70, 7, 6, 15, 0)
    assert np.array_equal(out["step"][1], out["component"][1])
    assert np.abs(out["step"][2] - out["component"][2]).max() < 1e-9
    assert np.abs(out["step"][0] - out["component"][0]).max() < 1e-8 * max(1.0, np.abs(out["step"][0]).max())
