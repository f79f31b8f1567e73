"""A resident context through operator, structure and mode changes (context_sequences.py): every step of a sequence on
ONE context equals, bit for bit, the same call on a fresh context that was only given the logical state -- the last
successful update_L / set_L, the samples, the mode setters in force.  Every step asserts the kernels and plans it
means; at the named points a step is also held to the oracle (check_chains / check_log_prob_grad of
test_gpu_dense_products.py with their tolerances), so that two contexts wrong alike cannot pass.

S1  the zero structure of a dense L changes under the band plans (BandPlan::reset, the skinny plan)
S2  sparse <-> dense operator on one context, the sampler state re-interpreted chain-major / column-major
S3  HMC, NUTS, exact draws and mvn_ll share the state buffers and the two-entry Cholesky graph cache
S4  queries change nothing
S5  a call that fails changes nothing; a failed update_L leaves no L
S6  after the drivers"""
import os
import subprocess
import sys

import numpy as np
import pytest

from glmmrmcml_amd import api
from glmmrmcml_amd._lib import McmlError

import context_sequences as cs
import driver_cases as dc
import test_gpu_dense_products as dp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENOTPD = -3
DENSE = {"band", "dlds", "reg"}


@pytest.fixture(autouse=True)
def _default_paths(monkeypatch):
    for k in ("GLMMR_MCML_SKINNY", "GLMMR_MCML_GEMM", "GLMMR_MCML_ZL", "GLMMR_MCML_CHOL_GRAPH", "GLMMR_MCML_LA_WAVES"):
        monkeypatch.delenv(k, raising=False)


def _oracle_L(orc, d, theta=None):
    return orc.gen_D(d["cov"], d["data"], d["eff_range"], d["theta"] if theta is None else theta, chol=True)


def _assert_same(a, b, what):
    assert cs.same(a, b), "%s: differs in %s" % (what, cs.diff(a, b))


def _refuses(fn):
    with pytest.raises(McmlError, match=r"L (not )?set") as e:
        fn()
    return e


# ---------------------------------------------------------------------------------------------------------------- S1
def _s1_step(t, d, name, V, banded, nempty):
    r130 = t.sample(name + ": hmc 130", cs.hmc(d, 130))
    p = t.step(name + ": plans 130", cs.plans(130))
    for which in ("band_fwd", "band_bwd"):
        assert p[which]["used"] == banded and not p[which]["paired"] and p[which]["gn"] == 2, (name, which, p[which])
        assert p[which]["nempty"] == nempty, (name, which, p[which])
        assert not banded or p[which]["nred"] > 0, (name, which, p[which])          # streamed, bands split
    if banded:
        assert r130["kernels"] == ("band", "band"), (name, r130["kernels"])
        assert t.ctx.band_plan(130, "fwd")["built"] and t.ctx.band_plan(130, "bwd")["built"]
    else:
        assert set(r130["kernels"]) <= {"dlds", "reg"}, (name, r130["kernels"])
    r5 = t.sample(name + ": hmc 5", cs.hmc(d, 5))
    assert r5["kernels"] == ("skinny", "skinny"), (name, r5["kernels"])
    g = t.step(name + ": log_prob_grad 130", cs.log_prob_grad(d, V))
    assert (g["kernels"] == ("band", "band")) if banded else (set(g["kernels"]) <= {"dlds", "reg"}), (name, g["kernels"])
    return r130, r5, g


def test_s1_zero_structure_changes_under_the_plans(orc):
    d = cs.s1_design()
    F = cs.s1_factors(dp.oracle_L(orc, d))
    V = cs.lpg_input(d, 130)
    seen = {}
    with cs.Twin(d) as t:
        for visit, name in enumerate(("LA", "LB", "LC", "LD", "LA", "theta")):
            if name == "theta":
                t.update_L(d["theta"])
            else:
                t.set_L(F[name])
            got = _s1_step(t, d, "%d %s" % (visit, name), V, banded=name != "LC", nempty=1 if name == "LD" else 0)
            if name in seen:
                _assert_same(seen[name], got, "the second visit of " + name)
            seen[name] = got
            if name in ("LB", "LD"):
                r130 = got[0]
                dp.check_chains(orc, d, r130["u"], r130["flags"], r130["probs"], [0, 127, 129], L=F[name])
            if name == "LD":
                dp.check_log_prob_grad(orc, d, got[2]["lp"], got[2]["G"], V, cols=dp.tile_columns(130), L=F[name])
    for a, b in (("LA", "LB"), ("LB", "LD"), ("LA", "LC")):
        assert not cs.same(seen[a][0]["u"], seen[b][0]["u"]), (a, b)     # the structures are different operators


def test_s1_whole_band_form(orc):
    """Q = 2000, 1921 chains: the only small shape at which whole bands are dealt to the workgroups"""
    d = cs.s1_design(2000)
    F = cs.s1_factors(dp.oracle_L(orc, d))
    seen = {}
    with cs.Twin(d) as t:
        for visit, name in enumerate(("LA", "LB", "LA")):
            t.set_L(F[name])
            r = t.sample("%d %s: hmc 1921" % (visit, name), cs.hmc(d, 1921))
            assert r["kernels"] == ("band", "band"), (name, r["kernels"])
            for which in ("fwd", "bwd"):
                p = t.ctx.band_plan(1921, which)
                assert p["used"] and p["built"] and p["paired"] and p["gn"] == 16 and p["nred"] == 0, (name, which, p)
            if name in seen:
                _assert_same(seen[name], r, "the second visit of " + name)
            seen[name] = r
    assert not cs.same(seen["LA"]["u"], seen["LB"]["u"])
    # LA's K-tile ranges cover LB's, so a plan of LA's kept for LB would only multiply zeros and give LB's bits: a second
    # context meets the narrow structure first
    with cs.Twin(d) as t:
        for visit, name in enumerate(("LB", "LA")):
            t.set_L(F[name])
            r = t.sample("second context, %d %s: hmc 1921" % (visit, name), cs.hmc(d, 1921))
            assert r["kernels"] == ("band", "band") and t.ctx.band_plan(1921, "fwd")["paired"], (name, r["kernels"])
            _assert_same(seen[name], r, name + " on the second context")


# ---------------------------------------------------------------------------------------------------------------- S2
def _agree(sparse, dense, what):
    """test_gpu_hmc.py::test_sparse_and_dense_zl_operators_agree"""
    assert np.array_equal(sparse["flags"], dense["flags"]), what
    assert np.abs(sparse["probs"] - dense["probs"]).max() < 1e-9, what
    assert np.abs(sparse["u"] - dense["u"]).max() < 1e-8, what


@pytest.mark.parametrize("C", [70, 130])
@pytest.mark.parametrize("name", ["product", "factored"])
def test_s2_sparse_and_dense_operator_on_one_context(orc, name, C):
    d, theta2, factored = cs.s2_designs()[name]
    Lo = np.asfortranarray(_oracle_L(orc, d))
    V = cs.lpg_input(d, C)

    def sample(t, step, operator):
        r = t.sample(step, cs.hmc(d, C))
        p = t.step(step + ": plans", cs.plans(C))
        if operator == "dense":
            assert set(r["kernels"]) <= DENSE and not p["sparse"]["active"] and not p["component"]["used"], (step, r["kernels"], p)
        else:
            assert p["sparse"]["active"] and p["sparse"]["factored"] == factored, (step, p["sparse"])
            assert not p["band_fwd"]["used"] and not p["band_bwd"]["used"], (step, p)
            comp = operator == "component"
            assert p["component"]["requested"] == comp and p["component"]["used"] == (comp and p["component"]["feasible"]), (step, p)
            assert r["kernels"] == (("component",) * 2 if p["component"]["used"] else ("sparse",) * 2), (step, r["kernels"])
        return r

    with cs.Twin(d) as t:
        t.update_L(d["theta"])
        r2 = sample(t, "2 sparse", "sparse")
        t.set_L(Lo)
        r4 = sample(t, "4 dense", "dense")
        g4 = t.step("4 dense: log_prob_grad", cs.log_prob_grad(d, V))
        assert set(g4["kernels"]) <= DENSE, g4["kernels"]
        _agree(r2, r4, "sparse and dense at theta")
        t.update_L(d["theta"])
        r5 = sample(t, "5 sparse again", "sparse")
        _assert_same(r2, r5, "the second sparse visit of theta")
        t.mode("set_trajectory", "component")
        r6 = sample(t, "6 component", "component")
        if name == "product":
            assert r6["kernels"] == ("component", "component")
        t.set_L(Lo)
        r7 = sample(t, "7 dense, component requested", "dense")
        _assert_same(r4, r7, "the second dense visit of theta")
        t.update_L(theta2)
        r8 = sample(t, "8 component, theta2", "component")
        t.mode("set_trajectory", "step")
        r9 = sample(t, "9 sparse, theta2", "sparse")
        assert not cs.same(r9["u"], r2["u"])
    for r in (r2, r4):
        dp.check_chains(orc, d, r["u"], r["flags"], r["probs"], [0, C - 1], L=Lo)
    assert r8["kernels"] == r6["kernels"]


def test_s2_exact_component_draws_follow_the_operator(orc):
    """set_draws("exact_component"): the component factors on the sparse operator, the dense exact draws after set_L, the
    component factors again at a second theta -- their layout is uploaded once, the factors must follow theta"""
    d, theta2, _ = cs.s2_designs()["gaussian"]
    Lo = np.asfortranarray(_oracle_L(orc, d))
    C = 70
    with cs.Twin(d) as t:
        t.mode("set_draws", "exact_component")
        t.update_L(d["theta"])
        assert t.step("plans", cs.plans(C))["exact_component"]["applicable"]
        r1 = t.sample("1 component draws", cs.hmc(d, C))
        assert r1["kernels"] == ("exact_component", "exact_component"), r1["kernels"]
        t.set_L(Lo)
        p = t.step("plans, dense", cs.plans(C))
        assert p["draws"]["applicable"] and not p["exact_component"]["applicable"], p
        r2 = t.sample("2 dense exact draws", cs.hmc(d, C))
        assert r2["kernels"] == ("exact", "exact"), r2["kernels"]
        t.update_L(theta2)
        r3 = t.sample("3 component draws, theta2", cs.hmc(d, C))
        assert r3["kernels"] == ("exact_component", "exact_component"), r3["kernels"]
        t.update_L(d["theta"])
        r4 = t.sample("4 component draws, theta again", cs.hmc(d, C))
        _assert_same(r1, r4, "the second visit of theta")
    assert not cs.same(r1["u"], r3["u"])


# ---------------------------------------------------------------------------------------------------------------- S3
def test_s3_samplers_draws_and_graph_cache_share_one_context(tmp_path):
    results = cs.s3_sequence(cs.s3_design())
    # ... and every value again from a process that never captures a graph (the switch is read once per process)
    code = ("import sys\nsys.path.insert(0, %r); sys.path.insert(0, %r)\nimport numpy as np\nimport context_sequences as cs\n"
            "np.savez(sys.argv[1], **cs.flatten(cs.s3_sequence(cs.s3_design())))\n" % (ROOT, os.path.join(ROOT, "tests")))
    f = str(tmp_path / "eager.npz")
    subprocess.run([sys.executable, "-c", code, f], check=True, env=dict(os.environ, GLMMR_MCML_CHOL_GRAPH="0"), timeout=300)
    flat = cs.flatten(results)
    with np.load(f) as z:
        assert sorted(z.files) == sorted(flat)
        for k in flat:
            assert cs.same(flat[k], z[k]), "with and without graphs: " + k


# ---------------------------------------------------------------------------------------------------------------- S4
def _queries(d, theta2, bad):
    """name -> query(ctx) -> result; the samples the queries read are those of the sampler call before them"""
    th = np.array(d["theta"], dtype=float)
    vp = cs.vp_of(d)
    V = cs.lpg_input(d, 20)
    rng = np.random.default_rng(41)
    B = rng.normal(size=(300, 300))
    A = np.asfortranarray(B @ B.T + 300 * np.eye(300))
    q = {"gen_D chol": lambda c: c.gen_D(theta2, chol=True),
         "gen_D": lambda c: c.gen_D(theta2, chol=False),
         "mvn_ll": lambda c: c.mvn_ll(theta2),
         "mvn_ll_batch": lambda c: c.mvn_ll_batch(np.array([th, bad, theta2])),
         "log_prob_grad": lambda c: c.log_prob_grad(d["beta"], vp, V),
         "loglik": lambda c: c.loglik(d["beta"], vp),
         "mcnr": lambda c: c.mcnr(d["beta"], vp),
         "aic_mcml": lambda c: c.aic_mcml(np.r_[d["beta"], vp] if d["family"] == "gaussian" else d["beta"], th),
         "dbg_chol": lambda c: c.dbg_chol(A, B=B[:, :3]),
         "plans": lambda c: (cs.plans(40)(c), c.la_plan(), c.last_kernels())}
    if d["X"].shape[1] == 1:
        q["mcml_hess"] = lambda c: c.mcml_hess(np.r_[d["beta"], th, 1.0])
    return q


@pytest.mark.parametrize("which", ["dense", "sparse"])
def test_s4_queries_are_pure(orc, which):
    if which == "dense":
        d, C = cs.s1_design(), 130
        L, theta2, bad = cs.s1_factors(dp.oracle_L(orc, d))["LA"], np.array(cs.THETA2), np.array([-0.05, 0.1])
    else:
        d, theta2, _ = cs.s2_designs()["product"]
        C, L, theta2, bad = 70, None, np.array(theta2), np.array([0.0, 0.1])
    sample = cs.hmc(d, C)
    with cs.new_context(d) as ctx:
        if L is None:
            ctx.update_L(d["theta"])
        else:
            ctx.set_L(L)
        B0 = sample(ctx)
        for name, query in _queries(d, theta2, bad).items():
            got = query(ctx)
            assert cs.same(ctx.get_u(), B0["u"]), name + ": the samples changed"
            _assert_same(B0, sample(ctx), "the sampler call after " + name)
            if name.startswith("gen_D"):
                with api.Context(d["cov"], d["data"], d["eff_range"]) as throwaway:
                    _assert_same(got, query(throwaway), name + " against a throwaway context")
            if name == "mvn_ll_batch":
                # the diagonal blocks of the sparse design have no pivot to fail: a zero variance gives no finite value
                assert np.isfinite(got[0]) and np.isfinite(got[2]), got
                assert np.isnan(got[1]) if which == "dense" else not np.isfinite(got[1]), got
                assert cs.same(float(got[2]), ctx.mvn_ll(theta2)) or abs(got[2] - ctx.mvn_ll(theta2)) <= 1e-10 * abs(got[2])
        Do = orc.gen_D(d["cov"], d["data"], d["eff_range"], theta2, chol=False)
        assert np.abs(ctx.gen_D(theta2, chol=False) - Do).max() <= 1e-12 * np.abs(Do).max()


# ---------------------------------------------------------------------------------------------------------------- S5
@pytest.mark.parametrize("which", ["fexp", "ar1"])
def test_s5_a_call_that_fails(which):
    d, good, bad = cs.bad_thetas()[which]
    C = 130 if which == "fexp" else 70
    sample = cs.hmc(d, C)
    V = cs.lpg_input(d, 20)
    with cs.new_context(d) as ctx:
        ctx.update_L(good)
        B0 = sample(ctx)
        # a query that fails: raises "not positive definite" or gives NaN, and changes nothing
        try:
            assert np.isnan(ctx.mvn_ll(bad))
        except McmlError as e:
            assert e.code == ENOTPD, e
        assert cs.same(ctx.get_u(), B0["u"])
        out = ctx.mvn_ll_batch(np.array([good, bad]))
        assert np.isfinite(out[0]) and np.isnan(out[1]), out
        assert cs.same(ctx.get_u(), B0["u"])
        _assert_same(B0, sample(ctx), "the sampler call after failed mvn_ll calls")
        ctx.update_L(good)                                     # no stale "not positive definite" flag
        _assert_same(B0, sample(ctx), "the sampler call after update_L after failed mvn_ll calls")
        # set_u with a wrong row count: refused, the samples and their shape stay
        with pytest.raises(McmlError):
            ctx.set_u(np.zeros((d["Q"] + 1, C + 3)))
        assert cs.same(ctx.get_u(), B0["u"])
        # a failed update_L: no L afterwards, every consumer refuses
        with pytest.raises(McmlError) as e:
            ctx.update_L(bad)
        assert e.value.code == ENOTPD, e.value
        _refuses(lambda: sample(ctx))
        _refuses(lambda: cs.nuts(d, 4)(ctx))
        _refuses(lambda: cs.log_prob_grad(d, V)(ctx))
        assert cs.same(ctx.get_u(), B0["u"])
        ctx.update_L(good)
        _assert_same(B0, sample(ctx), "the sampler call after update_L restored L")


def test_s5_exact_draws_refuse_after_a_failed_update_L():
    d = cs.s3_design()
    bad = np.array([-0.05, 0.1])
    sample = cs.hmc(d, 40)
    with cs.new_context(d) as ctx:
        ctx.set_draws("exact")
        ctx.update_L(d["theta"])
        B0 = sample(ctx)
        assert B0["kernels"] == ("exact", "exact")
        with pytest.raises(McmlError) as e:
            ctx.update_L(bad)
        assert e.value.code == ENOTPD, e.value
        assert not ctx.draws_plan()["applicable"]
        _refuses(lambda: sample(ctx))
        _refuses(lambda: ctx.exact_sample(d["beta"], cs.vp_of(d), 40, cs.SEED, chains=40))
        ctx.update_L(d["theta"])
        _assert_same(B0, sample(ctx), "the exact draws after update_L restored L")


# ---------------------------------------------------------------------------------------------------------------- S6
def _dc_context(d):
    return api.Context(*dc.args(d), d["family"], d["link"])


def test_s6_after_mcml_full():
    d = dc.case("DP")
    kw = dict(mcnr=True, m=24, maxiter=2, tol=1e-12, warmup=20, lambda_=0.3, maxsteps=8, target_accept=0.9, seed=4242, chains=8)
    with _dc_context(d) as ctx:
        start = np.r_[d["beta"], d["theta"], 1.0]
        r = ctx.mcml_full(start, **kw)
        assert not r["converged"], r
        u = ctx.get_u()
        one = api.mcml_full(*dc.args(d), d["family"], d["link"], start, verbose=False, **kw)
        assert cs.same(u, np.asfortranarray(one["u"])) and cs.same(r["beta"], one["beta"]) and cs.same(r["theta"], one["theta"])
        got = (ctx.mvn_ll(r["theta"]), ctx.loglik(r["beta"], 1.0))
        with _dc_context(d) as fresh:
            fresh.set_u(u)
            want = (fresh.mvn_ll(r["theta"]), fresh.loglik(r["beta"], 1.0))
        _assert_same(got, want, "mvn_ll / loglik after mcml_full")


@pytest.mark.parametrize("driver", ["mcml_optim", "mcml_simlik", "mcml_hess"])
def test_s6_after_the_theta_step_drivers(driver):
    d = dict(dc.case("DG"))
    start = d["start"]
    with cs.Twin(d, make=_dc_context) as t:
        t.set_u(d["u"], d["niter"])
        if driver == "mcml_hess":
            H = t.ctx.mcml_hess(start, tol=1e-4)
            assert np.all(np.isfinite(H))
        else:
            r = getattr(t.ctx, driver)(start, maxfun=60, theta_batch=8)      # rounds of 8 candidates side by side
            assert np.all(np.isfinite(r["theta"]))
        assert cs.same(t.ctx.get_u(), np.asfortranarray(d["u"])), "the driver changed the samples"
        t.update_L(d["theta"])
        r = t.sample("hmc 40 after " + driver, cs.hmc(d, 40))
        assert set(r["kernels"]) <= DENSE, r["kernels"]


def test_s6_after_mcml_la():
    d = dict(dc.case("DP"))
    with cs.Twin(d, make=_dc_context) as t:
        t.update_L(d["theta"])
        t.sample("hmc 24", cs.hmc(d, 24))
        r = t.ctx.mcml_la(d["start"], nr=True, maxiter=2)
        assert np.all(np.isfinite(r["beta"]))
        t.lose_L()                                            # the Laplace fit leaves no L: the caller sets it again
        _refuses(lambda: cs.hmc(d, 24)(t.ctx))
        t.update_L(d["theta"])
        t.sample("hmc 24 after mcml_la", cs.hmc(d, 24))
        t.step("log_prob_grad after mcml_la", cs.log_prob_grad(d, cs.lpg_input(d, 24)))
