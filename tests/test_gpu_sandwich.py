"""The cluster-robust sandwich query on the device (csrc/sandwich.hip: Context.sandwich, api.sandwich, ModelMCML.sandwich,
MCML(..., sandwich=)) against the definition.

The reference is tests/sandwich_reference.py: a = Sigma^-1 e by a long-double Cholesky solve, D being the float64 matrix the
device's own gen_D returns; scores G[c] = sum_{i in c} x_i a_i.  The scores are held to their uncancelled scale,

    max |G_dev - G_ref| <= C_SAND * 2^-52 * S_G,    C_SAND = 8 x the float64 twin's worst ratio = 4

calibrated on these very cases by tests/test_sandwich_reference_cpu.py, and the meat to the derived worst case of any order of
its sum, |B_dev - G_dev' G_dev| <= (ncl + 2) 2^-52 sum_c |G_ca G_cb|.  The bread is the information query's matrix to the bit.
Measured on an MI355X: worst score ratio 1.124 of 4 (family-gamma-log; next densez_poisson_log 0.805, family-poisson-log
0.715), worst meat ratio 0.231 of 1 (comp129); ModelMCML.sandwich device against host 1.983 of 8 (densez_poisson_log).
Every case is one of the small ones of information_reference.py and takes seconds."""
import ctypes as C

import numpy as np
import pytest

import information_reference as ir
import sandwich_reference as sr
from glmmrmcml_amd import _lib, api, synth
from glmmrmcml_amd.model import ModelMCML, components_of_rows

pytestmark = pytest.mark.gpu
LD = sr.LD


def context(c):
    return api.Context(c["cov"], c["data"], c["eff_range"], c["Z"], c["X"], c["y"], c["family"], c["link"])


@pytest.fixture(scope="module")
def refs():
    """name -> (D from the device, (a, G, B) in long double, S_G): computed once, shared, read-only"""
    out, Ds = {}, {}
    for name in sr.NAMES:
        c = sr.case(name)
        if c["key"] not in Ds:
            with api.Context(c["cov"], c["data"], c["eff_range"]) as ctx:
                Ds[c["key"]] = ctx.gen_D(c["theta"])
        D = Ds[c["key"]]
        a, G, B = sr.reference(c, D)
        for arr in (D, a, G, B):
            arr.setflags(write=False)
        out[name] = (D, (a, G, B), sr.score_scale(c, D))
    return out


def check(name, r, G_ref, scale, what="device"):
    rs, rm = sr.ratio(r["scores"], G_ref, scale), sr.meat_excess(r["meat"], r["scores"])
    print("%s %s: score ratio %.3f of C_SAND %.1f (S_G %.3g), meat ratio %.3f of 1" % (name, what, rs, sr.C_SAND, scale, rm))
    assert rs <= sr.C_SAND, (name, what, rs)
    assert rm <= 1.0, (name, what, rm)
    assert np.array_equal(r["meat"], r["meat"].T)
    assert r["ncluster"] == G_ref.shape[0] == r["scores"].shape[0]
    want = np.linalg.solve(r["information"], np.linalg.solve(r["information"], r["meat"]).T)
    assert np.array_equal(r["vcov"], want)


def run(name, refs, operator=None):
    """the query on a fresh context with theta given -> (result, plan); checked against the reference"""
    c = sr.case(name)
    with context(c) as ctx:
        r = ctx.sandwich(c["beta"], c["var_par"], theta=c["theta"], cluster=c["cluster"], operator=operator, scores=True)
        plan = ctx.sandwich_plan()
    D, (a, G, B), scale = refs[name]
    check(name, r, G, scale)
    assert plan["P"] == c["X"].shape[1] and plan["ncluster"] == G.shape[0]
    assert plan["default_clusters"] == (c["cluster"] is None)
    return r, plan


# ---------------------------------------------------------------------------------------------- the operators
@pytest.mark.parametrize("name", ir.FAMILY_KEYS)
def test_staged_items_on_every_family_and_link(name, refs):
    r, plan = run(name, refs)
    assert plan["op"] == 1 and plan["dense_bytes"] == 0 and plan["requested"] == 0
    assert (plan["ncluster"], plan["max_rows"]) == (6, 24) and plan["launches"] == 7


@pytest.mark.parametrize("name", ["longitudinal_70x3", "stepped_wedge_7x8x3", "longitudinal_70x3+across",
                                  "stepped_wedge_7x8x3+unions"])
def test_staged_items_pack_components_into_a_wave(name, refs):
    r, plan = run(name, refs)
    assert plan["op"] == 1 and plan["dense_bytes"] == 0
    assert plan["ncluster"] == {"longitudinal_70x3": 70, "stepped_wedge_7x8x3": 7, "longitudinal_70x3+across": 5,
                                "stepped_wedge_7x8x3+unions": 3}[name]


@pytest.mark.parametrize("waves", ["1", "4"])
@pytest.mark.parametrize("name", ir.WIDE_KEYS)
def test_one_wave_per_component(name, waves, refs, monkeypatch):
    """41 variables per component: k_comp_solve_wave works a component with the whole wave"""
    monkeypatch.setenv("GLMMR_MCML_LA_WAVES", waves)                   # the factor kernel's, read per call
    r, plan = run(name, refs)
    assert plan["op"] == 2 and plan["dense_bytes"] == 0 and (plan["ncluster"], plan["launches"]) == (3, 7)


@pytest.mark.parametrize("name", sr.DENSE_NAMES)
def test_dense_path(name, refs):
    r, plan = run(name, refs)
    assert plan["op"] == 0 and plan["dense_bytes"] > 0 and plan["launches"] == 5 and not plan["default_clusters"]


def test_dense_operator_on_a_sparse_context(refs):
    name = "stepped_wedge_7x8x3"
    c = sr.case(name)
    comp, _ = run(name, refs)
    D, (a, G, B), scale = refs[name]
    with context(c) as ctx:
        dense = ctx.sandwich(c["beta"], c["var_par"], theta=c["theta"], operator="dense", scores=True)
        plan = ctx.sandwich_plan()
        assert plan["requested"] == 1 and plan["op"] == 0 and plan["dense_bytes"] > 0 and plan["default_clusters"]
        check(name, dense, G, scale, "dense operator")
        again = ctx.sandwich(c["beta"], c["var_par"], scores=True)     # the context's operator is still the sparse one
        assert ctx.sandwich_plan()["op"] == 1 and ctx.sparse_plan(1)["active"]
        for k in ("information", "meat", "scores"):
            assert np.array_equal(again[k], comp[k]), k


# ---------------------------------------------------------------------------------------------- the bread
@pytest.mark.parametrize("name,operator", [("family-poisson-log", None), ("wide_41", "component"), ("geo300_p3", None),
                                           ("stepped_wedge_7x8x3", "dense")])
def test_bread_is_the_information_query_to_the_bit(name, operator):
    c = sr.case(name)
    with context(c) as ctx:
        r = ctx.sandwich(c["beta"], c["var_par"], theta=c["theta"], cluster=c["cluster"], operator=operator)
        info = ctx.information_matrix(c["beta"], c["var_par"], operator=operator)
        assert ctx.information_plan()["op"] == ctx.sandwich_plan()["op"]
    assert np.array_equal(r["information"], info) and "scores" not in r


# ---------------------------------------------------------------------------------------------- clusters
def test_default_clusters_equal_explicit_component_ids(refs):
    name = "longitudinal_70x3"
    c = sr.case(name)
    with context(c) as ctx:
        ids, ncomp = components_of_rows(c["Z"] @ ctx.gen_D(c["theta"], chol=True))
        assert ncomp == 70
        a = ctx.sandwich(c["beta"], c["var_par"], theta=c["theta"], scores=True)
        b = ctx.sandwich(c["beta"], c["var_par"], cluster=ids, scores=True)
        assert not ctx.sandwich_plan()["default_clusters"]
    assert a["ncluster"] == b["ncluster"] == 70
    for k in ("information", "meat", "scores", "vcov"):
        assert np.array_equal(a[k], b[k]), k


def test_permuting_the_labels_permutes_the_scores(refs):
    name = "geo300_p3"
    c = sr.case(name)
    perm = np.random.default_rng(5).permutation(12)
    with context(c) as ctx:
        a = ctx.sandwich(c["beta"], c["var_par"], theta=c["theta"], cluster=c["cluster"], scores=True)
        b = ctx.sandwich(c["beta"], c["var_par"], cluster=perm[c["cluster"]], scores=True)
    assert np.array_equal(b["scores"][perm], a["scores"])              # a cluster's sum does not depend on its label
    assert sr.meat_excess(b["meat"], a["scores"]) <= 1.0 and sr.meat_excess(a["meat"], a["scores"]) <= 1.0


def test_both_forms_of_the_score_kernel(refs, monkeypatch):
    """two clusters of 105 rows: a lane of the wave form adds two rows, a thread of the workgroup form one"""
    c = dict(sr.case("longitudinal_70x3"))
    c["cluster"] = (np.arange(210) % 2).astype(np.int32)
    D = refs["longitudinal_70x3"][0]
    a, G, B = sr.reference(c, D)
    scale = sr.score_scale(c, D)
    got = {}
    with context(c) as ctx:
        for form in ("wave", "wg"):
            monkeypatch.setenv("GLMMR_MCML_SAND_SCORES", form)         # read per call
            got[form] = ctx.sandwich(c["beta"], c["var_par"], theta=c["theta"], cluster=c["cluster"], scores=True)
            assert ctx.sandwich_plan()["max_rows"] == 105
            check("two clusters of 105", got[form], G, scale, form)
    assert np.array_equal(got["wave"]["information"], got["wg"]["information"])
    assert sr.ratio(got["wave"]["scores"], got["wg"]["scores"].astype(LD), scale) <= 2 * sr.C_SAND


# ---------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("name", ["geo300_p3", "stepped_wedge_7x8x3", "wide_41"])
def test_two_calls_and_two_contexts_give_the_same_bits(name):
    c = sr.case(name)
    with context(c) as ctx:
        a = ctx.sandwich(c["beta"], c["var_par"], theta=c["theta"], cluster=c["cluster"], scores=True)
        b = ctx.sandwich(c["beta"], c["var_par"], theta=c["theta"], cluster=c["cluster"], scores=True)
    with context(c) as ctx:
        ctx.update_L(c["theta"])
        d = ctx.sandwich(c["beta"], c["var_par"], cluster=c["cluster"], scores=True)
    for k in ("information", "meat", "scores"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], d[k]), k


def test_it_is_a_query():
    """mvn_ll, its score, a seeded hmc_sample, the information and the prediction query return the same bits with sandwich
    calls in between; with theta = None the resident L is the one of the last update_L"""
    c = sr.case("stepped_wedge_7x8x3")
    u = np.random.default_rng(3).standard_normal((56, 3)) * 0.3
    newdata = [np.array([[1.0, 2.5]])] + [None] * 6

    def values(query):
        with context(c) as ctx:
            ctx.update_L(c["theta"])
            ctx.set_u(u)
            if query:
                ctx.sandwich(c["beta"], c["var_par"], scores=True)
                ctx.sandwich(c["beta"] * 0.5, c["var_par"], cluster=np.arange(168) % 4, operator="dense")
            ll, grad = ctx.mvn_ll(c["theta"]), ctx.mvn_ll_grad(c["theta"])
            info = ctx.information_matrix(c["beta"], c["var_par"])
            pred = ctx.predict_re(c["theta"], newdata, means=True)
            if query:
                ctx.sandwich(c["beta"], c["var_par"])
            ctx.hmc_sample(c["beta"], c["var_par"], 3, 4, 0.5, 5, 0.9, seed=11, chains=2)
            return ll, grad, info, pred, ctx.get_u()

    a, b = values(True), values(False)
    assert a[0] == b[0] and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1])
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[4], b[4])
    for k in b[3]:
        assert np.array_equal(a[3][k], b[3][k], equal_nan=True), k


# ---------------------------------------------------------------------------------------------- refusals
def _raw(ctx, c, cluster, ncluster, theta=None, op=0):
    """the C entry point with outputs pre-filled with 7 -> (code, info, meat, scores, ncluster_out)"""
    P, n = c["X"].shape[1], c["X"].shape[0]
    info, meat = np.full((P, P), 7.0, order="F"), np.full((P, P), 7.0, order="F")
    G = np.full((n, P), 7.0, order="F")
    got = C.c_int(-7)
    beta = np.ascontiguousarray(c["beta"], dtype=np.float64)
    th = None if theta is None else np.ascontiguousarray(theta, dtype=np.float64)
    cl = None if cluster is None else np.ascontiguousarray(cluster, dtype=np.int32)
    rc = _lib.lib().glmmr_mcml_ctx_sandwich(ctx._h, api._p(beta), float(c["var_par"]), api._p(th), op, api._p(cl), ncluster,
                                            api._p(info), P, api._p(meat), P, api._p(G), n, C.byref(got))
    return rc, info, meat, G, got.value


def _unwritten(res):
    rc, info, meat, G, got = res
    return np.all(info == 7.0) and np.all(meat == 7.0) and np.all(G == 7.0) and got == -7


def test_refusals_leave_the_outputs_unwritten():
    c = sr.case("geo150_p1")
    with context(c) as ctx:
        ctx.update_L(c["theta"])
        res = _raw(ctx, c, None, 0)                                    # no plan on a dense context
        msg = _lib.lib().glmmr_mcml_last_error()
        assert res[0] == -1 and b"explicit cluster ids" in msg and _unwritten(res)
        ids = c["cluster"].copy()
        ids[17] = 12
        res = _raw(ctx, c, ids, 12)                                    # an id equal to ncluster
        assert res[0] == -1 and b"outside" in _lib.lib().glmmr_mcml_last_error() and _unwritten(res)
        res = _raw(ctx, c, c["cluster"], 0)
        assert res[0] == -1 and _unwritten(res)
        res = _raw(ctx, c, c["cluster"], 12, op=2)                     # the component operator on a dense context
        assert res[0] == -2 and _unwritten(res)
        with pytest.raises(_lib.McmlError) as e:
            ctx.sandwich(c["beta"], c["var_par"])
        assert e.value.code == -1
        res = _raw(ctx, c, c["cluster"], 12)                           # and the context still answers
        assert res[0] == 0 and res[4] == 12 and not np.any(res[1] == 7.0) and not np.any(res[3][:12] == 7.0)
        assert np.all(res[3][12:] == 7.0)
    c = sr.case("stepped_wedge_7x8x3")
    with context(c) as ctx:
        res = _raw(ctx, c, None, 0, theta=np.array([0.25, 1.5]))       # an AR1 parameter above 1: D is not positive definite
        assert res[0] == -3 and _unwritten(res)
        r = ctx.sandwich(c["beta"], c["var_par"], theta=c["theta"])
        assert r["ncluster"] == 7 and np.all(np.isfinite(r["vcov"]))


def test_a_residual_that_is_not_finite_raises():
    """poisson / log with a linear predictor of 800: h overflows"""
    c = dict(sr.case("family-poisson-log"))
    beta = c["beta"].copy()
    beta[0] = 800.0
    with context(c) as ctx:
        with pytest.raises(_lib.McmlError) as e:
            ctx.sandwich(beta, c["var_par"], theta=c["theta"])
        assert e.value.code == -1
        assert np.all(np.isfinite(ctx.sandwich(c["beta"], c["var_par"])["vcov"]))


# ---------------------------------------------------------------------------------------------- the caller layer
def test_one_shot_export_equals_the_context_query():
    c = sr.case("family-gamma-log")
    with context(c) as ctx:
        want = ctx.sandwich(c["beta"], c["var_par"], theta=c["theta"], scores=True)
    got = api.sandwich(c["cov"], c["data"], c["eff_range"], c["Z"], c["X"], c["y"], c["family"], c["link"], c["beta"], c["theta"],
                       var_par=c["var_par"], scores=True)
    for k in ("information", "meat", "scores", "vcov"):
        assert np.array_equal(got[k], want[k]), k
    assert got["ncluster"] == want["ncluster"] == 6


@pytest.mark.parametrize("name", ["family-gamma-inverse", "densez_poisson_log", "stepped_wedge_7x8x3+unions"])
def test_model_sandwich_device_against_host(name, refs):
    """Both lie within C_SAND eps S_G of the definition, so their scores differ by at most twice that.  vcov is what the two
    solves make of the device's own I and B: a solve is backward stable, (I + E) X = B with |E| <= c P eps |I| (Higham,
    Accuracy and Stability, 9.3), so each of the two leaves a residual of at most c P eps |I| |X| and I vcov I differs from B by
    at most 2 c P^2 eps cond(I) max|B| entrywise; c = 4 covers the growth of partial pivoting on these P <= 9 matrices"""
    c = sr.case(name)
    D, (a, G, B), scale = refs[name]
    m = ModelMCML(c["cov"], c["data"], c["eff_range"], c["Z"], c["X"], ir.model_family(c["family"]), c["link"], c["beta"],
                  c["theta"], var_par=c["var_par"])
    dev = m.sandwich(c["y"], c["theta"], c["beta"], c["var_par"], cluster=c["cluster"], on="device")
    host = m.sandwich(c["y"], c["theta"], c["beta"], c["var_par"], cluster=c["cluster"], on="host")
    r = sr.ratio(dev["scores"], host["scores"].astype(LD), scale)
    print("%s device against host: %.3f of %.1f" % (name, r, 2 * sr.C_SAND))
    assert r <= 2 * sr.C_SAND and dev["ncluster"] == host["ncluster"] == G.shape[0]
    for p in (dev, host):
        I, P = p["information"], c["X"].shape[1]
        tol = 8 * P * P * sr.EPS * np.linalg.cond(I) * np.abs(p["meat"]).max()
        assert np.all(np.abs(I @ p["vcov"] @ I - p["meat"]) <= tol)
        assert np.array_equal(p["se"], np.sqrt(np.diag(p["vcov"])))


def test_mcml_fit_with_a_robust_record():
    d = synth.cluster_rct()
    mod = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["family"], d["link"], d["beta"], d["theta"])
    mod.mcmc_options.update(warmup=20, samps=16)
    fit = mod.MCML(d["y"], max_iter=2, verbose=False, seed=5, sandwich="CR1")
    plain = mod.MCML(d["y"], max_iter=2, verbose=False, seed=5)
    rb = fit["robust"]
    P = d["P"]
    assert rb["adjust"] == "CR1" and rb["ncluster"] == 10 and rb["vcov"].shape == (P, P)
    assert np.all(np.isfinite(rb["se"])) and np.all(rb["se"] > 0)
    assert "robust" not in plain and str(fit) == str(plain)
    for key in ("est", "SE", "lower", "upper"):
        assert np.array_equal(fit["coefficients"][key], plain["coefficients"][key], equal_nan=True), key
    assert fit["coefficients"]["par"] == plain["coefficients"]["par"]
    cr0 = mod.sandwich(d["y"], fit["theta"][P:P + 2], fit["theta"][:P], 1.0, adjust="CR0")
    assert np.array_equal(rb["vcov"], cr0["vcov"] * (10 / 9.0 * (d["n"] - 1.0) / (d["n"] - P)))
