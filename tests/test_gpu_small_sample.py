"""The small-sample query on the device (csrc/small_sample.hip: Context.small_sample, api.small_sample,
ModelMCML.small_sample / MCML(small_sample=) / LA(small_sample=)) against the definition.

The reference is tests/small_sample_reference.py: P_r, Q_rs and R_rs on the n x n matrices by long-double Cholesky solves, D being
the float64 matrix the device's own gen_D returns, d_r D and d2_rs D analytic.  The bound is per output block against the block's
uncancelled scale S,

    max |dev - ref| <= C_SS * 2^-52 * S,    C_SS = 8 x the float64 twin's worst ratio = 136,

calibrated on these very cases by tests/test_small_sample_reference_cpu.py (the twin's worst ratio 16.626, rounded up to 17).
Measured on an MI355X, worst block ratio to 2^-52 S: 30.4 (family-poisson-log, component operator, Q_00), then 29.5
(family-binomial-logit), 21.3 (family-gaussian-identity), 10.5 (family-gamma-log), 8.8 (wide_41), 8.7 (weak), 4.1 (mixed), 3.8
(comp65), 3.7 (wide_41_p71), 2.9 (densez_poisson_log), 0.9 (longitudinal_70x3), 0.02 .. 0.13 (stepped_wedge_7x8x3, split_block,
geo150, geo300); the dense operator on a sparse context 0.02, 2.8 and 12.2 (wide_41); against the host formula 24.9 of 148.
Every case is the smallest at which its branch can go wrong; `why` in theta_information_reference.py says which branch."""
import numpy as np
import pytest

import family_designs as fd
import small_sample_reference as sr
from glmmrmcml_amd import _lib, api
from glmmrmcml_amd.model import ModelMCML

pytestmark = pytest.mark.gpu


def context(c, y=None):
    y = np.zeros(c["X"].shape[0]) if y is None else y                  # the query does not read y
    return api.Context(c["cov"], c["data"], c["eff_range"], c["Z"], c["X"], y, c["family"], c["link"])


@pytest.fixture(scope="module")
def refs():
    """key -> (long-double reference, scales) from the device's D: computed once, shared, read-only"""
    out = {}
    for key in sr.KEYS:
        c = sr.case(key)
        with api.Context(c["cov"], c["data"], c["eff_range"]) as ctx:
            D = ctx.gen_D(c["theta"])
        ref = sr.reference(c, D)
        for a in ref.values():
            a.setflags(write=False)
        out[key] = (ref, sr.scales(c, D))
    return out


def check(key, got, refs, what="device", extra=0.0):
    ref, sc = refs[key]
    br = sr.block_ratios(got, ref, sc)
    at = max(br, key=br.get)
    print("%s %s: worst block ratio %.3f at %s of C_SS %.1f" % (key, what, br[at], at, sr.C_SS + extra))
    assert br[at] <= sr.C_SS + extra, (key, what, at, br[at])
    return br[at]


def query(c, operator=None, ctx=None):
    if ctx is not None:
        return ctx.small_sample(c["beta"], c["var_par"], c["theta"], operator=operator)
    with context(c) as own:
        return own.small_sample(c["beta"], c["var_par"], c["theta"], operator=operator)


def expected_bytes(c, comp):
    """what the new part allocates: Q x P for c and d, Q x (R + the pairs r >= s some block reads together) P for U and V, twice
    Q x R P on the way to Y, and for gaussian / identity four n x P and two Q x P; leading dimensions padded to 32 rows.
    Nothing of size Q x Q"""
    import cov_layouts as cl
    import theta_information_reference as tr
    pad = lambda r: (max(r, 1) + 31) // 32 * 32
    n, Q = c["Z"].shape
    P, R = c["X"].shape[1], c["theta"].size
    pairs = set()
    for block in cl.from_wire(c["cov"], c["data"]):
        read = sorted(tr.dlog(block, c["theta"], np.float64))
        pairs |= {(r, s) for r in read for s in read if s <= r}
    cols = 2 * P + (R + len(pairs)) * P + 2 * R * P
    b = pad(Q) * cols
    if sr.sigma_row(c):
        b += 4 * pad(n) * P + 2 * pad(Q) * P
    return 8 * b


def symmetric(r):
    no = r["P"].shape[0]
    for a in range(no):
        assert np.array_equal(r["P"][a], r["P"][a].T)
        assert np.array_equal(r["Q"][a, a], r["Q"][a, a].T)
        for b in range(no):
            assert np.array_equal(r["R"][a, b], r["R"][a, b].T) and np.array_equal(r["R"][a, b], r["R"][b, a])
            assert np.array_equal(r["Q"][a, b], r["Q"][b, a].T)


def run(key, refs, operator=None):
    """the query on a fresh context -> (result, plan); checked against the reference, the two information blocks against the
    queries they come from, on the operator that ran"""
    c = sr.case(key)
    with context(c) as ctx:
        r = query(c, operator, ctx)
        plan = ctx.small_sample_plan()
        op = "component" if plan["op"] == 1 else "dense"
        info = ctx.information_matrix(c["beta"], c["var_par"], c["theta"], operator=op)
        tinfo = ctx.theta_information(c["beta"], c["var_par"], c["theta"], operator=op)
    no, P = sr.rows(c), c["X"].shape[1]
    assert r["P"].shape == (no, P, P) and r["Q"].shape == (no, no, P, P) and r["R"].shape == (no, no, P, P)
    assert all(np.all(np.isfinite(r[k])) for k in ("P", "Q", "R")) and r["names"] == sr.names(c)
    assert np.array_equal(r["information"], info) and np.array_equal(r["theta_information"], tinfo["information"])
    symmetric(r)
    check(key, r, refs)
    assert plan["R"] == c["theta"].size and plan["rows"] == no
    assert plan["bytes"] == expected_bytes(c, plan["op"] == 1)
    return r, plan


# ---------------------------------------------------------------------------------------------- the two operators
@pytest.mark.parametrize("key", sr.COMPONENT_KEYS)
def test_component_path(key, refs):
    r, plan = run(key, refs)
    assert plan["requested"] == 0 and plan["op"] == 1
    assert (plan["ncomp"], plan["max_vars"]) == sr.case(key)["comps"]
    # k_ss_comp_back, k_ss_apply, k_ss_comp_y, k_ss_gram and its final; gaussian / identity: two k_ss_ell, two k_ss_resid, one
    # more k_ss_comp_back -- whatever the number of components
    assert plan["launches"] == (10 if sr.sigma_row(sr.case(key)) else 5)


@pytest.mark.parametrize("key", sr.DENSE_KEYS)
def test_dense_path(key, refs):
    r, plan = run(key, refs)
    assert plan["requested"] == 0 and plan["op"] == 0
    assert plan["launches"] == (5 if sr.sigma_row(sr.case(key)) else 3)       # k_ss_apply, the Gram pair; two k_ss_resid
    comps = sr.case(key)["comps"]
    if comps is not None:                                               # a sparse context whose plan does not qualify
        assert (plan["ncomp"], plan["max_vars"]) == comps


@pytest.mark.parametrize("key", ["stepped_wedge_7x8x3", "family-gaussian-identity", "wide_41"])
def test_dense_operator_on_a_sparse_context(key, refs):
    c = sr.case(key)
    with context(c) as ctx:
        comp = query(c, None, ctx)
        assert ctx.small_sample_plan()["op"] == 1
        dense = query(c, "dense", ctx)
        plan = ctx.small_sample_plan()
        assert plan["requested"] == 1 and plan["op"] == 0
        check(key, comp, refs, "component operator")
        check(key, dense, refs, "dense operator")
        symmetric(dense)
        assert np.array_equal(dense["information"], ctx.information_matrix(c["beta"], c["var_par"], c["theta"], operator="dense"))
        again = query(c, None, ctx)                                     # the context's operator is still the sparse one
        assert ctx.small_sample_plan()["op"] == 1 and ctx.sparse_plan(1)["active"]
        for k in ("information", "theta_information", "P", "Q", "R"):
            assert np.array_equal(again[k], comp[k]), k


# ---------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("key", ["geo300", "stepped_wedge_7x8x3", "mixed"])
def test_bits(key):
    """two calls and two contexts give the same bits"""
    c = sr.case(key)
    with context(c) as ctx:
        a = query(c, None, ctx)
        b = query(c, None, ctx)
    d = query(c)
    for k in ("information", "theta_information", "P", "Q", "R"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], d[k]), k


def test_the_query_leaves_a_laplace_fit_its_bits():
    c = sr.case("stepped_wedge_7x8x3")

    def fit(with_query):
        with context(c, c["y"]) as ctx:
            ctx.update_L(c["theta"])
            if with_query:
                query(c, None, ctx)
                ctx.small_sample(c["beta"] * 0.5, c["var_par"], c["theta"] * 1.1, operator="dense")
                ctx.update_L(c["theta"])
            return ctx.mcml_la(c["start"], nr=True, maxiter=1)

    a, b = fit(True), fit(False)
    for k in ("beta", "theta", "u"):
        assert np.array_equal(a[k], b[k]), k
    assert a["sigma"] == b["sigma"] and a["iters"] == b["iters"]


def test_the_query_leaves_mvn_ll_the_sampler_and_the_other_queries_their_bits():
    c = sr.case("geo300")
    u = np.random.default_rng(3).standard_normal((300, 3)) * 0.3

    def values(with_query):
        with context(c, c["y"]) as ctx:
            ctx.update_L(c["theta"])
            ctx.set_u(u)
            if with_query:
                query(c, None, ctx)                                     # leaves the context as update_L(theta) leaves it
            ll = ctx.mvn_ll(c["theta"])
            ctx.hmc_sample(c["beta"], c["var_par"], 3, 4, 0.5, 5, 0.9, seed=11, chains=2)
            return (ll, ctx.get_u(), ctx.information_matrix(c["beta"], c["var_par"]),
                    ctx.theta_information(c["beta"], c["var_par"], c["theta"])["information"])

    (la, ua, ia, ta), (lb, ub, ib, tb) = values(True), values(False)
    assert la == lb and np.array_equal(ua, ub) and np.array_equal(ia, ib) and np.array_equal(ta, tb)


# ---------------------------------------------------------------------------------------------- refusals
def test_theta_is_required_also_after_set_L():
    c = sr.case("family-poisson-log")
    with context(c) as ctx:
        ctx.update_L(c["theta"])
        with pytest.raises(_lib.McmlError) as e:
            ctx.small_sample(c["beta"], c["var_par"], None)
        assert e.value.code == -1 and "theta" in str(e.value)
        ctx.set_L(np.eye(c["Z"].shape[1]))                              # a foreign L carries no parameter values
        with pytest.raises(_lib.McmlError) as e:
            ctx.small_sample(c["beta"], c["var_par"], None)
        assert e.value.code == -1
        good = query(c, None, ctx)                                      # theta given: L is made from it again
        assert np.all(np.isfinite(good["P"]))


def test_a_weight_that_is_not_finite_raises():
    """gamma / inverse: dhdmu = 1 / eta^2; beta[1] = 0 puts the linear predictor of the first period's control rows at 0"""
    d = fd.design("gamma", "inverse", ncl=6, nt=3, nind=8)
    c = dict(cov=d["cov"], data=d["data"], eff_range=d["eff_range"], Z=np.asfortranarray(d["Z"]), X=np.asfortranarray(d["X"]),
             family="gamma", link="inverse", beta=np.asarray(d["beta"], float), theta=np.asarray(d["theta"], float),
             var_par=fd.VAR_PAR[("gamma", "inverse")])
    beta = c["beta"].copy()
    beta[1] = 0.0
    assert np.any(c["X"] @ beta == 0.0)
    for operator in (None, "dense"):
        with context(c) as ctx:
            with pytest.raises(_lib.McmlError) as e:
                ctx.small_sample(beta, c["var_par"], c["theta"], operator=operator)
            assert e.value.code == -1 and "weight" in str(e.value)
            good = query(c, operator, ctx)                              # the context is usable afterwards
            assert np.all(np.isfinite(good["Q"])) and good["P"].shape[0] == 2


@pytest.mark.parametrize("key", ["geo150", "comp65", "split_block"])
def test_component_operator_where_it_does_not_apply(key):
    c = sr.case(key)
    with context(c) as ctx:
        with pytest.raises(_lib.McmlError) as e:
            query(c, "component", ctx)
        assert e.value.code == -2 and "small_sample" in str(e.value)
        with pytest.raises(KeyError):
            query(c, "component_wide", ctx)


def test_a_theta_that_makes_D_not_positive_definite():
    """ar1 with rho = 1.5: the leading 2 x 2 minor of every block is t^4 (1 - 2.25) < 0"""
    c = sr.case("stepped_wedge_7x8x3")
    theta = np.array([c["theta"][0], 1.5])
    with context(c) as ctx:
        with pytest.raises(_lib.McmlError) as e:
            ctx.small_sample(c["beta"], c["var_par"], theta)
        assert e.value.code == -3
        good = query(c, None, ctx)                                      # and the context recovers
        assert np.all(np.isfinite(good["R"]))


def _raw_call(ctx, c, beta, theta, op):
    """the C entry point with sentinel buffers of the test's own -> (return code, *nout, whether every buffer is untouched)"""
    import ctypes as C
    P, R = c["X"].shape[1], np.asarray(c["theta"]).size
    bufs = [np.full(k, 7.0) for k in (P * P, (R + 1) ** 2, (R + 1) * P * P, (R + 1) ** 2 * P * P, (R + 1) ** 2 * P * P)]
    got = C.c_int(-5)
    ptr = lambda a: np.ascontiguousarray(a, float).ctypes.data_as(C.c_void_p)
    beta, theta = np.ascontiguousarray(beta, float), np.ascontiguousarray(theta, float)
    rc = _lib.lib().glmmr_mcml_ctx_small_sample(ctx._h, ptr(beta), float(c["var_par"]), ptr(theta), op, bufs[0].ctypes.data_as(C.c_void_p),
                                                P, bufs[1].ctypes.data_as(C.c_void_p), R + 1, bufs[2].ctypes.data_as(C.c_void_p),
                                                bufs[3].ctypes.data_as(C.c_void_p), bufs[4].ctypes.data_as(C.c_void_p), C.byref(got))
    return rc, got.value, all(np.all(b == 7.0) for b in bufs)


def test_outputs_are_not_written_on_an_error():
    """the C entry point with buffers of its own: a refused operator, a weight that is not finite (both operators: the kernels run
    and the flag comes back with the download) and a D(theta) that is not positive definite leave them as they were"""
    c = sr.case("comp65")
    with context(c) as ctx:
        assert _raw_call(ctx, c, c["beta"], c["theta"], 2) == (-2, -5, True)
    d = fd.design("gamma", "inverse", ncl=6, nt=3, nind=8)
    g = dict(X=np.asfortranarray(d["X"]), theta=np.asarray(d["theta"], float), var_par=fd.VAR_PAR[("gamma", "inverse")])
    beta = np.asarray(d["beta"], float).copy()
    beta[1] = 0.0
    with api.Context(d["cov"], d["data"], d["eff_range"], np.asfortranarray(d["Z"]), g["X"], np.zeros(g["X"].shape[0]), "gamma",
                     "inverse") as ctx:
        for op in (0, 1):
            assert _raw_call(ctx, g, beta, g["theta"], op) == (-1, -5, True), op
        rc, nout, untouched = _raw_call(ctx, g, d["beta"], g["theta"], 0)       # and a good call writes them
        assert rc == 0 and nout == 2 and not untouched
    c = sr.case("stepped_wedge_7x8x3")
    with context(c) as ctx:
        assert _raw_call(ctx, c, c["beta"], np.array([c["theta"][0], 1.5]), 0) == (-3, -5, True)


# ---------------------------------------------------------------------------------------------- the caller layers
def test_one_shot_export_equals_the_context_query():
    for key in ("family-gamma-log", "geo150"):
        c = sr.case(key)
        want = query(c)
        got = api.small_sample(c["cov"], c["data"], c["eff_range"], c["Z"], c["X"], c["family"], c["link"], c["beta"], c["theta"],
                               var_par=c["var_par"])
        for k in ("information", "theta_information", "P", "Q", "R"):
            assert np.array_equal(got[k], want[k]), k
        assert got["names"] == want["names"]


@pytest.mark.parametrize("key", ["family-gaussian-identity", "stepped_wedge_7x8x3"])
def test_model_device_against_host(key, refs):
    """ModelMCML.small_sample(on="device") against on="host", on the blocks behind the two (_small_sample_blocks): they lie within
    (C_SS + HOST_RATIO) eps S of each other, the device's bound plus the host formula's measured ratio against the long-double
    reference (tests/test_small_sample_reference_cpu.py, and for the model's own host path test_model_small_sample_cpu.py).
    api.small_sample is held to the same.  vcov and dof are smooth functions of the blocks: with I_beta and I_theta well
    conditioned here they agree to a relative 1e-8, far below a wrong term"""
    c = sr.case(key)
    m = ModelMCML(c["cov"], c["data"], c["eff_range"], c["Z"], c["X"], c["family"], c["link"], c["beta"], c["theta"],
                  var_par=c["var_par"])
    sc = refs[key][1]
    host = m._small_sample_blocks(c["theta"], c["beta"], c["var_par"], "host")
    host_ld = {k: host[k].astype(sr.LD) for k in ("P", "Q", "R")}
    dev_m = m._small_sample_blocks(c["theta"], c["beta"], c["var_par"], "device")
    dev_a = api.small_sample(c["cov"], c["data"], c["eff_range"], c["Z"], c["X"], c["family"], c["link"], c["beta"], c["theta"],
                             var_par=c["var_par"])
    for what, dev in (("ModelMCML on=device", dev_m), ("api.small_sample", dev_a)):
        worst = max(sr.block_ratios(dev, host_ld, sc).values())
        print("%s %s against the model's host path: %.3f of %.1f" % (key, what, worst, sr.C_SS + sr.HOST_RATIO))
        assert worst <= sr.C_SS + sr.HOST_RATIO, (key, what, worst)
    for t in sr.TYPES:
        a = m.small_sample(c["theta"], c["beta"], c["var_par"], on="device", type=t)
        b = m.small_sample(c["theta"], c["beta"], c["var_par"], on="host", type=t)
        assert a["names"] == b["names"] and a["type"] == b["type"] == t
        for k in ("vcov", "dof", "vcov_unadjusted"):
            assert np.allclose(a[k], b[k], rtol=1e-8, atol=1e-10 * np.max(np.abs(b[k]))), (key, t, k)
        assert np.all(a["dof"] > 0)


def test_mcml_fit_with_small_sample():
    """MCML(small_sample="KR") on a family case: the record is there, the coefficient table is the default fit's"""
    d = fd.design("poisson", "log", ncl=6, nt=3, nind=8)
    mod = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], "poisson", "log", d["beta"], d["theta"])
    mod.mcmc_options.update(warmup=20, samps=16)
    fit = mod.MCML(d["y"], max_iter=2, verbose=False, seed=5, small_sample="KR")
    plain = mod.MCML(d["y"], max_iter=2, verbose=False, seed=5)
    P = d["X"].shape[1]
    for k in ("est", "SE", "lower", "upper"):
        assert np.array_equal(fit["coefficients"][k], plain["coefficients"][k], equal_nan=True), k
    assert "small_sample" not in plain and "Small-sample" not in str(plain)
    rec = fit["small_sample"]
    assert rec["type"] == "KR" and rec["vcov"].shape == (P, P) and rec["dof"].shape == (P,)
    assert np.all(rec["dof"] > 0) and np.all(np.isfinite(rec["se"])) and np.all(rec["upper"] > rec["lower"])
    # the model's own query at the fitted parameters gives the record
    th = fit["theta"]
    want = mod.small_sample(th[P:P + 2], th[:P], 1.0, on="device", type="KR")
    assert np.array_equal(rec["vcov"], want["vcov"]) and np.array_equal(rec["dof"], want["dof"])
    assert "Small-sample correction of the fixed effects (KR)" in str(fit)
    la = mod.LA(d["y"], method="nr", small_sample="sat")
    assert la["small_sample"]["type"] == "sat" and np.all(la["small_sample"]["dof"] > 0)
