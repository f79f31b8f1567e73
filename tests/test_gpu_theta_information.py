"""The GLS information of the covariance parameters on the device (csrc/theta_info.hip: Context.theta_information,
api.theta_information, ModelMCML.theta_information / MCML(theta_se=) / LA(theta_se=)) against the definition.

The reference is tests/theta_information_reference.py: 1/2 tr(Sigma^-1 d_r Sigma Sigma^-1 d_s Sigma) on the n x n matrices by
long-double Cholesky solves, D being the float64 matrix the device's own gen_D returns and d_r D analytic.  The bound is
normwise against the result,

    max |dev - ref| <= C_TI * 2^-52 * max |ref|,    C_TI = 8 x the float64 twin's worst ratio = 40,

calibrated on these very cases by tests/test_theta_information_reference_cpu.py (the twin's worst ratio 4.452, rounded up to
5).  Measured on an MI355X, ratio to 2^-52 max|ref|: worst 16.5 (family-poisson-log, component operator), then 9.65
(family-gamma-log), 8.31 (family-binomial-logit), 4.25 (wide_41), 3.51 (weak), 2.64 (longitudinal_70x3); the dense cases 0.25
(geo150) to 1.91 (densez_poisson_log), mixed 1.31; the dense operator on a sparse context 0.32 to 5.69 (wide_41), at most 1.44
away from the component operator.  Both operators form B = M^-1 N, not I - M^-1 (reference module, WHICH FORM OF B).
Every case is the smallest at which its branch can go wrong; `why` in the reference module says which branch."""
import numpy as np
import pytest

import family_designs as fd
import theta_information_reference as tr
from glmmrmcml_amd import _lib, api
from glmmrmcml_amd.model import ModelMCML

pytestmark = pytest.mark.gpu
LD = tr.LD


def context(c, y=None):
    y = np.zeros(c["X"].shape[0]) if y is None else y                  # the query does not read y
    return api.Context(c["cov"], c["data"], c["eff_range"], c["Z"], c["X"], y, c["family"], c["link"])


@pytest.fixture(scope="module")
def refs():
    """key -> the long-double reference from the device's D: computed once, shared, read-only"""
    out = {}
    for key in tr.KEYS:
        c = tr.case(key)
        with api.Context(c["cov"], c["data"], c["eff_range"]) as ctx:
            D = ctx.gen_D(c["theta"])
        ref = tr.reference(c, D)
        ref.setflags(write=False)
        out[key] = ref
    return out


def check(key, got, ref, what="device"):
    r = tr.ratio(got, ref)
    print("%s %s: ratio %.3f of C_TI %.1f (max|I| %.3g)" % (key, what, r, tr.C_TI, float(np.max(np.abs(ref)))))
    assert r <= tr.C_TI, (key, what, r)


def query(c, operator=None, ctx=None):
    if ctx is not None:
        return ctx.theta_information(c["beta"], c["var_par"], c["theta"], operator=operator)
    with context(c) as own:
        return own.theta_information(c["beta"], c["var_par"], c["theta"], operator=operator)


def run(key, refs, operator=None):
    """the query on a fresh context -> (matrix, plan); checked against the reference"""
    c = tr.case(key)
    with context(c) as ctx:
        r = query(c, operator, ctx)
        plan = ctx.theta_information_plan()
    got = r["information"]
    assert got.shape == (tr.rows(c),) * 2 and np.all(np.isfinite(got)) and r["names"] == tr.names(c)
    assert np.array_equal(got, got.T)
    check(key, got, refs[key])
    assert plan["R"] == c["theta"].size and plan["rows"] == tr.rows(c)
    return got, plan


# ---------------------------------------------------------------------------------------------- the two operators
@pytest.mark.parametrize("key", tr.COMPONENT_KEYS)
def test_component_path(key, refs):
    got, plan = run(key, refs)
    assert plan["requested"] == 0 and plan["op"] == 1 and plan["dense_bytes"] == 0 and plan["launches"] == 2
    assert (plan["ncomp"], plan["max_vars"]) == tr.case(key)["comps"]


@pytest.mark.parametrize("key", tr.DENSE_KEYS)
def test_dense_path(key, refs):
    got, plan = run(key, refs)
    assert plan["requested"] == 0 and plan["op"] == 0 and plan["dense_bytes"] > 0 and plan["launches"] > 0
    comps = tr.case(key)["comps"]
    if comps is not None:                                               # a sparse context whose plan does not qualify
        assert (plan["ncomp"], plan["max_vars"]) == comps


@pytest.mark.parametrize("key", ["stepped_wedge_7x8x3", "family-gaussian-identity", "wide_41"])
def test_dense_operator_on_a_sparse_context(key, refs):
    c = tr.case(key)
    comp, _ = run(key, refs)
    with context(c) as ctx:
        dense = query(c, "dense", ctx)["information"]
        plan = ctx.theta_information_plan()
        assert plan["requested"] == 1 and plan["op"] == 0 and plan["dense_bytes"] > 0
        check(key, dense, refs[key], "dense operator")
        # both lie within the bound of the definition: of each other within twice that
        diff = float(np.max(np.abs(dense - comp)) / (tr.EPS * float(np.max(np.abs(refs[key])))))
        print("%s dense against component: %.3f of %.1f" % (key, diff, 2 * tr.C_TI))
        assert diff <= 2 * tr.C_TI
        again = query(c, None, ctx)["information"]                     # the context's operator is still the sparse one
        assert ctx.theta_information_plan()["op"] == 1 and np.array_equal(again, comp)
        assert ctx.sparse_plan(1)["active"]


# ---------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("key", ["geo300", "stepped_wedge_7x8x3", "mixed"])
def test_bits(key):
    """symmetric to the bit; two calls and two contexts give the same bits"""
    c = tr.case(key)
    with context(c) as ctx:
        a = query(c, None, ctx)["information"]
        b = query(c, None, ctx)["information"]
    d = query(c)["information"]
    assert np.array_equal(a, a.T)
    assert np.array_equal(a, b) and np.array_equal(a, d)


def test_the_query_leaves_a_laplace_fit_its_bits():
    c = tr.case("stepped_wedge_7x8x3")

    def fit(with_query):
        with context(c, c["y"]) as ctx:
            ctx.update_L(c["theta"])
            if with_query:
                query(c, None, ctx)
                ctx.theta_information(c["beta"] * 0.5, c["var_par"], c["theta"] * 1.1, operator="dense")
                ctx.update_L(c["theta"])
            return ctx.mcml_la(c["start"], nr=True, maxiter=1)

    a, b = fit(True), fit(False)
    for k in ("beta", "theta", "u"):
        assert np.array_equal(a[k], b[k]), k
    assert a["sigma"] == b["sigma"] and a["iters"] == b["iters"]


def test_the_query_leaves_mvn_ll_the_sampler_and_the_information_query_their_bits():
    c = tr.case("geo300")
    u = np.random.default_rng(3).standard_normal((300, 3)) * 0.3

    def values(with_query):
        with context(c, c["y"]) as ctx:
            ctx.update_L(c["theta"])
            ctx.set_u(u)
            if with_query:
                query(c, None, ctx)                                     # leaves the context as update_L(theta) leaves it
            ll = ctx.mvn_ll(c["theta"])
            ctx.hmc_sample(c["beta"], c["var_par"], 3, 4, 0.5, 5, 0.9, seed=11, chains=2)
            return ll, ctx.get_u(), ctx.information_matrix(c["beta"], c["var_par"])

    (la, ua, ia), (lb, ub, ib) = values(True), values(False)
    assert la == lb and np.array_equal(ua, ub) and np.array_equal(ia, ib)


# ---------------------------------------------------------------------------------------------- refusals
def test_theta_is_required():
    c = tr.case("family-poisson-log")
    with context(c) as ctx:
        ctx.update_L(c["theta"])
        with pytest.raises(_lib.McmlError) as e:
            ctx.theta_information(c["beta"], c["var_par"], None)
        assert e.value.code == -1 and "theta" in str(e.value)


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
                ctx.theta_information(beta, c["var_par"], c["theta"], operator=operator)
            assert e.value.code == -1 and "weight" in str(e.value)
            good = query(c, operator, ctx)["information"]               # the context is usable afterwards
            assert np.all(np.isfinite(good)) and good.shape == (2, 2)


@pytest.mark.parametrize("key", ["geo150", "comp65", "split_block"])
def test_component_operator_where_it_does_not_apply(key):
    c = tr.case(key)
    with context(c) as ctx:
        with pytest.raises(_lib.McmlError) as e:
            query(c, "component", ctx)
        assert e.value.code == -2
        with pytest.raises(KeyError):
            query(c, "component_wide", ctx)


def test_a_theta_that_makes_D_not_positive_definite():
    """ar1 with rho = 1.5: the leading 2 x 2 minor of every block is t^4 (1 - 2.25) < 0"""
    c = tr.case("stepped_wedge_7x8x3")
    theta = np.array([c["theta"][0], 1.5])
    with context(c) as ctx:
        with pytest.raises(_lib.McmlError) as e:
            ctx.theta_information(c["beta"], c["var_par"], theta)
        assert e.value.code == -3
        good = query(c, None, ctx)["information"]                       # and the context recovers
        assert np.all(np.isfinite(good))


def test_one_shot_export_equals_the_context_query():
    for key in ("family-gamma-log", "geo150"):
        c = tr.case(key)
        want = query(c)
        got = api.theta_information(c["cov"], c["data"], c["eff_range"], c["Z"], c["X"], c["family"], c["link"], c["beta"],
                                    c["theta"], var_par=c["var_par"])
        assert np.array_equal(got["information"], want["information"]) and got["names"] == want["names"]


# ---------------------------------------------------------------------------------------------- end to end
def test_la_fit_with_theta_se():
    """LA(theta_se="device") against theta_se="host": the same estimates to the bit; the standard errors
    sqrt(diag(inv(I))) agree within what the bound on I allows.  Propagation as in test_gpu_information.py: the device and the
    host formula both lie within b = C_TI eps max|I| of the definition, so they differ by at most 2 b entrywise;
    inv(I + E) - inv(I) = -inv(I) E inv(I) to first order, on the diagonal at most 2 b (sum_j |inv_ij|)^2; d sqrt(v) =
    dv / (2 sqrt(v)); numpy's own inverse adds at most R eps kappa_2(I) max|inv| on either side (Higham, 14.1)."""
    d = fd.la_design("small_144x24", "poisson", "log")
    m = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["family"], d["link"], d["beta"], d["theta"])
    f0 = m.LA(d["y"], method="nr")
    fh = m.LA(d["y"], method="nr", theta_se="host")
    fdv = m.LA(d["y"], method="nr", theta_se="device")
    P, R = d["P"], 2
    for f in (fh, fdv):
        assert np.array_equal(f0["theta"], f["theta"])
        assert np.array_equal(f0["coefficients"]["est"], f["coefficients"]["est"])
        assert np.array_equal(f0["coefficients"]["SE"][:P], f["coefficients"]["SE"][:P])       # the beta column is untouched
    assert np.all(np.isnan(f0["coefficients"]["SE"][P:P + R])) and "theta_information" not in f0
    I = fh["theta_information"]["information"]
    assert I.shape == (R, R) and fdv["theta_information"]["names"] == fh["theta_information"]["names"]
    b = tr.C_TI * tr.EPS * np.max(np.abs(I))
    inv = np.linalg.inv(I)
    se = np.sqrt(np.diag(inv))
    tol = (2 * b * np.abs(inv).sum(1) ** 2 + 2 * R * tr.EPS * np.linalg.cond(I) * np.abs(inv).max()) / (2 * se)
    got_h, got_d = fh["coefficients"]["SE"][P:P + R], fdv["coefficients"]["SE"][P:P + R]
    print("SE host %s\nSE device %s\ntolerance %s" % (got_h, got_d, tol))
    assert np.all(np.isfinite(got_d)) and np.all(got_d > 0) and np.all(np.abs(got_h - got_d) <= tol)
