"""The GLS information matrix on the device (csrc/info.hip: Context.information_matrix, api.information_matrix,
ModelMCML(..., information="device")) against the definition.

The reference is tests/information_reference.py: X' (diag(w) + Z D Z')^-1 X by a long-double Cholesky solve, D being the float64
matrix the device's own gen_D returns (what the host formula downloads).  The bound is normwise against X'VX, not against the
result -- the Woodbury form X'VX - S'S cancels --

    max |dev - ref| <= C_INFO * 2^-52 * max |X'VX|,    C_INFO = 8 x the float64 twin's worst ratio = 20

calibrated on these very cases by tests/test_information_reference_cpu.py (measured on an MI355X: worst ratio 2.56 against the
long-double reference, wide_41; 4.70 against the host formula, wide_41_p71).  The host formula (ModelMCML.information_matrix) is the
second reference, with the same bound.  Every case is the smallest at which its branch can go wrong; `why` in the helper says
which branch."""
import numpy as np
import pytest

import family_designs as fd
import information_reference as ir
from glmmrmcml_amd import _lib, api
from glmmrmcml_amd.model import ModelMCML

pytestmark = pytest.mark.gpu
LD = ir.LD


def context(c, y=None):
    y = np.zeros(c["X"].shape[0]) if y is None else y                  # the query does not read y
    return api.Context(c["cov"], c["data"], c["eff_range"], c["Z"], c["X"], y, c["family"], c["link"])


@pytest.fixture(scope="module")
def refs():
    """key -> the long-double reference from the device's D: computed once, shared, read-only"""
    out = {}
    for key in ir.KEYS:
        c = ir.case(key)
        with api.Context(c["cov"], c["data"], c["eff_range"]) as ctx:
            D = ctx.gen_D(c["theta"])
        ref = ir.reference(c, D)
        ref.setflags(write=False)
        out[key] = ref
    return out


def host(c):
    m = ModelMCML(c["cov"], c["data"], c["eff_range"], c["Z"], c["X"], ir.model_family(c["family"]), c["link"], c["beta"],
                  c["theta"], var_par=c["var_par"])
    return m.information_matrix(c["theta"], c["beta"], c["var_par"])


def check(key, got, ref, what="device"):
    c = ir.case(key)
    r = ir.ratio(got, ref, c)
    print("%s %s: ratio %.3f of C_INFO %.1f (max|X'VX| %.3g, max|info| %.3g)" % (key, what, r, ir.C_INFO, ir.xtvx_max(c),
                                                                               float(np.max(np.abs(ref)))))
    assert r <= ir.C_INFO, (key, what, r)


def run(key, refs, operator=None, against_host=True):
    """the query on a fresh context with theta given -> (matrix, plan); checked against both references"""
    c = ir.case(key)
    with context(c) as ctx:
        got = ctx.information_matrix(c["beta"], c["var_par"], theta=c["theta"], operator=operator)
        plan = ctx.information_plan()
    assert got.shape == (c["X"].shape[1],) * 2 and np.all(np.isfinite(got))
    assert np.array_equal(got, got.T)
    check(key, got, refs[key])
    if against_host:
        check(key, got, host(c).astype(LD), "device against the host formula")
    assert plan["P"] == c["X"].shape[1]
    return got, plan


# ---------------------------------------------------------------------------------------------- the three operators
@pytest.mark.parametrize("key", ir.FAMILY_KEYS)
def test_component_path_on_every_family_and_link(key, refs):
    got, plan = run(key, refs)
    assert plan["op"] == 1 and plan["dense_bytes"] == 0 and plan["requested"] == 0
    assert (plan["ncomp"], plan["max_vars"]) == (6, 4) and plan["launches"] == 2


@pytest.mark.parametrize("key", ir.COMPONENT_KEYS)
def test_component_path_packs_components_into_a_wave(key, refs):
    got, plan = run(key, refs)
    assert plan["op"] == 1 and plan["dense_bytes"] == 0
    assert (plan["ncomp"], plan["max_vars"]) == {"longitudinal_70x3": (70, 4), "stepped_wedge_7x8x3": (7, 8)}[key]


@pytest.mark.parametrize("waves", ["1", "4"])
def test_component_path_under_both_forms_of_the_factor_kernel(waves, refs, monkeypatch):
    monkeypatch.setenv("GLMMR_MCML_LA_WAVES", waves)                   # read per call
    got, plan = run("stepped_wedge_7x8x3", refs, against_host=False)
    assert plan["op"] == 1 and plan["waves"] == int(waves)


@pytest.mark.parametrize("waves", ["1", "4"])
@pytest.mark.parametrize("key", ir.WIDE_KEYS)
def test_component_wide_path(key, waves, refs, monkeypatch):
    """41 variables per component: a wave per component in the solve, the workgroup form of the factor kernel whatever the
    variable says; P = 71 runs a second column chunk of 7"""
    monkeypatch.setenv("GLMMR_MCML_LA_WAVES", waves)
    got, plan = run(key, refs, against_host=(waves == "4"))
    assert plan["op"] == 2 and plan["dense_bytes"] == 0 and plan["waves"] == 4
    assert (plan["ncomp"], plan["max_vars"]) == (3, 41)


@pytest.mark.parametrize("key", ir.DENSE_KEYS)
def test_dense_path(key, refs):
    got, plan = run(key, refs)
    assert plan["op"] == 0 and plan["dense_bytes"] > 0 and plan["launches"] == 0


def test_a_component_above_the_cap_takes_the_dense_path(refs):
    got, plan = run("comp129", refs)
    assert plan["op"] == 0 and plan["max_vars"] == 129 and plan["requested"] == 0


def test_dense_operator_on_a_sparse_context(refs):
    key = "stepped_wedge_7x8x3"
    c = ir.case(key)
    comp, _ = run(key, refs, against_host=False)
    with context(c) as ctx:
        dense = ctx.information_matrix(c["beta"], c["var_par"], theta=c["theta"], operator="dense")
        plan = ctx.information_plan()
        assert plan["requested"] == 1 and plan["op"] == 0 and plan["dense_bytes"] > 0
        check(key, dense, refs[key], "dense operator")
        check(key, dense, comp.astype(LD), "dense against component")
        # the context's operator is still the sparse one
        again = ctx.information_matrix(c["beta"], c["var_par"])
        assert ctx.information_plan()["op"] == 1 and np.array_equal(again, comp)
        assert ctx.sparse_plan(1)["active"]


def test_component_operator_where_it_does_not_apply():
    c = ir.case("geo150_p1")
    with context(c) as ctx:
        ctx.update_L(c["theta"])
        with pytest.raises(_lib.McmlError) as e:
            ctx.information_matrix(c["beta"], c["var_par"], operator="component")
        assert e.value.code == -2
        with pytest.raises(KeyError):
            ctx.information_matrix(c["beta"], c["var_par"], operator="component_wide")
    c = ir.case("comp129")
    with context(c) as ctx:
        with pytest.raises(_lib.McmlError) as e:
            ctx.information_matrix(c["beta"], c["var_par"], theta=c["theta"], operator="component")
        assert e.value.code == -2


def test_no_L_is_refused():
    c = ir.case("family-poisson-log")
    with context(c) as ctx:
        with pytest.raises(_lib.McmlError) as e:
            ctx.information_matrix(c["beta"], c["var_par"])
        assert e.value.code == -1


def test_one_shot_export_equals_the_context_query():
    c = ir.case("family-gamma-log")
    with context(c) as ctx:
        want = ctx.information_matrix(c["beta"], c["var_par"], theta=c["theta"])
    got = api.information_matrix(c["cov"], c["data"], c["eff_range"], c["Z"], c["X"], c["family"], c["link"], c["beta"],
                                 c["theta"], var_par=c["var_par"])
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("key", ["geo300_p3", "stepped_wedge_7x8x3"])
def test_bits(key):
    """symmetric to the bit; two calls and two contexts give the same bits; theta=None after update_L(theta) = theta given"""
    c = ir.case(key)
    with context(c) as ctx:
        a = ctx.information_matrix(c["beta"], c["var_par"], theta=c["theta"])
        b = ctx.information_matrix(c["beta"], c["var_par"], theta=c["theta"])
    with context(c) as ctx:
        ctx.update_L(c["theta"])
        d = ctx.information_matrix(c["beta"], c["var_par"])
        e = ctx.information_matrix(c["beta"], c["var_par"])
    assert np.array_equal(a, a.T)
    assert np.array_equal(a, b) and np.array_equal(a, d) and np.array_equal(a, e)


def test_the_query_leaves_a_laplace_fit_its_bits():
    c = ir.case("stepped_wedge_7x8x3")

    def fit(query):
        with context(c, c["y"]) as ctx:
            ctx.update_L(c["theta"])
            if query:
                ctx.information_matrix(c["beta"], c["var_par"])
                ctx.information_matrix(c["beta"] * 0.5, c["var_par"], theta=c["theta"] * 1.1, operator="dense")
                ctx.update_L(c["theta"])
            return ctx.mcml_la(c["start"], nr=True, maxiter=1)

    a, b = fit(True), fit(False)
    for k in ("beta", "theta", "u"):
        assert np.array_equal(a[k], b[k]), k
    assert a["sigma"] == b["sigma"] and a["iters"] == b["iters"]


def test_the_query_leaves_mvn_ll_and_the_sampler_their_bits():
    c = ir.case("geo300_p3")
    u = np.random.default_rng(3).standard_normal((300, 3)) * 0.3

    def values(query):
        with context(c, c["y"]) as ctx:
            ctx.update_L(c["theta"])
            ctx.set_u(u)
            if query:
                ctx.information_matrix(c["beta"], c["var_par"])
            ll = ctx.mvn_ll(c["theta"])
            ctx.hmc_sample(c["beta"], c["var_par"], 3, 4, 0.5, 5, 0.9, seed=11, chains=2)
            return ll, ctx.get_u()

    (la, ua), (lb, ub) = values(True), values(False)
    assert la == lb and np.array_equal(ua, ub)


def test_a_weight_that_is_not_finite_raises():
    """gamma / inverse: dhdmu = 1 / eta^2; beta[1] = 0 puts the linear predictor of the first period's control rows at 0"""
    c = dict(ir.case("family-gamma-inverse"))
    beta = c["beta"].copy()
    beta[1] = 0.0
    assert np.any(c["X"] @ beta == 0.0)
    for operator in (None, "dense"):
        with context(c) as ctx:
            with pytest.raises(_lib.McmlError) as e:
                ctx.information_matrix(beta, c["var_par"], theta=c["theta"], operator=operator)
            assert e.value.code == -1 and "weight" in str(e.value)
            good = ctx.information_matrix(c["beta"], c["var_par"], operator=operator)      # the context is usable afterwards
            assert np.all(np.isfinite(good))


# ---------------------------------------------------------------------------------------------- end to end
def test_la_fit_with_device_information():
    """LA(information="device") against information="host": the same estimates to the bit; SE[:P] = sqrt(diag(inv(M))) agree
    within what the bound on M allows.  Propagation: both matrices lie within b = C_INFO eps max|X'VX| of the definition, so
    they differ by at most 2 b entrywise; inv(M + E) - inv(M) = -inv(M) E inv(M) to first order (the second-order term is
    O(b^2 |inv|^3), 1e-13 of the first here), entrywise on the diagonal at most 2 b (sum_j |inv_ij|)^2 = ||inv|| b ||inv||
    row-wise; d sqrt(v) = dv / (2 sqrt(v)).  numpy's own inverse adds its forward error, at most P eps kappa_2(M) max|inv| on
    either side (Higham, Accuracy and Stability, 14.1)."""
    d = fd.la_design("small_144x24", "poisson", "log")
    m = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["family"], d["link"], d["beta"], d["theta"])
    fh = m.LA(d["y"], method="nr", information="host")
    fdv = m.LA(d["y"], method="nr", information="device")
    assert np.array_equal(fh["theta"], fdv["theta"])
    assert np.array_equal(fh["coefficients"]["est"], fdv["coefficients"]["est"])
    P = d["P"]
    est = fh["theta"]
    c = dict(X=m.X, Z=m.Z, family=d["family"], link=d["link"], beta=est[:P], var_par=1.0)
    b = ir.bound(c)
    M = m.information_matrix(est[P:P + 2], est[:P], 1.0)
    inv = np.linalg.inv(M)
    se = np.sqrt(np.diag(inv))
    tol = (2 * b * np.abs(inv).sum(1) ** 2 + 2 * P * ir.EPS * np.linalg.cond(M) * np.abs(inv).max()) / (2 * se)
    got_h, got_d = fh["coefficients"]["SE"][:P], fdv["coefficients"]["SE"][:P]
    print("SE host %s\nSE device %s\ntolerance %s" % (got_h, got_d, tol))
    assert np.all(np.isfinite(got_d)) and np.all(np.abs(got_h - got_d) <= tol)
    assert np.all(np.isnan(fdv["coefficients"]["SE"][P:P + 2]))
