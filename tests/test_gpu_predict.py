"""Conditional prediction of the random effects at new points on the device (csrc/predict.hip: Context.predict_re,
api.predict_re, ModelMCML.predict) against the definition.

The reference and the bound are tests/kriging_reference.py's: C D^-1 u and p - C D^-1 C' from the float64 table, solved in
long double, every entry held to C_KRIGE 2^-52 S with S the scale of a Cholesky solve plus the table's own rounding, and
C_KRIGE = 8 x the float64 twins' worst ratio = 0.56, calibrated on these very cases by tests/test_kriging_reference_cpu.py.
Every case is the smallest at which its branch can go wrong; its `why` says which.

Chunked against unchunked (GLMMR_MCML_PREDICT_CHUNK): the large path's solve and product pick their tiles by the number of
columns at hand, so a chunked call is held to the bound, not to the bits of the unchunked one; the diagonal and the small
path do not depend on the chunk and are compared to the bit.

Measured on an MI355X (worst ratios over the cases, in units of 2^-52 S): means 0.0406 (MIXED_m70), cvar 0.0344 (MIXED_m3)
against C_KRIGE = 0.56; the summary mean 0.109 of its bound, sample_var 0.143 of its tolerance (EDGE32); the chunked call
of MIXED equal to the unchunked one to the bit."""
import numpy as np
import pytest

import cov_layouts as cl
import family_designs as fd
import kriging_reference as kr
from glmmrmcml_amd import _lib, api, synth
from glmmrmcml_amd.model import ModelMCML

pytestmark = pytest.mark.gpu
EFF = np.zeros(1)


def context(c):
    ctx = api.Context(*cl.layout(c["blocks"]), EFF)
    ctx.set_u(c["u"])
    return ctx


def check(name, got, ref, m, means=True):
    r = kr.ratios(got, ref, m)
    print("%s: means %.4f, cvar %.4f of C_KRIGE %.2f; summary mean %.4f of 1" % (name, r[0], r[2], kr.C_KRIGE, r[1]))
    assert r[0] <= kr.C_KRIGE and r[2] <= kr.C_KRIGE and r[1] <= 1.0, (name, r)
    if means and m > 1:
        sv = kr.sample_var_check(got, m)[0]
        print("%s: sample_var %.4f of its tolerance" % (name, sv))
        assert sv <= 1.0, (name, sv)
    assert np.all(np.asarray(got["cond_var"]) >= 0)


def run(key, monkeypatch=None):
    c = kr.case(key)
    if c["chunk"] and monkeypatch is not None:
        monkeypatch.setenv("GLMMR_MCML_PREDICT_CHUNK", str(c["chunk"]))      # read per call
    with context(c) as ctx:
        got = ctx.predict_re(c["theta"], c["newdata"], means=True)
        plan = ctx.predict_plan()
    assert got["means"].shape == (c["K"], c["m"]) and all(got[k].shape == (c["K"],) for k in ("mean", "cond_var", "sample_var"))
    check(key, got, kr.reference(key), c["m"])
    assert {k: plan[k] for k in ("diag", "small", "large")} == c["served"], (plan, c["served"])
    assert plan["K"] == c["K"] and plan["m"] == c["m"] and plan["factorisations"] == c["served"]["large"]
    assert plan["chunks"] == kr.chunks_expected(c) and plan["workspace_bytes"] > 0
    return c, got


def matched_levels_are_exact(c, got):
    """a new point that matches a level of a diagonal block: that level's samples to the bit and no variance; one that
    matches none: 0 and the prior variance"""
    ref = kr.reference("MIXED_m3")
    s = r = 0
    for block, xn in zip(c["blocks"], c["newdata"]):
        if xn is not None:
            if cl.kind(block) == "diag":
                row = int(np.flatnonzero((kr._block_columns(block)[0] == xn[0]).all(1))[0])
                assert np.array_equal(got["means"][r], c["u"][s + row]) and got["cond_var"][r] == 0.0
                if len(xn) > 1:
                    assert np.all(got["means"][r + 1] == 0.0) and got["cond_var"][r + 1] == float(ref["prior"][r + 1])
            r += len(xn)
        s += block[0]


# ---------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("key", [k for k in kr.KEYS if kr.case(k)["chunk"] is None])
def test_against_the_reference(key):
    c, got = run(key)
    if key.startswith("MIXED"):
        matched_levels_are_exact(c, got)


def test_chunked_call(monkeypatch):
    c, got = run("MIXED_chunk64", monkeypatch)
    matched_levels_are_exact(c, got)
    monkeypatch.delenv("GLMMR_MCML_PREDICT_CHUNK")
    with context(c) as ctx:
        whole = ctx.predict_re(c["theta"], c["newdata"], means=True)
    ref = kr.reference("MIXED_chunk64")
    same = {k: bool(np.array_equal(got[k], whole[k], equal_nan=True)) for k in got}
    print("chunked against unchunked, equal to the bit:", same)
    for sl, block in zip(ref["block"], [b for b, k in zip(c["blocks"], c["counts"]) if k]):
        if cl.kind(block) != "large":                            # these paths do not depend on the chunk
            assert np.array_equal(got["means"][sl], whole["means"][sl]) and np.array_equal(got["cond_var"][sl], whole["cond_var"][sl])


def test_on_a_context_that_also_samples():
    d = synth.geospatial(150)
    blocks = cl.from_wire(d["cov"], d["data"])
    with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
        ctx.update_L(d["theta"])
        ctx.hmc_sample(d["beta"], d["sigma"], 6, 8, 0.5, 5, 0.9, seed=11, chains=4)
        u = ctx.get_u()
        c = kr.make_case(blocks, d["theta"], [31], u, 150, "one large block of a model context")
        got = ctx.predict_re(d["theta"], c["newdata"], means=True)
        plan = ctx.predict_plan()
        assert np.array_equal(ctx.get_u(), u)
    assert plan["large"] == 1 and plan["m"] == u.shape[1] and plan["K"] == 31
    check("geospatial(150)", got, kr.evaluate(c), c["m"])


# ---------------------------------------------------------------------------------------------- one definition, one set of bits
def test_one_shot_summary_only_and_repeated_calls_return_the_same_bits():
    c = kr.case("MIXED_m70")
    with context(c) as ctx:
        a = ctx.predict_re(c["theta"], c["newdata"], means=True)
        b = ctx.predict_re(c["theta"], c["newdata"], means=True)
        s = ctx.predict_re(c["theta"], c["newdata"])
    with context(c) as ctx2:
        d = ctx2.predict_re(c["theta"], c["newdata"], means=True)
    o = api.predict_re(*cl.layout(c["blocks"]), EFF, c["theta"], c["u"], c["newdata"], means=True)
    for other in (b, d, o):
        assert all(np.array_equal(a[k], other[k], equal_nan=True) for k in a)
    assert set(s) == {"mean", "cond_var", "sample_var"} and all(np.array_equal(a[k], s[k]) for k in s)
    # column 0: the mean of the means in ascending order of the columns
    acc = np.zeros(c["K"])
    for j in range(c["m"]):
        acc = acc + a["means"][:, j]
    tol = 2 * 2.0 ** -52 * np.abs(a["means"]).sum(1) / c["m"]
    assert np.all(np.abs(a["mean"] - acc / c["m"]) <= tol)


def _neighbours(ctx, d, query):
    """a sequence of everything a query must leave alone, with the query in between or not"""
    th = d["theta"]
    nd = [d["data"].reshape(2, -1).T[:40] + 0.01]
    q = (lambda: ctx.predict_re(th * 1.1, nd)) if query else (lambda: None)
    out = []
    ctx.update_L(th)
    ctx.hmc_sample(d["beta"], d["sigma"], 6, 8, 0.5, 5, 0.9, seed=11, chains=4)
    for _ in range(4):                                            # past the two eager evaluations: the captured graph replays
        out.append(ctx.mvn_ll(th)); q()
    v, g = ctx.mvn_ll_grad(th); q()
    out += [v, g]
    out.append(ctx.mvn_ll_batch(np.array([th, th * 1.05, th * 0.95]))); q()
    out.append(ctx.mvn_ll(th * 1.02)); q()
    L, X, dims = ctx.mvn_workspace()
    out += [L, X, np.array(dims)]
    ctx.hmc_sample(d["beta"], d["sigma"], 6, 8, 0.5, 5, 0.9, seed=12, chains=4); q()
    out.append(ctx.get_u())
    la = ctx.mcml_la(d["start"], nr=True, maxiter=1); q()
    out += [la["beta"], la["theta"], la["u"], np.array(la["sigma"])]
    out.append(ctx.information_matrix(d["beta"], d["sigma"], theta=th)); q()
    out.append(ctx.mvn_ll(th))
    return out


def test_the_query_leaves_its_neighbours_their_bits():
    d = synth.geospatial(300)                                     # two full 128 panels and a ragged one: the graphed factorisation
    res = []
    for query in (False, True):
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
            res.append(_neighbours(ctx, d, query))
    assert len(res[0]) == len(res[1])
    for i, (a, b) in enumerate(zip(*res)):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), i


# ---------------------------------------------------------------------------------------------- errors
def _raw(ctx, theta, nnew, flat, K, m, length=None):
    summary = np.full((K, 3), 7.0, order="F")
    means = np.full((K, m), 7.0, order="F")
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    nnew = np.ascontiguousarray(nnew, dtype=np.int32)
    rc = _lib.lib().glmmr_mcml_ctx_predict_re(ctx._h, api._p(theta), api._p(nnew), api._p(flat),
                                              flat.size if length is None else length, api._p(summary), K, api._p(means), K)
    return rc, summary, means


def test_argument_errors():
    c = kr.case("EDGE32")
    cov, data = cl.layout(c["blocks"])
    nnew, flat, K = api._newdata(c["newdata"], cov)
    with api.Context(cov, data, EFF) as ctx:
        assert _raw(ctx, c["theta"], nnew, flat, K, c["m"])[0] == -1                     # no samples set
        assert b"no samples" in _lib.lib().glmmr_mcml_last_error()
        ctx.set_u(c["u"])
        assert _raw(ctx, c["theta"], nnew, flat, K, c["m"], length=flat.size - 1)[0] == -1
        assert _raw(ctx, c["theta"], np.zeros(2, dtype=np.int32), flat, K, c["m"], length=0)[0] == -1     # K = 0
        assert _raw(ctx, c["theta"], np.array([-1, 8], dtype=np.int32), flat, K, c["m"])[0] == -1
        with pytest.raises(_lib.McmlError) as e:
            ctx.predict_re(c["theta"], [None, None])
        assert e.value.code == -1
        with pytest.raises(ValueError):
            ctx.predict_re(c["theta"], c["newdata"][:1])
        rc, summary, means = _raw(ctx, c["theta"], nnew, flat, K, c["m"])
        assert rc == 0 and not np.any(summary[:, :2] == 7.0) and not np.any(means == 7.0)


@pytest.mark.parametrize("key,theta", [("EDGE32", -kr.case("EDGE32")["theta"]),
                                       ("MIXED_m3", np.where(np.arange(10) == cl.MIXED_RHO, 1.5, kr.case("MIXED_m3")["theta"]))],
                         ids=["large-path", "small-path"])
def test_a_block_that_is_not_positive_definite(key, theta):
    """fexp0 with a negative range grows with the distance (the 33 block, factorised by the blocked Cholesky); an AR1
    parameter of 1.5 does the same on the 5 block (factorised in LDS)"""
    c = kr.case(key)
    cov, data = cl.layout(c["blocks"])
    nnew, flat, K = api._newdata(c["newdata"], cov)
    with context(c) as ctx:
        rc, summary, means = _raw(ctx, theta, nnew, flat, K, c["m"])
        assert rc == -3 and b"positive definite" in _lib.lib().glmmr_mcml_last_error()
        assert np.all(summary == 7.0) and np.all(means == 7.0)                           # nothing written
        got = ctx.predict_re(c["theta"], c["newdata"], means=True)                       # and the context still answers
        ll = ctx.mvn_ll(c["theta"])
    check(key + " after the failure", got, kr.reference(key), c["m"])
    assert np.isfinite(ll)


# ---------------------------------------------------------------------------------------------- end to end
def _end_to_end(name, mod, fit, d, newdata):
    dev = mod.predict(fit, newdata, on="device")
    host = mod.predict(fit, newdata, on="host")
    P, R = mod.X.shape[1], mod.cov_parameters.size
    u = np.asarray(fit["re_samps"], float).reshape(mod.Z.shape[1], -1)
    c = kr.make_case(cl.from_wire(d["cov"], d["data"]), fit["theta"][P:P + R], [0 if x is None else len(x) for x in newdata],
                     u, 0, name)
    c["newdata"] = newdata
    ref = kr.evaluate(c)
    for what, p in (("device", dev), ("host", host)):
        got = dict(mean=p["re_mean"], cond_var=p["cond_var"], sample_var=p["sample_var"])
        check("%s %s" % (name, what), got, ref, c["m"], means=False)
    assert set(dev) == set(host)
    if c["m"] > 1:
        assert np.array_equal(dev["re_var"], dev["cond_var"] + dev["sample_var"])
    else:
        assert np.all(np.isnan(dev["sample_var"])) and np.array_equal(dev["re_var"], dev["cond_var"])
    return dev


def test_model_predict_on_a_laplace_fit():
    d = fd.la_design("small_144x24", "poisson", "log")
    mod = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], "poisson", "log", d["beta"], d["theta"])
    fit = mod.LA(d["y"], method="nr")
    blocks = cl.from_wire(d["cov"], d["data"])
    newdata = [None] * len(blocks)
    for b in (0, 3, 7, 23):                                      # a level that matches
        newdata[b] = kr._block_columns(blocks[b])[0][:1].copy()
    newdata[5] = kr._block_columns(blocks[5])[0][:1] + 100.5     # and one that does not
    X = np.tile(d["X"][:1], (5, 1))
    dev = _end_to_end("LA small_144x24", mod, fit, d, newdata)
    lp = mod.predict(fit, newdata, X=X, on="device")["linear_predictor"]
    assert np.array_equal(lp, X @ fit["theta"][:mod.X.shape[1]] + dev["re_mean"])
    assert np.array_equal(dev["re_mean"][[0, 1]], fit["re_samps"][[0, 3], 0]) and dev["re_mean"][2] == 0.0


def test_model_predict_on_an_mcml_fit():
    d = synth.geospatial(150)
    mod = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], "gaussian", "identity", d["beta"], d["theta"],
                    var_par=d["sigma"])
    mod.mcmc_options.update(warmup=20, samps=16)
    fit = mod.MCML(d["y"], max_iter=2, verbose=False, se_method="none", seed=5)
    rng = np.random.default_rng(8)
    xy = d["data"].reshape(2, -1).T
    newdata = [np.vstack([xy[:1], xy[rng.integers(0, 150, 20)] + rng.uniform(-0.03, 0.03, (20, 2))])]
    _end_to_end("MCML geospatial(150)", mod, fit, d, newdata)
