"""The beta-step statistics -- Context.loglik (k_zgather / the GEMM branch of z_times, k_xb, k_loglik) and Context.mcnr
(k_mcnr_col, k_mcnr_row, k_mcnr_rowsum, k_mcnr_fin), csrc/model.hip -- against the oracle past one row block and one
chunk of sample columns, for every family / link case.

The shapes are those of tests/family_designs.py (BETA_CASES names the boundary each one crosses;
tests/test_family_designs_cpu.py recomputes the claims and checks every case finite and in-domain on the oracle alone, so
nothing here is skipped).  u = L V as in tests/test_gpu_families.py.  Tolerances are the project's for these quantities
(tests/test_gpu_families.py, tests/test_gpu_mvn_model.py): the log-likelihood 1e-10 relative, X'WX rtol 1e-11, X'Wr rtol
1e-9 / atol 1e-9, beta rtol 1e-8 / atol 1e-10, sigma (and its sum) 1e-9 relative.  Every one of these is a sum over all
n x m (observation, sample) pairs of terms of one sign or of like size: one pair dropped, duplicated or read from a
neighbouring column moves it by 1 / (n m) ~ 1e-5 relative at the smallest multi-block shape, five orders above the
tolerance.  The column count the statistics carry is read back as sigma_sum / sigma (the step divides by it)."""
import numpy as np
import pytest

import family_designs as fd
from glmmrmcml_amd import api

pytestmark = pytest.mark.gpu


def _ctx(d):
    return api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"])


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _compare(tag, ll, r, llo, ro, niter):
    err = dict(loglik=_rel(ll, llo), XtWX=float(np.abs(r["XtWX"] - ro["XtWX"]).max() / np.abs(ro["XtWX"]).max()),
               XtWr=float(np.abs(r["XtWr"] - ro["XtWr"]).max()), beta=float(np.abs(r["beta"] - ro["beta"]).max()),
               sigma=_rel(r["sigma"], ro["sigma"]), sigma_sum=_rel(r["sigma_sum"], ro["sigma_sum"]),
               count=r["sigma_sum"] / r["sigma"])
    print(tag, " ".join("%s %.3g" % kv for kv in err.items()))
    assert ll == pytest.approx(llo, rel=1e-10), tag
    assert np.allclose(r["XtWX"], ro["XtWX"], rtol=1e-11), tag
    assert np.allclose(r["XtWr"], ro["XtWr"], rtol=1e-9, atol=1e-9), tag
    assert np.allclose(r["beta"], ro["beta"], rtol=1e-8, atol=1e-10), tag
    assert r["sigma"] == pytest.approx(ro["sigma"], rel=1e-9), tag
    assert r["sigma_sum"] == pytest.approx(ro["sigma_sum"], rel=1e-9), tag
    assert r["sigma_sum"] / r["sigma"] == pytest.approx(niter, rel=1e-13), tag      # the column count summed over


@pytest.mark.parametrize("key,family,link", fd.BETA_POINTS, ids=fd.BETA_IDS)
def test_loglik_and_mcnr_match_oracle(key, family, link):
    c = fd.BETA_CASES[key]
    d = fd.beta_design(key, family, link)
    u, niter, llo, ro = fd.beta_reference(key, family, link)
    vp = fd.VAR_PAR[(family, link)]
    with _ctx(d) as ctx:
        assert (ctx.n, ctx.Q, ctx.P) == (d["n"], d["Q"], d["P"])
        ctx.set_u(u, niter=c.get("niter"))
        ll = ctx.loglik(d["beta"], vp)
        r = ctx.mcnr(d["beta"], vp)
        ll2 = ctx.loglik(d["beta"], vp)                 # on the cached ZU, after mcnr reused the partial-sum buffer
    _compare("%s %s-%s" % (key, family, link), ll, r, llo, ro, niter)
    assert ll2 == ll


def _same(a, b, tag):
    (lla, ra), (llb, rb) = a, b
    assert lla == llb, (tag, lla, llb)
    for k in ("beta", "XtWX", "XtWr"):
        assert np.array_equal(ra[k], rb[k]), (tag, k)
    assert ra["sigma"] == rb["sigma"] and ra["sigma_sum"] == rb["sigma_sum"], tag


@pytest.mark.parametrize("family,link", fd.CACHE_FAMILIES)
def test_cached_zu_follows_the_samples(orc, family, link):
    """ZU = Z u is kept until the samples change.  One context sees set_u(u150), set_u(u20) (fewer columns: ZU is
    re-allocated), set_u(u150, niter = 149) and a changed beta on unchanged samples; after each, loglik and mcnr equal
    those of a fresh context given the same inputs, bit for bit.  Then the sampler replaces the samples itself
    (hmc_sample), and the statistics equal the oracle's on get_u()."""
    d = fd.beta_design("all_297x150", family, link)
    vp = fd.VAR_PAR[(family, link)]
    u150 = fd.beta_reference("all_297x150", family, link)[0]
    u20 = fd.samples(orc, d, fd.CACHE_M[1], seed=1 + fd.CACHE_M[1])
    beta2 = d["beta"] * 1.01

    def both(ctx, beta):
        return ctx.loglik(beta, vp), ctx.mcnr(beta, vp)

    def fresh(u, niter, beta):
        with _ctx(d) as c:
            c.set_u(u, niter=niter)
            return both(c, beta)

    with _ctx(d) as ctx:
        seen = {}
        for tag, u, niter, beta in (("u150", u150, None, d["beta"]), ("u20", u20, None, d["beta"]),
                                    ("u150_niter149", u150, 149, d["beta"]), ("beta", None, 149, beta2)):
            if u is not None:
                ctx.set_u(u, niter=niter)
                cur = u
            seen[tag] = both(ctx, beta)
            _same(seen[tag], fresh(cur, niter, beta), tag)
        # the four states differ from one another: a stale ZU, column count or xb would have shown
        lls = [seen[t][0] for t in ("u150", "u20", "u150_niter149", "beta")]
        assert len(set(lls)) == 4, lls
        llo, ro = fd.beta_oracle(orc, d, u150, niter=149, beta=beta2)
        _compare("cache beta %s-%s" % (family, link), seen["beta"][0], seen["beta"][1], llo, ro, 149)
        llo, ro = fd.beta_oracle(orc, d, u20)
        _compare("cache u20 %s-%s" % (family, link), seen["u20"][0], seen["u20"][1], llo, ro, 20)
        ctx.update_L(d["theta"])
        ctx.hmc_sample(d["beta"], vp, 8, 6, 0.2, 5, 0.9, 4242, chains=2, adapt=6)
        us = ctx.get_u()
        assert us.shape == (d["Q"], 6) and np.isfinite(us).all() and np.abs(us).max() > 0
        got = both(ctx, d["beta"])
    llo, ro = fd.beta_oracle(orc, d, us)
    _compare("after hmc_sample %s-%s" % (family, link), got[0], got[1], llo, ro, 6)
