"""The cases of tests/family_designs.py on the CPU oracle alone: what makes it safe that no case of
tests/test_gpu_beta_step_shapes.py / tests/test_gpu_la_families.py is skipped.

Every beta-step case: model_loglik and every entry of mcnr's outputs finite, eta = xb + Z u inside the link's domain for
every observation and sample column, y inside the family's support, Z taking the branch of z_times the case names, and
the boundaries it claims to cross recomputed from n and m.  Every Laplace case: the three functors and the mcnr_b step
finite, eta inside the domain at each of the points the path evaluates it (xb + Z v for W and the score, xb + ZL v for the
log density and the Newton step's W), the sizes it claims.

The constants the claims are computed with are restated here next to the line of csrc/model.hip each one comes from; the
test reads the source and fails if a statement it quotes is gone."""
import os

import numpy as np
import pytest

import family_designs as fd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# constant -> (value, the statement of csrc/model.hip it restates, its line when this was written)
CONSTANTS = {
    "ROW_BLOCK": (256, "int i = blockIdx.x * 256 + threadIdx.x;", 93),            # k_zgather; k_loglik :356, k_mcnr_row :427
    "COL_LOOP": (256, "for (int j = threadIdx.x; j < n; j += 256)", 401),        # k_mcnr_col; k_mcnr_fin :475
    "MCNR_CHUNK": (16, "constexpr int MCNR_CHUNK = 16;", 419),
    "ROWSUM_UNROLL": (8, "for (; k + 8 <= nchunks; k += 8)", 454),               # k_mcnr_rowsum
    "LOGLIK_GRID_Y": (64, "gy = c.niter < 64 ? c.niter : 64;", 371),              # model_loglik_sum
    "ZGATHER_GRID_Y": (1024, "int gy = ncols < 1024 ? ncols : 1024;", 105),       # z_times
    "Z_WIDTH_MAX": (8, "if (maxrow > 0 && maxrow <= 8 &&", 44),                   # model_setup
}


def test_constants_are_those_of_model_hip():
    with open(os.path.join(ROOT, "glmmrmcml_amd", "csrc", "model.hip")) as f:
        src = f.read()
    for name, (value, statement, _) in CONSTANTS.items():
        assert statement in src, (name, statement)
        assert getattr(fd, name, value) == value, name
    assert (fd.ROW_BLOCK, fd.MCNR_CHUNK, fd.ROWSUM_UNROLL, fd.LOGLIK_GRID_Y, fd.ZGATHER_GRID_Y, fd.Z_WIDTH_MAX) == \
        tuple(CONSTANTS[k][0] for k in ("ROW_BLOCK", "MCNR_CHUNK", "ROWSUM_UNROLL", "LOGLIK_GRID_Y", "ZGATHER_GRID_Y",
                                        "Z_WIDTH_MAX"))


def _reach(n, m):
    """fd.reach restated with the literals above"""
    nchunks = (m + 16 - 1) // 16
    return dict(row_blocks=(n + 255) // 256, chunks=nchunks, last_chunk=m - 16 * (nchunks - 1), unrolled=nchunks // 8,
                tail=nchunks % 8, loglik_stride=m > 64, zgather_stride=m > 1024, ragged_rows=n % 256 != 0)


def test_families_are_the_twelve_of_the_switch(orc):
    assert len(fd.CASES) == 12
    for i, (f, l, vp) in enumerate(fd.CASES):
        assert orc.flink(f, l) == i + 1 == fd.FLINK[(f, l)]
    assert all(vp != 1.0 for f, l, vp in fd.CASES if f in ("gaussian", "gamma", "beta"))


def test_default_sizes_are_those_of_test_gpu_families():
    d = fd.design("poisson", "log")
    assert (d["n"], d["Q"], d["P"]) == (108, 24, 4) and fd.z_branch(d["Z"]) == "gather"
    assert np.array_equal(d["theta"], [0.05, 0.03]) and d["X"].flags.f_contiguous and d["Z"].flags.f_contiguous


# ---------------------------------------------------------------------------------------------- beta-step
@pytest.mark.parametrize("key", list(fd.BETA_CASES))
def test_beta_case_reaches_what_it_claims(key):
    c = fd.BETA_CASES[key]
    for f, l in c["families"]:
        d = fd.beta_design(key, f, l)
        niter = c.get("niter", c["m"])
        assert 0 < niter <= c["m"]
        got = _reach(d["n"], niter)
        assert got == fd.reach(d["n"], niter) == c["reach"], (key, got)
        assert d["X"].shape == (d["n"], d["P"]) and d["Z"].shape == (d["n"], d["Q"]) and d["y"].shape == (d["n"],)
        assert d["P"] == (1 if c.get("intercept_only") else 4)
        assert fd.z_branch(d["Z"]) == ("gemm" if c.get("z") == "dense" else "gather")
        if c.get("z") == "dense":
            assert np.count_nonzero(d["Z"], axis=1).min() >= 9 > fd.Z_WIDTH_MAX
            assert np.abs(d["Z"]).max() <= 0.5


def test_beta_cases_cover_every_boundary():
    """the list as a whole, from the recomputed figures (not from the written claims)"""
    R = {}
    for key, c in fd.BETA_CASES.items():
        f, l = c["families"][0]
        R[key] = _reach(fd.beta_design(key, f, l)["n"], c.get("niter", c["m"]))
    r = R["all_297x150"]
    assert fd.beta_design("all_297x150", "poisson", "log")["n"] == 297 and 297 % 64 != 0 and 297 % 256 == 41
    assert r["row_blocks"] == 2 and (r["chunks"], r["unrolled"], r["tail"], r["last_chunk"]) == (10, 1, 2, 6) and r["loglik_stride"]
    assert len(fd.BETA_CASES["all_297x150"]["families"]) == 12
    assert R["m128"]["unrolled"] == 1 and R["m128"]["tail"] == 0 and R["m128"]["last_chunk"] == 16     # empty tail
    assert R["m129"]["last_chunk"] == 1 and R["m129"]["tail"] == 1                                     # one column, one tail chunk
    assert R["m1"]["chunks"] == 1 and R["m17"]["chunks"] == 2 and R["m17"]["last_chunk"] == 1
    assert R["m65"]["loglik_stride"] and not R["m17"]["loglik_stride"]
    assert R["m150_niter149"]["last_chunk"] == 5 and fd.BETA_CASES["m150_niter149"]["m"] == 150
    assert R["m1030"]["zgather_stride"] and not any(R[k]["zgather_stride"] for k in R if k != "m1030")
    assert R["m1030"]["unrolled"] >= 2 and R["m1030"]["tail"] >= 1
    # a partial last chunk that is not the first one, below and above the eight-at-a-time loop
    assert any(r["chunks"] > 1 and r["last_chunk"] < 16 and r["unrolled"] == 0 for r in R.values())
    assert any(r["chunks"] > 1 and r["last_chunk"] < 16 and r["unrolled"] >= 1 and r["tail"] >= 1 for r in R.values())
    assert [fd.beta_design(k, "poisson", "log")["n"] for k in ("n255", "n256", "n257", "n513")] == [255, 256, 257, 513]
    assert [R[k]["row_blocks"] for k in ("n255", "n256", "n257", "n513")] == [1, 1, 2, 3] and not R["n256"]["ragged_rows"]
    # every sweep has one compile-time instance of dispatch_flink<1, 3, 7> and one run-time family
    for c in fd.BETA_CASES.values():
        fls = {fd.FLINK[fl] for fl in c["families"]}
        assert len(fls) == 1 or (fls & {1, 3, 7} and fls - {1, 3, 7}), fls


@pytest.mark.parametrize("key,family,link", fd.BETA_POINTS, ids=fd.BETA_IDS)
def test_beta_case_is_finite_and_in_domain(orc, key, family, link):
    d = fd.beta_design(key, family, link)
    u, niter, ll, r = fd.beta_reference(key, family, link)
    assert u.shape == (d["Q"], fd.BETA_CASES[key]["m"])
    assert fd.in_support(family, link, d["y"])
    eta = (d["X"] @ d["beta"])[:, None] + d["Z"] @ u
    assert eta.shape == (d["n"], u.shape[1]) and fd.in_domain(family, link, eta)
    c = fd.centre(family, link)
    assert np.abs(eta - c).max() < 0.25, np.abs(eta - c).max()          # |treatment effect 0.05| + |Z u|
    assert np.isfinite(ll)
    for k in ("beta", "XtWX", "XtWr"):
        assert np.isfinite(r[k]).all(), k
    assert np.isfinite(r["sigma"]) and np.isfinite(r["sigma_sum"]) and r["sigma"] > 0
    assert r["sigma_sum"] == pytest.approx(r["sigma"] * niter, rel=1e-12)
    assert np.linalg.cond(r["XtWX"]) < 1e4                               # the step's solve loses no more than 4 digits


@pytest.mark.parametrize("family,link", fd.CACHE_FAMILIES)
def test_cache_samples_are_in_domain(orc, family, link):
    d = fd.beta_design("all_297x150", family, link)
    for m in fd.CACHE_M:
        u = fd.samples(orc, d, m, seed=1 + m)
        eta = (d["X"] @ d["beta"])[:, None] + d["Z"] @ u
        assert fd.in_domain(family, link, eta)
        ll, r = fd.beta_oracle(orc, d, u, beta=d["beta"] * 1.01)
        assert np.isfinite(ll) and np.isfinite(r["beta"]).all()


# ---------------------------------------------------------------------------------------------- Laplace
@pytest.mark.parametrize("key", list(fd.LA_CASES))
def test_la_case_reaches_what_it_claims(key):
    d = fd.la_design(key, "poisson", "log")
    got = dict(n=d["n"], Q=d["Q"], row_blocks=(d["n"] + 255) // 256, q_blocks=(d["Q"] + 255) // 256, q_mod_256=d["Q"] % 256)
    assert got == fd.la_reach(d["n"], d["Q"]) == fd.LA_CASES[key]["reach"], got
    if key == "wide_420x280":
        assert d["n"] > 256 and d["Q"] > 256 and d["Q"] % (4 * 64) != 0 and d["Q"] % 4 == 0


@pytest.mark.parametrize("key,family,link", fd.LA_POINTS, ids=fd.LA_IDS)
def test_la_case_is_finite_and_in_domain(orc, key, family, link):
    d = fd.la_design(key, family, link)
    assert fd.in_support(family, link, d["y"])
    assert d["start"].size == d["P"] + 2 + (family == "gaussian")
    v, vs, beta, theta, vp = fd.la_points(d)
    assert vp == fd.VAR_PAR[(family, link)] and (vp != 1.0 or family in ("poisson", "binomial"))
    L0 = orc.gen_D(d["cov"], d["data"], d["eff_range"], d["theta"], chol=True)
    L1 = orc.gen_D(d["cov"], d["data"], d["eff_range"], theta, chol=True)
    xb0, xb = d["X"] @ d["beta"], d["X"] @ beta
    etas = dict(bv=xb + d["Z"] @ (L0 @ v),                      # kind 0: log density at xb + ZL v
                cov_W=xb0 + d["Z"] @ v, cov_ll=xb0 + d["Z"] @ (L1 @ v),      # kind 1: W at xb + Z v, density with L(theta)
                btheta_W=xb + d["Z"] @ v, btheta_ll=xb + d["Z"] @ (L1 @ v),  # kind 2
                step_W=xb0 + d["Z"] @ (L0 @ vs), step_score=xb0 + d["Z"] @ vs)   # kind 3: update_W(useL), log_grad(usezl = false)
    for k, eta in etas.items():
        assert fd.in_domain(family, link, eta), (k, eta.min(), eta.max())
    ref = fd.la_reference(key, family, link)
    for k in ("bv", "cov", "btheta"):
        assert np.isfinite(ref[k]), k
    st = ref["step"]
    assert np.isfinite(st["v"]).all() and np.isfinite(st["beta"]).all() and np.isfinite(st["sigma"]) and st["sigma"] > 0
    # the Newton step is compared at rtol 1e-8: the reference's two solves must be well conditioned
    m = fd.la_model(d); m.var_par = vp; m.v = vs.copy(); m.update_W(True)
    assert (m.W > 0).all()
    M = m.ZL.T @ (m.W[:, None] * m.ZL) + np.eye(m.Q)
    assert np.linalg.cond(M) < 1e3 and np.linalg.cond(m.X.T @ (m.W[:, None] * m.X)) < 1e4


def test_la_component_case_is_block_structured():
    """the coupling graph of Z (D is diagonal: every block is gr of dimension 1) at the component shape: 6 clusters, each
    one component of its cluster effect and 3 cluster-period effects"""
    d = fd.la_design(fd.LA_COMPONENT_KEY, "poisson", "log")
    assert (d["cov"][:, 1] == 1).all() and (d["cov"][:, 2] == 1).all()
    Q = d["Q"]
    parent = list(range(Q))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for row in d["Z"]:
        nz = np.nonzero(row)[0]
        for j in nz[1:]:
            parent[find(int(j))] = find(int(nz[0]))
    roots = np.array([find(q) for q in range(Q)])
    comps = sorted(set(roots))
    nvars = [int((roots == c).sum()) for c in comps]
    nrows = [int(sum(1 for row in d["Z"] if find(int(np.nonzero(row)[0][0])) == c)) for c in comps]
    assert (len(comps), max(nvars), max(nrows)) == fd.LA_COMPONENT_COUNTS
