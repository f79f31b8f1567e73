"""The sampler's two products per leapfrog step on the SPARSE chain-major operator (csrc/hmc_cm.h: the ELL / CSR pair of
ZL, or the two factors Z and L applied in turn), against the CPU oracle: log_prob / log_grad of all 12 family / link
cases and chains compared one by one, on every form -- k_cm_forward with both of its metadata loads, k_cm_backward
(short rows), k_cm_backward_long, k_cm_Lrow / k_cm_Lcol and the fused k_cm_Lcol_Lrow<8> / <16> -- at more than one
64-chain group and at the row-shape edges of each kernel.  Every case asserts the form it means through
ctx.sparse_plan() (which reports the decisions of csrc/sparse_plan.h that hmc.hip launches by), besides
ctx.last_kernels() == ("sparse", "sparse").

Tolerances are those of test_gpu_dense_products: log_prob / log_grad 1e-10 relative; chains: identical accept flags,
probabilities within 1e-9, samples within 1e-8 relative.  Identical flags need every compared proposal's acceptance
probability to sit away from its uniform draw: the oracle hands the draws back and |u - prob| >= 1e-6 is asserted for
every compared chain and proposal.  A chain's draws depend on (seed, global chain id) only, so at 130 chains (three
groups, the last holding two chains) the edges of every group are compared."""
import numpy as np
import pytest

from glmmrmcml_amd import api, synth
from test_gpu_dense_products import (ADAPT, CASES, CHAIN_CASES, IT, LAM, MS, SEED, TA, WARM, _oracle_model, _y,
                                     oracle_L, run_chains)
from test_gpu_dense_products import check_log_prob_grad as dense_check_log_prob_grad

gpu = pytest.mark.gpu             # every test but test_design_shapes, which checks the designs on the CPU

GROUP_EDGES = [0, 63, 64, 127, 128, 129]         # of 130 chains
MARGIN = 1e-6

# kind -> (generator, sizes, theta).  theta is small so that eta stays inside every link's domain.
KINDS = {
    "rct": (synth.cluster_rct, dict(ncl=7, nt=5, nind=3), (0.1, 0.07)),          # n = 105 (odd), Q = 42, blocks of 1
    "sw_short": (synth.stepped_wedge, dict(ncl=6, nt=5, nind=3), (0.1, 0.8)),    # n = 90, Q = 30, 3 observations per effect
    "sw_long": (synth.stepped_wedge, dict(ncl=7, nt=5, nind=40), (0.1, 0.8)),    # n = 1400, nnz(Z) = 40 Q, nnz(ZL) = 120 Q
    "sw_blk8": (synth.stepped_wedge, dict(ncl=5, nt=8, nind=3), (0.1, 0.8)),
    "sw_blk12": (synth.stepped_wedge, dict(ncl=5, nt=12, nind=2), (0.1, 0.8)),
    "sw_blk16": (synth.stepped_wedge, dict(ncl=5, nt=16, nind=2), (0.1, 0.8)),
    "sw_blk17": (synth.stepped_wedge, dict(ncl=5, nt=17, nind=2), (0.1, 0.8)),
    "long_wide": (synth.longitudinal, dict(nsubj=410, nvisit=9), (0.1, 0.07)),   # Q = 4100 > 4096, n = 3690
    "tiny": (synth.cluster_rct, dict(ncl=3, nt=2, nind=3), (0.1, 0.07)),         # n = 18, Q = 9
}

# random effects whose observations are removed: a cluster's last period (an empty row of ZL' and of Z') and a middle
# one (an empty row of Z' only)
DROP = {"sw_short": (9, 17), "sw_long": (9, 17)}
# effect -> observations kept, for a long-row design with ragged rows: rows of Z' of 39 (4k + 3), 37 (4k + 1), 2 and 1
# entries; the effects kept at 1 and 2 are last periods of their clusters, so ZL' has these two rows as well
RAGGED = {3: 39, 7: 37, 14: 1, 24: 2}


def _centre(family, link):
    centre = {"log": 0.3, "identity": 0.5, "logit": 0.2, "probit": 0.1, "inverse": 1.5}[link]
    if family == "binomial" and link == "log":
        centre = -1.0
    if family == "poisson" and link == "identity":
        centre = 3.0
    if family == "gamma" and link == "identity":
        centre = 2.0
    if family == "gaussian" and link == "log":
        centre = 1.5
    return centre


def design(kind, family, link, slope=False, drop=(), ragged=None, seed=5):
    """cov / data / Z of a synth design at a small size, with the mean replaced by X = 1, beta = [centre(link)] and y
    drawn for the family (as test_gpu_dense_products.design).
    slope: every nonzero of Z is multiplied by a per-observation covariate in [0.5, 1.5] (a random slope);
    drop:  random effects whose observations are removed -- the effect stays in cov (a cluster-period with no data);
    ragged: {effect: observations kept}: single observations removed, so that rows of Z' / ZL' get odd lengths"""
    gen, kw, theta = KINDS[kind]
    s = gen(**kw)
    Z = np.array(s["Z"], order="F")
    if drop:
        keep = ~(Z[:, list(drop)] != 0).any(axis=1)
        Z = np.asfortranarray(Z[keep])
    if ragged:
        keep = np.ones(Z.shape[0], dtype=bool)
        for q, k in ragged.items():
            keep[np.nonzero(Z[:, q])[0][k:]] = False
        Z = np.asfortranarray(Z[keep])
    n, Q = Z.shape
    if slope:
        x = 0.5 + np.random.default_rng(seed + 77).random(n)
        Z = np.asfortranarray(Z * x[:, None])
    centre = _centre(family, link)
    yrng = np.random.default_rng(seed + 1000 + 17 * CASES.index(next(c for c in CASES if c[:2] == (family, link))))
    y = _y(family, link, np.full(n, centre), yrng)
    cov = s["cov"]
    dims, seen = [], set()
    for r in cov:
        if int(r[0]) not in seen:
            seen.add(int(r[0])); dims.append(int(r[1]))
    assert sum(dims) == Q
    return dict(cov=cov, data=s["data"], eff_range=s["eff_range"], Z=Z, X=np.ones((n, 1), order="F"), y=y, family=family,
                link=link, beta=np.array([centre]), theta=np.array(theta), n=n, Q=Q, dims=dims, kind=kind, zkind=kind,
                seed=("sparse", kind))          # key of test_gpu_dense_products.oracle_L's cache: L depends on cov and theta


def structure(d):
    """nnz(Z), nnz(L), nnz(ZL), the ELL width of ZL and the row lengths of ZL' and Z', from Z and the block sizes"""
    start = np.repeat(np.cumsum([0] + d["dims"][:-1]), d["dims"])
    nzr, nzc = np.nonzero(d["Z"])
    width = np.zeros(d["n"], dtype=int)
    rows_zl = np.zeros(d["Q"], dtype=int)
    for i, j in zip(nzr, nzc):
        width[i] += j - start[j] + 1
        rows_zl[start[j]:j + 1] += 1
    return dict(nnz_z=int(nzr.size), nnz_l=int(sum(b * (b + 1) // 2 for b in d["dims"])), nnz=int(width.sum()),
                W=int(width.max()), rows_zl=rows_zl, rows_z=np.bincount(nzc, minlength=d["Q"]))


def context(d, monkeypatch, form, lfuse=None):
    """form: "product" / "factored" (GLMMR_MCML_ZL, read when the operator is set up) or None for the heuristic;
    lfuse: "0" for the separate k_cm_Lcol / k_cm_Lrow (GLMMR_MCML_CM_LFUSE, read per call)"""
    if lfuse is None:
        monkeypatch.delenv("GLMMR_MCML_CM_LFUSE", raising=False)
    else:
        monkeypatch.setenv("GLMMR_MCML_CM_LFUSE", lfuse)
    if form is None:
        monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    else:
        monkeypatch.setenv("GLMMR_MCML_ZL", form)
    ctx = api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"])
    ctx.update_L(d["theta"])
    return ctx


def assert_plan(ctx, d, C, **expect):
    """the operator ran sparse, in the form the case means; the hook's counts are those of Z and the blocks"""
    assert ctx.last_kernels() == ("sparse", "sparse"), ctx.last_kernels()
    assert ctx.profile(enable=False)["operator"] == "sparse"
    p = ctx.sparse_plan(C)
    st = structure(d)
    assert p["active"] and p["ncb"] == -(-C // 64), p
    for k in ("nnz", "nnz_z", "nnz_l", "W"):
        assert p[k] == st[k], (k, p, st[k])
    assert p["nblk"] == len(d["dims"]) and p["max_blk"] == max(d["dims"]), p
    assert p["qrows"] == (16 if d["Q"] <= 4096 else 64), p
    assert p["long_rows"] == ((p["nnz_z"] if p["factored"] else p["nnz"]) >= 24 * d["Q"]), p
    for k, v in expect.items():
        assert p[k] == v, (k, v, p)
    return p


def _vp(d):
    return next(c[2] for c in CASES if c[:2] == (d["family"], d["link"]))


def check_log_prob_grad(orc, d, lp, G, V, cols=None, L=None):
    """test_gpu_dense_products.check_log_prob_grad; L: the factor of D where it is not the oracle's dense Cholesky"""
    if L is None:
        return dense_check_log_prob_grad(orc, d, lp, G, V, cols)
    ZL, xb, yo, fl = _oracle_model(orc, d, L)
    vp = _vp(d)
    for c in (range(V.shape[1]) if cols is None else cols):
        lo = orc.log_prob(xb, ZL, yo, vp, fl, V[:, c])
        go = orc.log_grad(xb, ZL, yo, vp, fl, V[:, c])
        assert np.isfinite(lo) and np.all(np.isfinite(go)), (d["family"], d["link"], c)
        assert abs(lp[c] - lo) <= 1e-10 * abs(lo), (d["family"], d["link"], c, lp[c], lo)
        assert np.abs(G[:, c] - go).max() <= 1e-10 * max(1.0, np.abs(go).max()), (d["family"], d["link"], c)


def oracle_chain(orc, d, c, nsamp=1, seed=SEED, L=None):
    """chain c on the oracle (whitened samples Q x (nsamp + 1), flags, probabilities), its accept margins asserted"""
    Lo = oracle_L(orc, d) if L is None else L
    ZL, xb, yo, fl = _oracle_model(orc, d, Lo)
    so, fo, po, dg = orc.hmc_chain(xb, ZL, yo, _vp(d), fl, WARM, nsamp, LAM, MS, TA, seed, chain_id=c, iter_idx=IT,
                                   adapt=ADAPT)
    assert np.all(np.isfinite(so)) and np.all(np.isfinite(po)), (d["kind"], d["family"], d["link"], c)
    gap = np.abs(dg["unif"] - po).min()
    assert gap >= MARGIN, (d["kind"], d["family"], d["link"], c, gap)
    return Lo, so, fo, po


def check_chains(orc, d, u, flags, probs, chains, nsamp=None, per_chain=1, seed=SEED, L=None):
    """test_gpu_dense_products.check_chains with the oracle's accept margins asserted.  u holds per_chain draws per
    chain, chain-major (C > 1), or the single chain's Q x (nsamp + 1)"""
    for c in chains:
        Lo, so, fo, po = oracle_chain(orc, d, c, nsamp or per_chain, seed, L)
        assert np.array_equal(flags[c], fo), (d["kind"], d["family"], d["link"], c, flags[c], fo, probs[c], po)
        assert np.abs(probs[c] - po).max() < 1e-9, (d["kind"], d["family"], d["link"], c)
        uo = Lo @ (so if nsamp else so[:, 1:])
        got = u if nsamp else u[:, c * per_chain:(c + 1) * per_chain]
        assert got.shape == uo.shape
        assert np.abs(got - uo).max() < 1e-8 * max(1.0, np.abs(uo).max()), (d["kind"], d["family"], d["link"], c)


# form -> (kind, GLMMR_MCML_ZL, what sparse_plan() must say)
FORMS = {
    "product_short": ("rct", "product", dict(factored=False, long_rows=False, fused=0, max_blk=1, W=2)),
    "product_long": ("sw_long", "product", dict(factored=False, long_rows=True, fused=0, max_blk=5, W=5)),
    "fused8_long": ("sw_long", "factored", dict(factored=True, long_rows=True, fused=8, max_blk=5)),
    "fused16": ("sw_blk12", "factored", dict(factored=True, long_rows=False, fused=16, max_blk=12)),
    "unfused17": ("sw_blk17", "factored", dict(factored=True, long_rows=False, fused=0, max_blk=17)),
}
# the block-size edges of the fused kernels and the short-row kernel on rows of 1-3 and 4 + remainder entries
EDGE_FORMS = {
    "sw_short_product": ("sw_short", "product", dict(factored=False, long_rows=False, fused=0, max_blk=5)),
    "sw_short_factored": ("sw_short", "factored", dict(factored=True, long_rows=False, fused=8, max_blk=5)),
    "fused8_blk8": ("sw_blk8", "factored", dict(factored=True, long_rows=False, fused=8, max_blk=8)),
    "fused16_blk16": ("sw_blk16", "factored", dict(factored=True, long_rows=False, fused=16, max_blk=16)),
}


def test_design_shapes():
    """the shape conditions the cases below rely on, so that a later edit of the sizes cannot lose them"""
    n = {k: design(k, "poisson", "log")["n"] for k in KINDS}
    assert n["rct"] % 2 == 1 and n["rct"] % 4 != 0                      # misaligned ELL slots, ragged last wave
    assert n["sw_long"] % 4 == 0 and n["sw_long"] % 16 != 0             # whole waves, a partly filled last workgroup
    assert n["tiny"] < 64 and design("tiny", "poisson", "log")["Q"] < 16
    assert design("long_wide", "poisson", "log")["Q"] > 4096
    assert design("sw_long", "poisson", "log")["Q"] * 3 % 8 != 0          # k_cm_backward_long's 8-XCD map, 130 chains
    for kind, blk in (("rct", 1), ("sw_short", 5), ("sw_blk8", 8), ("sw_blk12", 12), ("sw_blk16", 16), ("sw_blk17", 17)):
        d = design(kind, "poisson", "log")
        assert max(d["dims"]) == blk and len(d["dims"]) % 4 != 0, kind
    st = structure(design("sw_short", "poisson", "log"))
    assert set(st["rows_z"]) == {3}                                     # Z': rows shorter than 4
    assert {3, 6, 9}.issubset(set(st["rows_zl"]))                       # ZL': below 4, 4 + remainder, 8 + remainder
    st = structure(design("sw_long", "poisson", "log"))
    assert st["nnz"] == 120 * 35 and st["nnz_z"] == 40 * 35
    assert set(st["rows_z"]) == {40} and {40, 200}.issubset(set(st["rows_zl"]))
    d = design("sw_short", "poisson", "log", slope=True)
    z = d["Z"][d["Z"] != 0]
    assert z.min() >= 0.5 and z.max() <= 1.5 and np.abs(z - 1).max() > 0.3
    d = design("sw_long", "poisson", "log", ragged=RAGGED)
    st = structure(d)
    assert {1, 2, 37, 39, 40}.issubset(set(st["rows_z"])) and st["nnz_z"] >= 24 * d["Q"]      # long rows, factored
    assert {1, 2}.issubset(set(st["rows_zl"])) and any(r % 4 == 3 for r in st["rows_zl"]) and \
        any(r % 8 in (5, 6, 7) for r in st["rows_zl"]) and st["nnz"] >= 24 * d["Q"]            # long rows, product
    for kind in ("sw_short", "sw_long"):
        d = design(kind, "poisson", "log", drop=DROP[kind])
        st = structure(d)
        assert (st["rows_z"] == 0).sum() == 2 and (st["rows_zl"] == 0).sum() == 1, kind


# ---------------------------------------------------------------- a) log_prob / log_grad, all 12 cases x 5 forms
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("family,link,vp", CASES)
@gpu
def test_log_prob_grad(orc, family, link, vp, form, monkeypatch):
    """3 columns (one partly filled group), 64 (one full), 65 (a second group of one chain), 130 (three groups)"""
    kind, zl, expect = FORMS[form]
    d = design(kind, family, link)
    with context(d, monkeypatch, zl) as ctx:
        for ncols in (3, 64, 65, 130):
            V = np.asfortranarray(np.random.default_rng(3 + ncols).normal(size=(d["Q"], ncols)) * 0.3)
            lp, G = ctx.log_prob_grad(d["beta"], vp, V)
            p = assert_plan(ctx, d, ncols, **expect)
            if form == "product_long" and ncols == 130:
                assert p["ncb"] >= 2 and d["Q"] * p["ncb"] % 8 != 0, p
            check_log_prob_grad(orc, d, lp, G, V, cols=GROUP_EDGES if ncols == 130 else None)


# ---------------------------------------------------------------- b) chain by chain
def _run_and_check(orc, monkeypatch, d, zl, expect, C, compare):
    with context(d, monkeypatch, zl) as ctx:
        u, flags, probs = run_chains(ctx, d, C)
        assert_plan(ctx, d, C, **expect)
    assert u.shape == (d["Q"], C)
    check_chains(orc, d, u, flags, probs, compare)
    return u, flags, probs


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("family,link,vp", CHAIN_CASES)
@gpu
def test_chains(orc, family, link, vp, form, monkeypatch):
    """130 chains after a short adaptive warm-up: step size and step count differ per chain, so the s >= st masking of
    cm_leapfrog and live / last of k_cm_Lcol_Lrow decide what is written"""
    kind, zl, expect = FORMS[form]
    _run_and_check(orc, monkeypatch, design(kind, family, link), zl, expect, 130, GROUP_EDGES)


@pytest.mark.parametrize("form", list(EDGE_FORMS))
@pytest.mark.parametrize("family,link,vp", [CASES[2], CASES[6]])
@gpu
def test_chains_block_and_row_edges(orc, family, link, vp, form, monkeypatch):
    """blocks of exactly 8 and 16 (the last size each fused instance takes) and rows of 3 / 6 / 9 entries on the short-row
    kernel; binomial-logit and gaussian-identity (post = 1 / vp^2)"""
    kind, zl, expect = EDGE_FORMS[form]
    _run_and_check(orc, monkeypatch, design(kind, family, link), zl, expect, 130, GROUP_EDGES)


@pytest.mark.parametrize("C,compare", [(64, [0, 31, 63]), (65, [0, 63, 64])])
@gpu
def test_chains_at_the_group_boundary(orc, C, compare, monkeypatch):
    """exactly one full group, and one chain more, on the long-row product form (gamma-log: post = vp)"""
    kind, zl, expect = FORMS["product_long"]
    _run_and_check(orc, monkeypatch, design(kind, "gamma", "log"), zl, expect, C, compare)


# ---------------------------------------------------------------- c) several kept draws per chain
@gpu
def test_three_draws_per_chain(orc, monkeypatch):
    """nsamp = 3 x chains: k_cm_commit runs between the stored draws instead of the commit folded into k_cm_propose"""
    kind, zl, expect = FORMS["fused8_long"]
    d = design(kind, "gaussian", "log")
    C = 70
    with context(d, monkeypatch, zl) as ctx:
        diag, flags, probs = ctx.hmc_sample(d["beta"], _vp(d), WARM, 3 * C, LAM, MS, TA, SEED, chains=C, iter_idx=IT,
                                            adapt=ADAPT, want_trace=True)
        u = ctx.get_u()
        assert_plan(ctx, d, C, **expect)
    assert u.shape == (d["Q"], 3 * C) and flags.shape == (C, WARM + 3)
    check_chains(orc, d, u, flags, probs, [0, 63, 64, 69], per_chain=3)


@pytest.mark.parametrize("form", ["product_short", "product_long", "fused8_long", "unfused17"])
@gpu
def test_single_chain_reference_layout(orc, form, monkeypatch):
    """chains = 1: the reference's Q x (nsamp + 1) layout, on the product and on the factored form"""
    kind, zl, expect = FORMS[form]
    d = design(kind, "binomial", "probit")
    nsamp = 3
    with context(d, monkeypatch, zl) as ctx:
        diag, flags, probs = ctx.hmc_sample(d["beta"], _vp(d), WARM, nsamp, LAM, MS, TA, SEED, chains=1, iter_idx=IT,
                                            adapt=ADAPT, want_trace=True)
        u = ctx.get_u()
        assert_plan(ctx, d, 1, **expect)
    assert u.shape == (d["Q"], nsamp + 1)
    check_chains(orc, d, u, flags, probs, [0], nsamp=nsamp)


# ---------------------------------------------------------------- d) edges
# (name, kind, design options, form, plan, families for log_prob / log_grad, family for the chains)
EDGES = [
    ("slope_product", "sw_short", dict(slope=True), "product", dict(factored=False, long_rows=False),
     [CASES[0], CASES[6]], CASES[6]),
    ("slope_factored", "sw_short", dict(slope=True), "factored", dict(factored=True, long_rows=False, fused=8),
     [CASES[2], CASES[8]], CASES[8]),
    ("slope_long", "sw_long", dict(slope=True), "factored", dict(factored=True, long_rows=True, fused=8),
     [CASES[5], CASES[7]], CASES[7]),
    ("empty_short_product", "sw_short", dict(drop=DROP["sw_short"]), "product", dict(factored=False, long_rows=False),
     [CASES[2], CASES[6]], CASES[6]),
    ("empty_short_factored", "sw_short", dict(drop=DROP["sw_short"]), "factored", dict(factored=True, long_rows=False),
     [CASES[0], CASES[11]], CASES[0]),
    ("empty_long_product", "sw_long", dict(drop=DROP["sw_long"]), "product", dict(factored=False, long_rows=True),
     [CASES[0], CASES[9]], CASES[8]),
    ("empty_long_factored", "sw_long", dict(drop=DROP["sw_long"]), "factored", dict(factored=True, long_rows=True),
     [CASES[2], CASES[6]], CASES[6]),
    ("ragged_long_product", "sw_long", dict(ragged=RAGGED), "product", dict(factored=False, long_rows=True),
     [CASES[2], CASES[6]], CASES[8]),
    ("ragged_long_factored", "sw_long", dict(ragged=RAGGED), "factored", dict(factored=True, long_rows=True, fused=8),
     [CASES[0], CASES[8]], CASES[6]),
    ("tiny", "tiny", dict(), None, dict(factored=False, long_rows=False, W=2),
     [CASES[2], CASES[10]], CASES[2]),
]


@pytest.mark.parametrize("name,kind,opts,zl,expect,lp_cases,chain_case", EDGES, ids=[e[0] for e in EDGES])
@gpu
def test_edges(orc, name, kind, opts, zl, expect, lp_cases, chain_case, monkeypatch):
    """z != 1 in ell_val / zcsr_val (a dropped or squared z), empty CSR rows in both backward kernels (G = -x), rows of
    1, 2, 4k + 1 and 4k + 3 entries on the long-row kernel (quarters that are clipped or empty), and a design smaller than one chunk of every two-stage sum: 70 columns (two groups), then 70 chains"""
    for family, link, vp in lp_cases:
        d = design(kind, family, link, **opts)
        V = np.asfortranarray(np.random.default_rng(4).normal(size=(d["Q"], 70)) * 0.3)
        with context(d, monkeypatch, zl) as ctx:
            lp, G = ctx.log_prob_grad(d["beta"], vp, V)
            assert_plan(ctx, d, 70, **expect)
        check_log_prob_grad(orc, d, lp, G, V)
        if "drop" in opts:
            st = structure(d)
            rows = st["rows_z"] if expect["factored"] else st["rows_zl"]
            assert (rows == 0).any()
            if not expect["factored"]:
                q = int(np.nonzero(rows == 0)[0][0])
                assert np.array_equal(G[q], -V[q])                       # no observation loads on q: g = -x exactly
    family, link, vp = chain_case
    _run_and_check(orc, monkeypatch, design(kind, family, link, **opts), zl, expect, 70, [0, 63, 64, 69])


@gpu
def test_more_than_4096_random_effects(orc, monkeypatch):
    """Q = 4100: the per-chain sums take chunks of 64 rows (cm_qrows) and cm_sum_chunks its eight-loads-in-flight loop
    (65 chunks over the effects, 231 over the observations).  L is diagonal here, so the oracle's factor is taken as
    sqrt(D) instead of a dense Cholesky of 4100 x 4100; the oracle's dense 3690 x 4100 products make one short chain
    cost seconds, so a few columns and three chains are compared"""
    for family, link, vp in (CASES[0], CASES[6]):
        d = design("long_wide", family, link)
        assert d["Q"] > 4096 and max(d["dims"]) == 1
        D = orc.gen_D(d["cov"], d["data"], d["eff_range"], d["theta"], chol=False)
        assert np.count_nonzero(D) == d["Q"]
        L = np.sqrt(D)
        V = np.asfortranarray(np.random.default_rng(4).normal(size=(d["Q"], 70)) * 0.3)
        with context(d, monkeypatch, None) as ctx:
            lp, G = ctx.log_prob_grad(d["beta"], vp, V)
            assert_plan(ctx, d, 70, factored=False, long_rows=False, qrows=64, W=2)
            check_log_prob_grad(orc, d, lp, G, V, cols=[0, 63, 64, 69], L=L)
            if family == "gaussian":
                u, flags, probs = run_chains(ctx, d, 70)
                assert_plan(ctx, d, 70, factored=False, long_rows=False, qrows=64)
                check_chains(orc, d, u, flags, probs, [0, 64, 69], L=L)


# ---------------------------------------------------------------- e) form against form
FORM_DESIGNS = [(k, {}) for k in ("rct", "sw_short", "sw_long", "sw_blk8", "sw_blk12", "sw_blk16", "sw_blk17", "long_wide",
                                  "tiny")] + \
               [("sw_short", dict(slope=True)), ("sw_long", dict(slope=True)), ("sw_short", dict(drop=DROP["sw_short"])),
                ("sw_long", dict(drop=DROP["sw_long"])), ("sw_long", dict(ragged=RAGGED))]


@pytest.mark.parametrize("kind,opts", FORM_DESIGNS, ids=["%s%s" % (k, "".join("_" + o for o in v)) for k, v in FORM_DESIGNS])
@gpu
def test_forms_agree(kind, opts, monkeypatch):
    """product, factored and factored with GLMMR_MCML_CM_LFUSE=0 are the same sampler at 130 chains: identical flags,
    probabilities within 1e-9, draws within 1e-8; fused against unfused bit for bit"""
    d = design(kind, "gaussian", "identity", **opts)
    C = 130
    blk = max(d["dims"])
    fused = 0 if blk > 16 else (8 if blk <= 8 else 16)
    out = {}
    for name, zl, lfuse in (("product", "product", None), ("factored", "factored", None), ("unfused", "factored", "0")):
        with context(d, monkeypatch, zl, lfuse) as ctx:
            u, flags, probs = run_chains(ctx, d, C)
            assert_plan(ctx, d, C, factored=(zl == "factored"), fused=fused if name == "factored" else 0)
            out[name] = (u, flags, probs)
    for k in range(3):
        assert np.array_equal(out["factored"][k], out["unfused"][k]), k
    assert np.array_equal(out["product"][1], out["factored"][1])
    assert np.abs(out["product"][2] - out["factored"][2]).max() < 1e-9
    assert np.abs(out["product"][0] - out["factored"][0]).max() < 1e-8


# ---------------------------------------------------------------- f) fallbacks of sparse_zl_setup
def _last_effect_design(nblk, blk, family, link):
    """nblk gr x ar1 blocks of blk; every observation loads on the LAST effect of every block: a row of ZL is
    nblk * blk wide"""
    s = synth.stepped_wedge(ncl=nblk, nt=blk, nind=1)
    n, Q = 40, nblk * blk
    Z = np.zeros((n, Q), order="F")
    for b in range(nblk):
        Z[:, (b + 1) * blk - 1] = 1.0
    centre = _centre(family, link)
    y = _y(family, link, np.full(n, centre), np.random.default_rng(99))
    return dict(cov=s["cov"], data=s["data"], eff_range=s["eff_range"], Z=Z, X=np.ones((n, 1), order="F"), y=y,
                family=family, link=link, beta=np.array([centre]), theta=np.array((0.1, 0.8)), n=n, Q=Q,
                dims=[blk] * nblk, kind="last%dx%d" % (nblk, blk), zkind="last", seed=("sparse", "last", nblk, blk))


@pytest.mark.parametrize("which", ["block33", "row72"])
@gpu
def test_dense_fallbacks_still_equal_the_oracle(orc, which, monkeypatch):
    """a block of 33 (above SMALL_BLOCK: its factor takes the dense path) and a row of ZL 72 wide (above the ELL limit
    of 64) leave the sparse operator inactive; a dense kernel runs and equals the oracle"""
    if which == "block33":
        s = synth.stepped_wedge(ncl=2, nt=33, nind=2)
        d = dict(s, X=np.ones((s["n"], 1), order="F"), beta=np.array([0.2]), theta=np.array((0.1, 0.8)), dims=[33, 33],
                 kind="block33", zkind="block33", seed=("sparse", "block33"))
        d["y"] = _y("binomial", "logit", np.full(d["n"], 0.2), np.random.default_rng(98))
    else:
        d = _last_effect_design(3, 24, "binomial", "logit")
    C = 40
    with context(d, monkeypatch, None) as ctx:
        assert not ctx.sparse_plan(C)["active"]
        u, flags, probs = run_chains(ctx, d, C)
        kinds = set(ctx.last_kernels())
        assert kinds <= {"band", "dlds", "reg"}, kinds
        assert ctx.profile(enable=False)["operator"] != "sparse"
        p = ctx.sparse_plan(C)
        assert not p["active"] and not p["factored"] and p["fused"] == 0 and p["W"] == 0, p
    check_chains(orc, d, u, flags, probs, [0, 15, 16, 39])


@gpu
@pytest.mark.parametrize("zl", ["product", None])
def test_row_of_exactly_64_stays_sparse(orc, zl, monkeypatch):
    """two blocks of 32, every observation on the last effect of both: W = 64, the widest row the ELL form takes.  As the
    product (64 ELL slots per observation) and as the heuristic has it: nz = 80, nl = 2 * 528, Q = 64, nnz = 2560,
    4 (80 + 1056 + 128) = 5056 < 7680: factored, and blocks of 32 keep k_cm_Lcol / k_cm_Lrow apart"""
    d = _last_effect_design(2, 32, "binomial", "logit")
    C = 70
    with context(d, monkeypatch, zl) as ctx:
        u, flags, probs = run_chains(ctx, d, C)
        assert_plan(ctx, d, C, W=64, max_blk=32, fused=0, factored=(zl is None), long_rows=(zl == "product"))
    check_chains(orc, d, u, flags, probs, [0, 63, 64, 69])


# ---------------------------------------------------------------- g) the forms the benchmark's configurations run
@gpu
def test_sparse_plan_of_the_bench_configurations(monkeypatch):
    """configs 1, 4 and 5 at full size (context and update_L only).  factored when 4 (nz + nl + 2 Q) < 3 nnz; long rows
    when nnz >= 24 Q of the operand the backward product gathers through (Z' when factored); fused width from max_blk.
    config 1, cluster_rct(10, 5, 10): n = 500, Q = 60 blocks of 1; nz = nnz = 1000, nl = 60.
        4 (1000 + 60 + 120) = 4720 >= 3000: product;  1000 < 24 * 60 = 1440: short rows.
    config 4, stepped_wedge(40, 8, 50): n = 16000, Q = 320 in 40 blocks of 8; nz = 16000, nl = 40 * 36 = 1440,
        nnz = 40 * 50 * (1 + ... + 8) = 72000.  4 (16000 + 1440 + 640) = 72320 < 216000: factored;
        nnz(Z) = 16000 >= 24 * 320 = 7680: long rows on Z';  max_blk = 8: k_cm_Lcol_Lrow<8>.
    config 5, longitudinal(2000, 10): n = 20000, Q = 22000 blocks of 1; nz = nnz = 40000, nl = 22000.
        4 (40000 + 22000 + 44000) = 424000 >= 120000: product;  40000 < 528000: short rows;  Q > 4096: chunks of 64."""
    want = [(synth.cluster_rct(), 64, dict(factored=False, W=2, nnz=1000, nnz_z=1000, nnz_l=60, nblk=60, max_blk=1,
                                           long_rows=False, fused=0, qrows=16, ncb=1)),
            (synth.stepped_wedge(40, 8, 50), 512, dict(factored=True, W=8, nnz=72000, nnz_z=16000, nnz_l=1440, nblk=40,
                                                       max_blk=8, long_rows=True, fused=8, qrows=16, ncb=8)),
            (synth.longitudinal(2000, 10), 1024, dict(factored=False, W=2, nnz=40000, nnz_z=40000, nnz_l=22000,
                                                      nblk=22000, max_blk=1, long_rows=False, fused=0, qrows=64, ncb=16))]
    monkeypatch.delenv("GLMMR_MCML_ZL", raising=False)
    monkeypatch.delenv("GLMMR_MCML_CM_LFUSE", raising=False)
    for d, C, expect in want:
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
            ctx.update_L(d["theta"])
            p = ctx.sparse_plan(C)
        assert p == dict(expect, active=True), (p, expect)
