"""GPU parity of mvn_ll, genD and what follows from L on covariance layouts with more than one kind of block
(tests/cov_layouts.py): diagonal, one-wave and blocked-Cholesky blocks in one model, several large blocks in one
workspace, large blocks at odd and even non-zero offsets, blocks of exactly 32 and 33, three-term products, shared
parameters, m = 1 and m > 1024.  Every value is compared with the CPU oracle AND with the numpy definition
(test_cov_layouts_cpu.py pins the one to the other).  Tolerances are those of test_gpu_mvn_model.py: 1e-10 relative
for mvn_ll, L within 1e-10 max|L| and by reconstruction, 1e-11 between a batched and a single evaluation."""
import numpy as np
import pytest

import cov_layouts as cl

pytestmark = pytest.mark.gpu
RTOL = 1e-10
NAMES = sorted(cl.LAYOUTS)


def _rel(a, b):
    return abs(a - b) / max(1e-300, abs(b))


def _wire(blocks):
    cov, data = cl.layout(blocks)
    return cov, data, np.zeros(cov.shape[0])


def _worst(D, want, bound):
    """largest |D - want| as a multiple of the entrywise bound, and where"""
    ratio = np.abs(D - want) / np.where(bound > 0, bound, 1.0)
    at = np.unravel_index(ratio.argmax(), ratio.shape)
    return float(ratio[at]), tuple(int(i) for i in at)


# ------------------------------------------------------------------------------------------------ log-likelihood
@pytest.mark.parametrize("m", [1, 70, 1100])
def test_mvn_ll_mixed(orc, m):
    """all three paths into one scalar; 70 columns cross one 64-column pass of k_small_ll, 1100 cross its 16 x 64
    grid and the 64-row cap of k_diag_ll's; nine evaluations on one context take the 289-block (the one above 256)
    through eager, eager, capture and replay, and every repeat at one theta gives the same bits"""
    from glmmrmcml_amd import api
    cov, data, eff = _wire(cl.MIXED)
    thetas = cl.thetas("MIXED")
    u = cl.sample_matrix("MIXED")[:, :m]
    want_o = [orc.mvn_ll(cov, data, eff, t, u) for t in thetas]
    want_d = [cl.reference_ll("MIXED", ti, m) for ti in range(3)]
    got = api.mvn_ll(cov, data, eff, thetas[0], u if m > 1 else u[:, 0])
    assert _rel(got, want_o[0]) < RTOL and _rel(got, want_d[0]) < RTOL, (got, want_o[0], want_d[0])
    with api.Context(cov, data, eff) as ctx:
        ctx.set_u(u)
        first = [None] * 3
        for ti in (0, 0, 0, 0, 0, 1, 1, 2, 2, 0):
            v = ctx.mvn_ll(thetas[ti])
            assert _rel(v, want_o[ti]) < RTOL and _rel(v, want_d[ti]) < RTOL, (ti, v, want_o[ti], want_d[ti])
            first[ti] = v if first[ti] is None else first[ti]
            assert v == first[ti], (ti, v, first[ti])


def test_mvn_ll_mixed_is_the_sum_of_its_paths(orc):
    """the diagonal blocks alone, the small blocks alone and the large blocks alone, as models of their own on the
    matching rows of u: each equals the oracle, and the three add up to the mixed model's value (1e-12: the same
    terms in another order) -- a failure of the mixed value is then one path's, or the accumulation's"""
    from glmmrmcml_amd import api
    m = 70
    theta = cl.MIXED_THETA
    u = cl.sample_matrix("MIXED")[:, :m]
    cov, data, eff = _wire(cl.MIXED)
    full = api.mvn_ll(cov, data, eff, theta, u)
    parts = {}
    for kind in ("diag", "small", "large"):
        sub = [b for b in cl.MIXED if cl.kind(b) == kind]
        rows = np.concatenate([np.arange(s, s + b[0]) for s, b in zip(cl.starts(cl.MIXED), cl.MIXED) if cl.kind(b) == kind])
        assert len(sub) >= 2 and rows.size == cl.total_dim(sub)
        scov, sdata, seff = _wire(sub)
        su = np.asfortranarray(u[rows])
        parts[kind] = api.mvn_ll(scov, sdata, seff, theta, su)
        assert _rel(parts[kind], orc.mvn_ll(scov, sdata, seff, theta, su)) < RTOL, kind
        assert _rel(parts[kind], cl.definition(sub, theta, su)[1]) < RTOL, kind
    assert _rel(sum(parts.values()), full) < 1e-12, (parts, full)
    assert _rel(full, orc.mvn_ll(cov, data, eff, theta, u)) < RTOL


# ------------------------------------------------------------------------------------------------ genD
@pytest.fixture(scope="module")
def gpu_D_L():
    """D and L of every named layout at its first theta, computed once"""
    from glmmrmcml_amd import api
    out = {}
    for name in NAMES:
        cov, data, eff = _wire(cl.LAYOUTS[name][0])
        with api.Context(cov, data, eff) as ctx:
            D = ctx.gen_D(cl.LAYOUTS[name][1], chol=False)
            L = ctx.gen_D(cl.LAYOUTS[name][1], chol=True)
        D.setflags(write=False); L.setflags(write=False)
        out[name] = (D, L)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_gen_D_and_chol(orc, gpu_D_L, name):
    """D and its Cholesky factor, block by block: MIXED has large blocks at 3 and 233 (odd starts: mvn_gen_L
    factorises in an aligned copy and copies back) and at 158, TWO_LARGE_B one at 161 (odd), TWO_LARGE_A one at
    300 (even: factorised in place), EDGE32 the sizes either side of the small / large threshold"""
    blocks, theta = cl.LAYOUTS[name]
    cov, data, eff = _wire(blocks)
    D, L = gpu_D_L[name]
    ref = cl.reference(name)
    Do = orc.gen_D(cov, data, eff, theta)
    Lo = orc.gen_D(cov, data, eff, theta, chol=True)
    Q = cl.total_dim(blocks)
    assert D.shape == (Q, Q) and L.shape == (Q, Q)
    inside = np.zeros((Q, Q), dtype=bool)
    for s, b in zip(cl.starts(blocks), blocks):
        inside[s:s + b[0], s:s + b[0]] = True
    assert not D[~inside].any() and not L[~inside].any(), "non-zero outside the blocks"
    assert np.array_equal(np.triu(L, 1), np.zeros_like(L)), "upper triangle of L"
    assert np.array_equal(D, D.T)
    for s, b in zip(cl.starts(blocks), blocks):
        sl = slice(s, s + b[0])
        tag = (name, "block of %d at %d" % (b[0], s))
        # D: 2^-52 (8 + 2 sum |a_k|) |D_ij| against the oracle and the definition, the derived bound
        # (cov_layouts.dense_definition) against the definition's long-double value
        for what, Dw, bound in (("oracle", Do, "bound"), ("definition", ref["D"], "bound"), ("long-double value", ref["exact"], "derived")):
            worst, at = _worst(D[sl, sl], Dw[sl, sl], ref[bound][sl, sl])
            assert worst <= 1.0, tag + ("D against the " + what, at, worst)
        # L: entries span many orders of magnitude: compare in the norm, and by reconstruction
        for what, Lw, Dw in (("oracle", Lo, Do), ("definition", ref["L"], ref["D"])):
            assert np.abs(L[sl, sl] - Lw[sl, sl]).max() < 1e-10 * np.abs(Lw[sl, sl]).max(), tag + ("L against the " + what,)
            recon = np.abs(L[sl, sl] @ L[sl, sl].T - Dw[sl, sl]).max()
            assert recon < 1e-13 * max(1.0, np.abs(Dw[sl, sl]).max()) * b[0], tag + ("L L' against the " + what, recon)
    assert np.abs(L - Lo).max() < 1e-10 * np.abs(Lo).max()
    assert np.abs(L @ L.T - Do).max() < 1e-13 * max(1.0, np.abs(Do).max()) * Q


# ------------------------------------------------------------------------------------------------ batched
def _candidates(name, k):
    """k parameter vectors around the layout's own, inside the ranges the condition bound was checked for"""
    spread = np.array([0.3, 0.04, 0.2, 0.05])
    return np.array([cl.LAYOUTS[name][1] * (1 + s * spread) for s in np.linspace(-1.0, 1.0, k)])


@pytest.mark.parametrize("name", ["TWO_LARGE_A", "TWO_LARGE_B"])
def test_mvn_ll_batch_two_large_blocks(orc, name):
    """the batchable path (large blocks only) with two blocks of different padded size in one workspace, in either
    order: 2, 8 and 8 + 1 candidates equal the single evaluations (1e-11), the oracle and the definition (1e-10),
    repeat bit for bit, and a candidate whose AR1 block is not positive definite is NaN without touching the rest"""
    from glmmrmcml_amd import api
    blocks = cl.LAYOUTS[name][0]
    cov, data, eff = _wire(blocks)
    u = cl.sample_matrix(name)
    T = _candidates(name, 9)
    want_o = np.array([orc.mvn_ll(cov, data, eff, t, u) for t in T])
    want_d = np.array([cl.definition(blocks, t, u)[1] for t in T])
    assert np.abs(want_o - want_d).max() < 1e-12 * np.abs(want_d).max()
    with api.Context(cov, data, eff) as ctx:
        ctx.set_u(u)
        single = np.array([ctx.mvn_ll(t) for t in T])
        assert np.abs(single - want_o).max() < RTOL * np.abs(want_o).max()
        for k in (2, 8, 9):
            first = None
            for rep in range(3):
                got = ctx.mvn_ll_batch(T[:k])
                assert got.shape == (k,)
                assert (np.abs(got - single[:k]) < 1e-11 * np.abs(single[:k])).all(), (k, rep, got, single[:k])
                assert (np.abs(got - want_o[:k]) < RTOL * np.abs(want_o[:k])).all(), (k, rep, got, want_o[:k])
                assert (np.abs(got - want_d[:k]) < RTOL * np.abs(want_d[:k])).all(), (k, rep, got, want_d[:k])
                first = got if first is None else first
                assert np.array_equal(got, first), (k, rep, got, first)
        clean = ctx.mvn_ll_batch(T[:3])
        bad = T[:3].copy(); bad[1, cl.TWO_LARGE_RHO] = 1.5
        got = ctx.mvn_ll_batch(bad)
        assert np.isnan(got[1]) and got[0] == clean[0] and got[2] == clean[2], (got, clean)
        assert np.array_equal(ctx.mvn_ll_batch(T[:3]), clean)
        assert ctx.mvn_ll(T[0]) == single[0]


def test_mvn_ll_batch_mixed_falls_back_to_single_evaluations():
    """a model with diagonal or small blocks is not batchable: the loop over single evaluations, the same bits"""
    from glmmrmcml_amd import api
    cov, data, eff = _wire(cl.MIXED)
    T = np.array(cl.thetas("MIXED"))
    with api.Context(cov, data, eff) as ctx:
        ctx.set_u(cl.sample_matrix("MIXED")[:, :70])
        single = np.array([ctx.mvn_ll(t) for t in T])
        assert np.array_equal(ctx.mvn_ll_batch(T), single)
        bad = T.copy(); bad[1, cl.MIXED_RHO] = 1.5
        got = ctx.mvn_ll_batch(bad)
        assert np.isnan(got[1]) and got[0] == single[0] and got[2] == single[2], (got, single)


# ------------------------------------------------------------------------------------------------ error state
@pytest.mark.parametrize("name,rho,m", [("MIXED", cl.MIXED_RHO, 70), ("TWO_LARGE_A", cl.TWO_LARGE_RHO, 40)])
def test_not_positive_definite_block_among_others(orc, name, rho, m):
    """an AR1 parameter of 1.5 makes one block (MIXED: the 5-dim one-wave block; TWO_LARGE_A: the second large block)
    not positive definite while the others are fine: error -3, and the context goes on giving right values"""
    from glmmrmcml_amd import api, _lib
    blocks = cl.LAYOUTS[name][0]
    cov, data, eff = _wire(blocks)
    thetas = cl.thetas(name)
    u = cl.sample_matrix(name)[:, :m]
    bad = thetas[0].copy(); bad[rho] = 1.5
    with api.Context(cov, data, eff) as ctx:
        ctx.set_u(u)
        good = ctx.mvn_ll(thetas[0])
        assert _rel(good, cl.reference_ll(name, 0, m)) < RTOL
        for rep in range(2):
            with pytest.raises(_lib.McmlError) as e:
                ctx.mvn_ll(bad)
            assert e.value.code == -3
            assert ctx.mvn_ll(thetas[0]) == good
            v = ctx.mvn_ll(thetas[1 + rep])
            assert _rel(v, orc.mvn_ll(cov, data, eff, thetas[1 + rep], u)) < RTOL
            assert _rel(v, cl.reference_ll(name, 1 + rep, m)) < RTOL
        L = ctx.gen_D(thetas[0], chol=True)
    ref = cl.reference(name)
    assert np.abs(L - ref["L"]).max() < 1e-10 * np.abs(ref["L"]).max()
    assert np.abs(L @ L.T - ref["D"]).max() < 1e-13 * max(1.0, np.abs(ref["D"]).max()) * L.shape[0]
    assert np.array_equal(np.triu(L, 1), np.zeros_like(L))


# ------------------------------------------------------------------------------------------------ downstream of L
def test_log_prob_grad_on_a_partly_dense_L(orc):
    """update_L on MIXED, then the sampler's products with Z = two stacked identities (n = 2 Q), poisson-log:
    log_prob / log_grad against the oracle's with Z L_oracle, 1e-10 as in test_gpu_families.py -- whichever form the
    planner picks for an L with diagonal, small dense and large dense parts"""
    from glmmrmcml_amd import api
    cov, data, eff = _wire(cl.MIXED)
    theta = cl.MIXED_THETA
    Q = cl.total_dim(cl.MIXED)
    rng = np.random.default_rng(12)
    Z = np.asfortranarray(np.vstack([np.eye(Q), np.eye(Q)]))
    X = np.ones((2 * Q, 1), order="F")
    beta = np.array([0.2])
    Lo = orc.gen_D(cov, data, eff, theta, chol=True)
    assert np.abs(Lo - cl.reference("MIXED")["L"]).max() < 1e-10 * np.abs(Lo).max()
    ZL, xb = Z @ Lo, X @ beta
    y = rng.poisson(np.exp(xb + ZL @ (0.5 * rng.normal(size=Q)))).astype(float)
    V = rng.normal(size=(Q, 4)) * 0.5
    fl = orc.flink("poisson", "log")
    with api.Context(cov, data, eff, Z, X, y, "poisson", "log") as ctx:
        ctx.update_L(theta)
        lp, G = ctx.log_prob_grad(beta, 1.0, V)
    for c in range(4):
        lo = orc.log_prob(xb, ZL, y, 1.0, fl, V[:, c])
        go = orc.log_grad(xb, ZL, y, 1.0, fl, V[:, c])
        assert lp[c] == pytest.approx(lo, rel=1e-10)
        assert np.abs(G[:, c] - go).max() < 1e-10 * max(1.0, np.abs(go).max())


# ------------------------------------------------------------------------------------------------ parser
def test_parser_errors():
    from glmmrmcml_amd import api, _lib
    cov, data, eff = _wire(cl.EDGE32)
    theta = cl.EDGE32_THETA
    u = cl.sample_matrix("EDGE32")[:, :3]
    for fn in (5, 6, 8, 9, 10, 11, 12, 13):                   # in the parameter-count table, not built
        bad = cov.copy(); bad[1, 2] = fn
        with pytest.raises(_lib.McmlError) as e:
            api.mvn_ll(bad, data, eff, np.r_[theta, 0.1], u)
        assert e.value.code == -2, fn
    mcov, mdata, meff = _wire(cl.MIXED)
    bad = mcov.copy()
    assert bad[4, 0] == bad[5, 0] and bad[5, 1] == 5          # the two rows of the gr * ar1 block
    bad[5, 1] = 6
    with pytest.raises(_lib.McmlError):
        api.Context(bad, mdata, meff)
    with pytest.raises(_lib.McmlError):
        api.Context(mcov, mdata[:-1], meff)
    with api.Context(mcov, mdata, meff) as ctx:                # the unmodified triple is accepted
        assert ctx.Q == 522 and ctx.npar() == len(cl.MIXED_THETA)
