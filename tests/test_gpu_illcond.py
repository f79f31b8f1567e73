"""mvn_ll, its score, gen_D and the Cholesky stack on ill-conditioned blocks (kappa_2 = 1e6 .. 2e12), against the
long-double reference of tests/illcond_cases.py under bounds calibrated by that module's float64 twins of the library's own
algorithm (C = max(existing constant, 4 x twin) per rung; cases, rungs, scales and constants are listed there), and the
breakdown contract past numerical singularity: a call fails with code -3 or returns finite numbers, never a NaN with a
success code, and a failure leaves the context as it was.

Every test prints the device's ratio to the C = 1 bound; the worst per rung are copied into illcond_cases.DEVICE and
DESIGN.md section 2."""
import functools

import numpy as np
import pytest

import chol_reference as cr
import cov_layouts as cl
import illcond_cases as ic

pytestmark = pytest.mark.gpu
LD = np.longdouble
VALUE_M = 17
BATCH_CASES = [(n, r, k) for n in ("SQ300", "FE300", "MIX") for r in ic.RUNGS[n] for k in (2, 8)]


def _ctx(name, m):
    from glmmrmcml_amd import api
    ctx = api.Context(*ic.wire(name))
    ctx.set_u(ic.sample_matrix(name)[:, :m])
    return ctx


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ a. factor and solves
@pytest.fixture(scope="module")
def chol_ctx():
    from glmmrmcml_amd import api
    cov, data = cl.layout([cr.block_S(40)])
    with api.Context(cov, data, np.zeros(cov.shape[0])) as c:
        yield c


@functools.lru_cache(maxsize=4)
def _factor_ratio_of(name, rung, Lbytes):
    A = ic.matrix(name, rung)
    return cr.factor_ratio(A, np.frombuffer(Lbytes).reshape(A.shape))


@pytest.mark.parametrize("m", ic.DIRECT_M)
@pytest.mark.parametrize("name,rung", ic.DIRECT)
def test_factor_and_solves_on_graded_blocks(chol_ctx, name, rung, m):
    """the matrix handed over as it is: factor residual, the three solves' residuals and the inverted diagonal blocks, each
    under its rung's constant; the same bits with the strict upper triangle NaN"""
    A = ic.matrix(name, rung)
    n = A.shape[0]
    B = cr.rhs(n, m)
    C = ic.constants(rung)
    got = chol_ctx.dbg_chol(np.tril(A), B)
    L = np.tril(got["A"])
    wf, at = _factor_ratio_of(name, rung, np.ascontiguousarray(L).tobytes())
    ws = {kind: fn(L, got[kind], B) for kind, fn in (("fwd", cr.forward_ratio), ("trans", cr.trans_ratio),
                                                     ("potrs", lambda l, z, b: cr.potrs_ratio(l, z, b, C["solve"])))}
    wl = []
    for k in range((n + cr.NB - 1) // cr.NB):
        nb = min(cr.NB, n - k * cr.NB)
        X = got["linv"][k]
        assert not np.any(np.triu(X, 1)), ("linv above the diagonal", name, k)
        assert not np.any(X[nb:]) and not np.any(X[:, nb:]), ("linv beyond n", name, k)
        wl.append(cr.linv_ratio(L[k * cr.NB:k * cr.NB + nb, k * cr.NB:k * cr.NB + nb], X[:nb, :nb]))
    print("%s %s m=%d: factor %.3g (C %.3g), fwd %.3g trans %.3g potrs %.3g (C %.3g), linv %s (C %.3g)" % (
        name, rung, m, wf, C["factor"], ws["fwd"][0], ws["trans"][0], ws["potrs"][0], C["solve"],
        ["%.3g" % w for w, _ in wl], C["linv"]))
    assert wf <= C["factor"], ("factor", name, rung, wf, at)
    for kind, (w, where) in ws.items():
        assert w <= C["solve"], (kind, name, rung, m, w, where)
    for k, (w, where) in enumerate(wl):
        assert w <= C["linv"], ("linv", name, rung, k, w, where)
    poisoned = np.tril(A)
    poisoned[np.triu_indices(n, 1)] = np.nan
    again = chol_ctx.dbg_chol(poisoned, B)
    assert np.array_equal(np.tril(again["A"]), L), "the factor changed with the upper triangle"
    for kind in ("fwd", "trans", "potrs", "linv"):
        assert np.array_equal(again[kind], got[kind]), (kind, "changed with the upper triangle")


# ------------------------------------------------------------------------------------------------ b. gen_D
def _block_rung(name, rung, bi):
    return ic.MIX_BLOCK_RUNG[bi] if name == "MIX" else rung


@pytest.mark.parametrize("name,rung", ic.CASE_RUNGS)
def test_gen_D(name, rung):
    """chol=False: every entry within dense_definition's bound (exact zeros outside the blocks).  chol=True: each dense block's
    |L L' - D| within the factor bound of its rung (plus the build bound), the diagonal rows' square roots to 2 ulp, and
    exact zeros above the diagonal and outside the blocks"""
    blocks, th = ic.CASES[name], ic.theta(name, rung)
    D, bound, _, _ = cl.dense_definition(blocks, th)
    with _ctx(name, 1) as ctx:
        got = ctx.gen_D(th, chol=False)
        L = ctx.gen_D(th, chol=True)
    err = np.abs(got - D)
    at = np.unravel_index(int(np.argmax(err - bound)), err.shape)
    assert np.all(err <= bound), (name, rung, at, err[at], bound[at])
    assert np.all(np.isfinite(L)) and not np.any(np.triu(L, 1)), "L above the diagonal"
    inside = np.zeros(L.shape, dtype=bool)
    for bi, (block, s) in enumerate(zip(blocks, cl.starts(blocks))):
        d = block[0]
        sl = slice(s, s + d)
        inside[sl, sl] = True
        if cl.kind(block) == "diag":
            assert np.all(np.abs(np.diag(L[sl, sl]) - np.sqrt(np.diag(D[sl, sl]))) <= 2 * 2.0 ** -52 * np.sqrt(np.diag(D[sl, sl])))
            continue
        C = ic.constants(_block_rung(name, rung, bi))["factor"]
        w, where = cr.factor_ratio(D[sl, sl], L[sl, sl], bound[sl, sl])
        print("%s %s block %d: |L L' - D| at %.3g of the C = 1 bound (C %.3g)" % (name, rung, bi, w, C))
        assert w <= C, (name, rung, bi, w, where)
    assert not np.any(L[~inside]), "L outside the blocks"


# ------------------------------------------------------------------------------------------------ c. mvn_ll
@pytest.mark.parametrize("name,rung", ic.CASE_RUNGS)
def test_mvn_ll_value(name, rung):
    """Context.mvn_ll and the stateless export, m = 1, 17 (SQ300: 130 too): within C_V 2^-52 kappa value_mag of the
    reference; four calls in a row -- eager, eager, captured, replayed where the block takes the graph -- give the same bits"""
    from glmmrmcml_amd import api
    th = ic.theta(name, rung)
    C = ic.constants(rung)["value"]
    for m in ic.MS[name]:
        ref = ic.ref_score(name, rung, m)
        with _ctx(name, m) as ctx:
            vals = [ctx.mvn_ll(th) for _ in range(4)]
        free = api.mvn_ll(*ic.wire(name), th, ic.sample_matrix(name)[:, :m])
        r, rf = ic.value_ratio(vals[0], ref), ic.value_ratio(free, ref)
        print("%s %s m=%d: |value - ref| at %.3g (context), %.3g (stateless) of the C = 1 bound (C %.3g); kappa %.3g" % (
            name, rung, m, r, rf, C, ref["kappa"]))
        assert r <= C and rf <= C, (name, rung, m, r, rf)
        assert all(v == vals[0] for v in vals), (name, rung, m, vals)


@functools.lru_cache(maxsize=None)
def _candidate_reference(name, th, m):
    """(value, kappa, value_mag) of the long-double definition at one candidate"""
    blocks = ic.CASES[name]
    u = ic.sample_matrix(name)[:, :m]
    _, Ls, ll = cl.definition_columns(blocks, np.array(th), u)
    logs = sum(np.abs(np.log(np.diag(L).astype(LD))).sum() for L in Ls)
    const = -sum(np.log(np.diag(L).astype(LD)).sum() for L in Ls) - LD(0.5) * cl.total_dim(blocks) * cl.LOG_2PI
    quad = 2 * (const - ll)
    value_mag = LD(0.5) * cl.total_dim(blocks) * cl.LOG_2PI + logs + LD(0.5) * quad.mean()
    return dict(value=ll.mean(), kappa=ic.kappa_of(name, np.array(th)), value_mag=value_mag)


@pytest.mark.parametrize("name,rung,k", BATCH_CASES)
def test_mvn_ll_batch(name, rung, k):
    """k candidates spread inside one rung (SQ300, FE300: evaluated side by side; MIX: one after the other): each within the
    value bound of its own reference, within the same bound of the single evaluation at that candidate, and a repeated
    round gives the same bits"""
    cand = ic.candidates(name, rung, k)
    C = ic.constants(rung)["value"]
    with _ctx(name, VALUE_M) as ctx:
        vals = ctx.mvn_ll_batch(cand)
        again = ctx.mvn_ll_batch(cand)
        single = [ctx.mvn_ll(th) for th in cand]
    assert np.array_equal(vals, again)
    for j, th in enumerate(cand):
        ref = _candidate_reference(name, tuple(th), VALUE_M)
        r = ic.value_ratio(vals[j], ref)
        rs = float(abs(LD(vals[j]) - LD(single[j])) / (ic.EPS * ref["kappa"] * ref["value_mag"]))
        print("%s %s candidate %d of %d: batch at %.3g, batch - single at %.3g of the C = 1 bound (C %.3g)" % (name, rung, j, k, r, rs, C))
        assert r <= C and rs <= C, (name, rung, j, r, rs)


# ------------------------------------------------------------------------------------------------ d. mvn_ll_grad
@pytest.mark.parametrize("name,rung", ic.CASE_RUNGS)
def test_mvn_ll_grad(name, rung):
    """unweighted and weighted: every entry within 2^-52 kappa mag_k AND within C_G 2^-52 kappa |ref grad_k|; the value within
    its bound; unweighted, the value is mvn_ll's to the bit; a repeated call gives the same bits"""
    th = ic.theta(name, rung)
    C = ic.constants(rung)
    for m in ic.MS[name]:
        with _ctx(name, m) as ctx:
            for w in (None, ic.weights(m)):
                value, grad = ctx.mvn_ll_grad(th, w)
                ref = ic.ref_score(name, rung, m, w)
                loose, tight = ic.grad_ratios(grad, ref)
                rv = ic.value_ratio(value, ref)
                print("%s %s m=%d %s: |grad - ref| / (2^-52 kappa |ref|) = %s (C %.3g), / (2^-52 kappa mag) = %s, value %.3g (C %.3g)" % (
                    name, rung, m, "weighted" if w is not None else "unweighted", np.array2string(tight, precision=3), C["grad"],
                    np.array2string(loose, precision=3), rv, C["value"]))
                assert np.all(np.isfinite(grad))
                assert (loose <= 1.0).all(), (name, rung, m, loose)
                assert (tight <= C["grad"]).all(), (name, rung, m, tight)
                assert rv <= C["value"], (name, rung, m, rv)
                if w is None:
                    assert value == ctx.mvn_ll(th)
                assert _same(ctx.mvn_ll_grad(th, w), (value, grad))


# ------------------------------------------------------------------------------------------------ e. breakdown
def _model_ctx(blocks, m):
    from glmmrmcml_amd import api
    Q = cl.total_dim(blocks)
    cov, data = cl.layout(blocks)
    y = np.random.default_rng(12).poisson(1.0, size=Q).astype(float)
    ctx = api.Context(cov, data, np.zeros(cov.shape[0]), np.asfortranarray(np.eye(Q)), np.ones((Q, 1), order="F"), y, "poisson", "log")
    u = np.asfortranarray(np.random.default_rng(Q).standard_normal((Q, m)) * ic.SAMPLE_SCALE)
    ctx.set_u(u)
    return ctx, u


def _outcome(call):
    """("ok", result) with every number finite, or ("-3", None); anything else fails the test"""
    from glmmrmcml_amd import _lib
    try:
        out = call()
    except _lib.McmlError as e:
        assert e.code == -3, (e.code, str(e))
        return "-3", None
    for a in (out if isinstance(out, tuple) else (out,)):
        assert a is None or np.all(np.isfinite(a)), "a NaN or an infinity with a success code"
    return "ok", out


@pytest.mark.parametrize("name", list(ic.LADDERS))
def test_breakdown_ladder(name):
    """every parameter vector of the ladder through mvn_ll, mvn_ll_grad, mvn_ll_batch (between two good candidates), gen_D(chol=True)
    and update_L: -3 or finite numbers; success where the reference factorises with kappa <= 2e12; after a failure the next
    good call has its earlier bits and the samples are untouched; after a failed update_L the samplers refuse; once a path
    fails it fails on every later rung (COIN's three ranges are three exactly singular matrices, not a ladder: the pivot that
    decides is rounding noise, so each is held to "-3 or finite" on its own)"""
    from glmmrmcml_amd import _lib
    blocks, thetas, good, ordered = ic.LADDERS[name]
    m = 5
    ctx, u = _model_ctx(blocks, m)
    V = np.random.default_rng(3).normal(size=(cl.total_dim(blocks), 2)) * 0.5
    beta = np.array([0.2])
    paths = ("mvn_ll", "mvn_ll_grad", "mvn_ll_batch", "gen_D", "update_L")
    broke = {p: None for p in paths}
    with ctx:
        if good is not None:
            ll0, g0 = ctx.mvn_ll(good), ctx.mvn_ll_grad(good)
            ctx.update_L(good)
            lp0 = ctx.log_prob_grad(beta, 1.0, V)
        for i, th in enumerate(thetas):
            must = ic.must_succeed(blocks, th)
            calls = {"mvn_ll": lambda: ctx.mvn_ll(th), "mvn_ll_grad": lambda: ctx.mvn_ll_grad(th),
                     "gen_D": lambda: ctx.gen_D(th, chol=True), "update_L": lambda: ctx.update_L(th)}
            for p in paths:
                if p == "mvn_ll_batch":
                    cand = np.array([good if good is not None else th, th, good if good is not None else th])
                    vals = ctx.mvn_ll_batch(cand)
                    assert not np.any(np.isinf(vals)), vals
                    if good is not None:
                        assert vals[0] == vals[2] and np.isfinite(vals[0]), vals
                    what = "-3" if np.isnan(vals[1]) else "ok"
                else:
                    what, _ = _outcome(calls[p])
                if must:
                    assert what == "ok", (name, i, th, p, "the reference factorises this rung with kappa <= 2e12")
                if what == "-3" and broke[p] is None:
                    broke[p] = i
                if ordered:
                    assert (broke[p] is None) == (what == "ok"), (name, p, "failed at rung %s, succeeded at rung %d" % (broke[p], i), th)
                if what == "-3":
                    assert np.array_equal(ctx.get_u(), u)
                    if p == "update_L":
                        for sampler in (lambda: ctx.log_prob_grad(beta, 1.0, V),
                                        lambda: ctx.hmc_sample(beta, 1.0, 1, 1, 0.1, 3, 0.8, 1)):
                            with pytest.raises(_lib.McmlError) as e:
                                sampler()
                            assert "L not set" in str(e.value), str(e.value)
                    if good is not None:
                        assert ctx.mvn_ll(good) == ll0 and _same(ctx.mvn_ll_grad(good), g0)
                        if p == "update_L":
                            ctx.update_L(good)
                            lp = ctx.log_prob_grad(beta, 1.0, V)
                            assert np.array_equal(lp[0], lp0[0]) and np.array_equal(lp[1], lp0[1])
        print("%s first fails at rung (of %d): %s" % (name, len(thetas), ", ".join(
            "%s %s" % (p, "never" if broke[p] is None else "%d (theta %s)" % (broke[p], thetas[broke[p]])) for p in paths)))


# ------------------------------------------------------------------------------------------------ f. the workspace at E6
def test_workspace_at_E6_eager_and_graphed():
    """SQ300 at E6, m = 17, through the checks of test_gpu_mvn_workspace.py: six calls at one theta (eager, eager, captured,
    replays), every fetch within the rung's factor constant on factor and solved rows, and with the bits of the first"""
    name, rung, m = "SQ300", "E6", 17
    th = ic.theta(name, rung)
    C = ic.constants(rung)["factor"]
    D, bb = cr.build_D(ic.CASES[name][0], th)
    u = ic.sample_matrix(name)[:, :m]
    with _ctx(name, m) as ctx:
        first = None
        for call in range(6):
            ctx.mvn_ll(th)
            L, X, dims = ctx.mvn_workspace(-1)
            assert dims[:3] == (300, 304, m), dims
            L = np.tril(L)
            if first is None:
                first = (L, X)
                (wf, af), (wr, ar) = cr.factor_ratio(D, L, bb), cr.rows_ratio(L, X, u.T)
                print("SQ300 E6 workspace: factor %.3g at %s, rows %.3g at %s (C %.3g)" % (wf, af, wr, ar, C))
                assert wf <= C and wr <= C, (wf, af, wr, ar)
            assert np.array_equal(L, first[0]) and np.array_equal(X, first[1]), "call %d" % call
