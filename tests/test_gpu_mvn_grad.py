"""The analytic score of mvn_ll on the device (csrc/mvn_grad.h) against the long-double reference of
tests/mvn_grad_reference.py, on the covariance layouts of tests/cov_layouts.py: MIXED (Q = 522: diagonal, one-wave and
blocked-Cholesky blocks, odd dimensions 150 and 289 past one and two panels, parameter 1 shared by all three kinds),
TWO_LARGE_A / _B (two large blocks of different size in either order: the inverted diagonal blocks of one factorisation
must not serve the other block's solves) and EDGE32 (the 32 / 33 boundary).

Tolerance of the gradient: bound_k = 2^-52 kappa mag_k (the helper's docstring), of which the float64 numpy twin of the
same algorithm uses at most 0.0101 (test_mvn_grad_reference_cpu.py) and the device, measured, at most 0.016 (TWO_LARGE_B,
m = 1); the value: the 1e-10 relative mvn_ll is pinned to.

mag_k carries |inv(D)|, so bound_k is loose by about kappa once kappa is large (the device sits at 1e-9 to 1e-11 of it at
kappa >= 1e9): tests/test_gpu_illcond.py holds the gradient to C 2^-52 kappa |ref grad_k| as well, on blocks up to
kappa = 2e12."""
import functools

import numpy as np
import pytest

import cov_layouts as cl
import mvn_grad_reference as gr

pytestmark = pytest.mark.gpu
RTOL = 1e-10
EPS = 2.0 ** -52
CASES = ([("MIXED", m) for m in (1, 17, 64, 65, 129, 130)] + [("TWO_LARGE_A", m) for m in (1, 17, 40)]
         + [("TWO_LARGE_B", m) for m in (1, 17, 40)] + [("EDGE32", m) for m in (1, 64, 65, 70)])
ONE_EACH = [("MIXED", 65), ("TWO_LARGE_A", 17), ("TWO_LARGE_B", 40), ("EDGE32", 70)]
RHO = {"MIXED": cl.MIXED_RHO, "TWO_LARGE_A": cl.TWO_LARGE_RHO, "TWO_LARGE_B": cl.TWO_LARGE_RHO}


@functools.lru_cache(maxsize=None)
def _wire(name):
    cov, data = cl.layout(cl.LAYOUTS[name][0])
    return cov, data, np.zeros(cov.shape[0])


def _ctx(name, m):
    from glmmrmcml_amd import api
    ctx = api.Context(*_wire(name))
    ctx.set_u(cl.sample_matrix(name)[:, :m])
    return ctx


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("name,m", CASES)
def test_gradient_and_value_against_the_reference(name, m):
    """every theta of thetas(name), unweighted and with weights that contain exact zeros and do not sum to 1: each entry of
    the gradient within bound_k of the reference, the value within 1e-10; unweighted, the value is mvn_ll's to the bit; a
    repeated call gives the same bits"""
    worst = 0.0
    with _ctx(name, m) as ctx:
        for ti, theta in enumerate(cl.thetas(name)):
            for w in (None, gr.weights(m)):
                value, grad = ctx.mvn_ll_grad(theta, w)
                rv, rg, mag, kappa = gr.reference(name, ti, m, w)
                ratio = np.abs(grad.astype(np.longdouble) - rg) / (EPS * kappa * mag)
                worst = max(worst, float(ratio.max()))
                print("%s m=%d theta %d %s: |grad - ref| / bound = %s, value rel %.2e" % (
                    name, m, ti, "weighted" if w is not None else "unweighted",
                    np.array2string(ratio.astype(float), precision=3), abs(value - rv) / abs(rv)))
                assert (ratio <= 1.0).all(), (name, m, ti, w is not None, ratio)
                assert abs(value - rv) <= RTOL * abs(rv), (value, rv)
                if w is None:
                    assert value == ctx.mvn_ll(theta)
                assert _same(ctx.mvn_ll_grad(theta, w), (value, grad))
    print("%s m=%d: largest |grad - ref| / bound = %.3g" % (name, m, worst))


# ------------------------------------------------------------------------------------------------ call history
@pytest.mark.parametrize("name,m", ONE_EACH)
def test_same_bits_whatever_came_before(name, m):
    """the gradient at one theta before and after mvn_ll at another theta, a batched round, a gradient elsewhere, and
    against a fresh context's and the stateless export's"""
    from glmmrmcml_amd import api
    thetas = cl.thetas(name)
    w = gr.weights(m)
    with _ctx(name, m) as ctx:
        first = ctx.mvn_ll_grad(thetas[0])
        first_w = ctx.mvn_ll_grad(thetas[0], w)
        ctx.mvn_ll(thetas[1])
        assert _same(ctx.mvn_ll_grad(thetas[0]), first)
        ctx.mvn_ll_batch(np.array(thetas))
        assert _same(ctx.mvn_ll_grad(thetas[0], w), first_w)
        ctx.mvn_ll_grad(thetas[2], w)
        assert _same(ctx.mvn_ll_grad(thetas[0]), first)
    with _ctx(name, m) as ctx:
        assert _same(ctx.mvn_ll_grad(thetas[0], w), first_w)
    u = cl.sample_matrix(name)[:, :m]
    assert _same(api.mvn_ll_grad(*_wire(name), thetas[0], u), first)
    assert _same(api.mvn_ll_grad(*_wire(name), thetas[0], u, w), first_w)


def _model_ctx():
    from glmmrmcml_amd import api
    Q = cl.total_dim(cl.MIXED)
    rng = np.random.default_rng(12)
    Z = np.asfortranarray(np.vstack([np.eye(Q), np.eye(Q)]))
    X = np.ones((2 * Q, 1), order="F")
    y = rng.poisson(1.0, size=2 * Q).astype(float)
    V = rng.normal(size=(Q, 4)) * 0.5
    ctx = api.Context(*_wire("MIXED"), Z, X, y, "poisson", "log")
    ctx.set_u(cl.sample_matrix("MIXED")[:, :17])
    return ctx, V


def test_model_context_update_L_in_between_and_log_prob_grad_untouched():
    """on a context with a model: the gradient repeats bit for bit after update_L at another theta, and the sampler's
    log_prob_grad returns the same bits with and without a gradient call in between (L and the operator are not touched)"""
    thetas = cl.thetas("MIXED")
    beta = np.array([0.2])
    ctx, V = _model_ctx()
    with ctx:
        ctx.update_L(thetas[0])
        lp0, G0 = ctx.log_prob_grad(beta, 1.0, V)
        first = ctx.mvn_ll_grad(thetas[1])
        lp1, G1 = ctx.log_prob_grad(beta, 1.0, V)
        assert np.array_equal(lp0, lp1) and np.array_equal(G0, G1)
        ctx.update_L(thetas[2])
        assert _same(ctx.mvn_ll_grad(thetas[1]), first)
    with _ctx("MIXED", 17) as plain:
        assert _same(plain.mvn_ll_grad(thetas[1]), first)


# ------------------------------------------------------------------------------------------------ a query
@pytest.mark.parametrize("name,m", ONE_EACH)
def test_the_call_is_a_query(name, m):
    """mvn_ll(theta_2) and mvn_workspace() return the same bits with and without a gradient call in between, and after
    mvn_ll_grad(theta) the workspace is what mvn_ll(theta) leaves: the factor (the lower triangle of the array; the strict
    upper triangle is never read by the factorisation or the solves and comes back changed, csrc/chol.hip potrf_lower, so it
    follows the number of calls before it; test_gpu_mvn_workspace.py compares np.tril too) and the solved sample rows"""
    thetas = cl.thetas(name)

    def workspace(ctx):
        L, X, dims = ctx.mvn_workspace()
        return np.tril(L), X, dims

    with _ctx(name, m) as ctx:
        ctx.mvn_ll(thetas[1])
        v_without = ctx.mvn_ll(thetas[2])
        L_without, X_without, dims_without = workspace(ctx)
    with _ctx(name, m) as ctx:
        ctx.mvn_ll(thetas[1])
        ctx.mvn_ll_grad(thetas[1], gr.weights(m))
        v_with = ctx.mvn_ll(thetas[2])
        L_with, X_with, dims_with = workspace(ctx)
        assert v_with == v_without and dims_with == dims_without
        assert np.array_equal(L_with, L_without), int((L_with != L_without).sum())
        assert np.array_equal(X_with, X_without)
        ctx.mvn_ll_grad(thetas[2])
        L_after, X_after, dims_after = workspace(ctx)
        assert dims_after == dims_without and np.array_equal(L_after, L_without) and np.array_equal(X_after, X_without)


# ------------------------------------------------------------------------------------------------ failure
@pytest.mark.parametrize("name,m", [("MIXED", 65), ("TWO_LARGE_A", 17), ("TWO_LARGE_B", 40)])
def test_not_positive_definite_raises_and_changes_nothing(name, m):
    """the AR1 parameter past 1: McmlError -3 (MIXED: raised in the one-wave kernel; TWO_LARGE: in the blocked
    factorisation of the second / first block); the next good calls return the earlier bits and the samples are untouched"""
    from glmmrmcml_amd import _lib
    thetas = cl.thetas(name)
    bad = thetas[0].copy(); bad[RHO[name]] = 1.5
    w = gr.weights(m)
    with _ctx(name, m) as ctx:
        u0 = ctx.get_u()
        good, good_w, ll = ctx.mvn_ll_grad(thetas[0]), ctx.mvn_ll_grad(thetas[0], w), ctx.mvn_ll(thetas[0])
        for weights in (None, w):
            with pytest.raises(_lib.McmlError) as e:
                ctx.mvn_ll_grad(bad, weights)
            assert e.value.code == -3
            assert _same(ctx.mvn_ll_grad(thetas[0]), good) and _same(ctx.mvn_ll_grad(thetas[0], w), good_w)
            assert ctx.mvn_ll(thetas[0]) == ll
        assert np.array_equal(ctx.get_u(), u0)


def test_refusals():
    """weights of the wrong length, negative or NaN, and a context without samples: the argument error, and the context
    goes on as before"""
    from glmmrmcml_amd import api, _lib
    theta = cl.EDGE32_THETA
    m = 5
    u = cl.sample_matrix("EDGE32")[:, :m]
    with api.Context(*_wire("EDGE32")) as ctx:
        with pytest.raises(_lib.McmlError) as e:
            ctx.mvn_ll_grad(theta)
        assert e.value.code == -1 and "no samples" in str(e.value)
        with pytest.raises(_lib.McmlError) as e2:
            ctx.mvn_ll(theta)
        assert e2.value.code == e.value.code and str(e2.value).split(": ", 1)[1] == str(e.value).split(": ", 1)[1]
        ctx.set_u(u)
        good = ctx.mvn_ll_grad(theta, np.ones(m))
        for w in (np.ones(m + 1), np.ones(m - 1), np.r_[np.ones(m - 1), -0.5], np.r_[np.nan, np.ones(m - 1)],
                  np.r_[np.ones(m - 1), np.inf]):
            with pytest.raises(_lib.McmlError) as e:
                ctx.mvn_ll_grad(theta, w)
            assert e.value.code == -1, w
            with pytest.raises(_lib.McmlError) as e:
                api.mvn_ll_grad(*_wire("EDGE32"), theta, u, w)
            assert e.value.code == -1, w
        assert _same(ctx.mvn_ll_grad(theta, np.ones(m)), good)
        # unit weights are m times the default
        value, grad = ctx.mvn_ll_grad(theta)
        assert abs(good[0] - m * value) <= 1e-13 * abs(good[0]) and np.allclose(good[1], m * grad, rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------ the device's own objective
@pytest.mark.parametrize("name,m", ONE_EACH)
def test_central_differences_of_the_device_objective(name, m):
    """central differences of mvn_ll_batch at theta_k (1 +- 1e-5) against the device gradient: within 1e-9 mag_k (the
    truncation bounded in test_mvn_grad_reference_cpu.py) + 2 * 1e-10 |l| / h (two values, each pinned to 1e-10 relative)"""
    theta = cl.thetas(name)[0]
    R = len(theta)
    cand = np.repeat(theta[None, :], 2 * R, axis=0)
    for k in range(R):
        cand[2 * k, k] = theta[k] * (1 + 1e-5)
        cand[2 * k + 1, k] = theta[k] * (1 - 1e-5)
    with _ctx(name, m) as ctx:
        value, grad = ctx.mvn_ll_grad(theta)
        ll = ctx.mvn_ll_batch(cand)
    _, _, mag, _ = gr.reference(name, 0, m, None)
    for k in range(R):
        h = 1e-5 * theta[k]
        fd = (ll[2 * k] - ll[2 * k + 1]) / (cand[2 * k, k] - cand[2 * k + 1, k])
        tol = 1e-9 * float(mag[k]) + 2 * 1e-10 * abs(value) / h
        print("%s parameter %d: fd %.12g, gradient %.12g, difference %.3g, tolerance %.3g" % (name, k, fd, grad[k], abs(fd - grad[k]), tol))
        assert abs(fd - grad[k]) <= tol, (name, k, fd, grad[k], tol)
