"""What mvn_ll and mvn_ll_batch leave in their workspace -- the factor of the large block and, below it, the solved sample
rows the fused factorisation carries as `extra` rows -- element by element (glmmr_mcml_dbg_mvn_workspace), on the eager
schedule, on the captured and replayed graph, and on a batch with and without the K = 1024 super-panel regrouping.

Single-block layouts: S-type, gr x ar1 on times 0 .. d-1 with rho = 0.5 (D = sigma^2 rho^|i - j|), and F, a fexp0 block of
300 points.  The reference matrix is cov_layouts.block_matrix in float64; that module's entrywise bound on another float64
evaluation of the same table is added to the factor's residual bound.  Bounds and constants: tests/chol_reference.py.
"""
import numpy as np
import pytest

import chol_reference as cr
import cov_layouts as cl

pytestmark = pytest.mark.gpu

_cache = {}


def _context(block, u):
    from glmmrmcml_amd import api
    cov, data = cl.layout([block])
    ctx = api.Context(cov, data, np.zeros(cov.shape[0]))
    ctx.set_u(u)
    return ctx


def _fetch(ctx, cand, d, m):
    L, X, dims = ctx.mvn_workspace(cand)
    assert dims[:3] == (d, (d + 15) // 16 * 16, m), dims
    return np.tril(L), X


def _check(label, block, theta, u, L, X, C):
    """factor residual against the float64 definition of D (plus its build bound) and |X L' - U'| <= C d u |X| |L'|; the same
    bits are judged once"""
    key = (label[0], tuple(np.ravel(theta)), u.shape, L.tobytes(), X.tobytes())
    if key not in _cache:
        if len(_cache) > 4:
            _cache.clear()
        D, bb = cr.build_D(block, theta)
        _cache[key] = cr.factor_ratio(D, L, bb), cr.rows_ratio(L, X, u.T)
    (wf, af), (wr, ar) = _cache[key]
    print("%s: factor %.4f at %s, rows %.4f at %s" % (label, wf, af, wr, ar))
    assert wf <= C, (label, "factor", wf, af)
    assert wr <= C, (label, "rows", wr, ar)


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), (what, "factor", np.argwhere(a[0] != b[0])[:3])
    assert np.array_equal(a[1], b[1]), (what, "solved rows", np.argwhere(a[1] != b[1])[:3])


LAYOUTS = {"S": (cr.block_S, cr.thetas_S, cr.C_WS), "F": (lambda d: cr.block_F(), lambda k: cr.F_THETAS[:k], cr.C_F)}


@pytest.mark.parametrize("d", cr.WS_EAGER_D)
@pytest.mark.parametrize("m", cr.WS_EAGER_M)
def test_single_evaluation_eager(d, m):
    """up to two panels the factorisation is launched eagerly on one stream: the first large size (33, padded to 48 with an
    identity border), a multiple of 16, one panel plus one row, and the last size before the look-ahead (255 -> 256)"""
    block, theta = cr.block_S(d), cr.thetas_S(1)[0]
    u = cr.samples(d, m)
    with _context(block, u) as ctx:
        ctx.mvn_ll(theta)
        L, X = _fetch(ctx, -1, d, m)
        _check(("S", d, m), block, theta, u, L, X, cr.C_WS)
        ctx.mvn_ll(theta)
        _same(_fetch(ctx, -1, d, m), (L, X), "second call")


@pytest.mark.parametrize("kind,d", [("S", 300), ("F", 300), ("S", 1153)])
def test_single_evaluation_graph_replays_the_eager_bits(kind, d):
    """six calls at one theta -- eager, eager, captured, then replays under calibration -- one at another theta and one back:
    every fetch meets the bounds, and every fetch at the first theta has the bits of the first (eager) one, as the comment
    above potrf_la2_capture promises"""
    make, thetas, C = LAYOUTS[kind]
    block, th = make(d), thetas(2)
    m = cr.WS_M
    u = cr.samples(d, m)
    with _context(block, u) as ctx:
        first = None
        for call in range(6):
            ctx.mvn_ll(th[0])
            got = _fetch(ctx, -1, d, m)
            _check((kind, d, "call %d" % call), block, th[0], u, got[0], got[1], C)
            first = got if first is None else first
            _same(got, first, "call %d" % call)
        ctx.mvn_ll(th[1])
        other = _fetch(ctx, -1, d, m)
        _check((kind, d, "other theta"), block, th[1], u, other[0], other[1], C)
        assert not np.array_equal(other[0], first[0])
        ctx.mvn_ll(th[0])
        _same(_fetch(ctx, -1, d, m), first, "back at the first theta")


@pytest.mark.parametrize("kind,k,d", [("S", k, d) for k, d in cr.WS_BATCH] + [("F", 2, 300), ("F", 8, 300)])
def test_batch(kind, k, d):
    """every candidate of a batch meets the bounds; up to d = 1152 (no super-panel regrouping) its factor and solved rows are,
    bit for bit, what a single evaluation at that theta leaves.  1153 regroups with one super-panel, 2200 with two."""
    make, thetas, C = LAYOUTS[kind]
    block, th = make(d), thetas(k)
    m = cr.WS_M
    u = cr.samples(d, m)
    with _context(block, u) as ctx:
        ctx.mvn_ll_batch(th)
        got = [_fetch(ctx, j, d, m) for j in range(k)]
        for j in range(k):
            _check((kind, d, "candidate %d of %d" % (j, k)), block, th[j], u, got[j][0], got[j][1], C)
        if d <= 1152:
            for j in range(k):
                ctx.mvn_ll(th[j])
                _same(got[j], _fetch(ctx, -1, d, m), "candidate %d against its single evaluation" % j)


def test_batch_with_a_candidate_outside_the_positive_definite_region():
    """an AR1 parameter of 1.5 in the middle: that candidate is NaN, its neighbours' workspaces stay within the bounds"""
    d, m = 129, cr.WS_M
    block, u = cr.block_S(d), cr.samples(d, m)
    th = cr.thetas_S(3)
    th[1, 1] = 1.5
    with _context(block, u) as ctx:
        vals = ctx.mvn_ll_batch(th)
        assert np.isnan(vals[1]) and np.isfinite(vals[0]) and np.isfinite(vals[2])
        for j in (0, 2):
            L, X = _fetch(ctx, j, d, m)
            _check(("S", d, "neighbour %d" % j), block, th[j], u, L, X, cr.C_WS)


def test_workspace_hook_needs_a_call_before_it():
    from glmmrmcml_amd import _lib
    with _context(cr.block_S(48), cr.samples(48, 2)) as ctx:
        with pytest.raises(_lib.McmlError):
            ctx.mvn_workspace(-1)
        ctx.mvn_ll(cr.thetas_S(1)[0])
        ctx.mvn_workspace(-1)
        with pytest.raises(_lib.McmlError):
            ctx.mvn_workspace(0)
