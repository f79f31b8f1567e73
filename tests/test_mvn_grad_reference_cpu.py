"""The reference of the mvn_ll score (tests/mvn_grad_reference.py) pinned without a GPU: against central differences of
the definition in long double, its float64 twin against it in units of the bound the GPU test uses, the shared-parameter
and gr rules by hand, and ModelMCML's theta_score wiring with a recording backend."""
import numpy as np
import pytest

import cov_layouts as cl
import mvn_grad_reference as gr
from test_model_caller import FakeBackend, _model

LD = np.longdouble
NAMES = sorted(cl.LAYOUTS)
EPS = 2.0 ** -52


# ------------------------------------------------------------------------------------------------ 1. central differences
@pytest.mark.parametrize("name", NAMES)
def test_reference_against_central_differences_of_the_definition(name):
    """d/d theta_k of sum_j w_j ll_j(theta), ll from cov_layouts.definition_columns in long double, by central differences
    with h = 1e-5 theta_k: within 1e-9 mag_k of the reference (the difference's own truncation error, ~ h^2 f''' / 6, is
    what remains: 1.7e-10 mag_k at the layouts' first theta), for m = 1 and 17, with and without weights"""
    blocks = cl.LAYOUTS[name][0]
    u = cl.sample_matrix(name)[:, :17]
    worst = 0.0
    for ti, theta in enumerate(cl.thetas(name)):
        diffs = []
        for k in range(len(theta)):
            h = 1e-5 * theta[k]
            tp, tm = theta.copy(), theta.copy()
            tp[k] += h; tm[k] -= h
            llp = cl.definition_columns(blocks, tp, u)[2]
            llm = cl.definition_columns(blocks, tm, u)[2]
            diffs.append((llp - llm) / (LD(tp[k]) - LD(tm[k])))          # one value per column
        diffs = np.array(diffs)
        for m in (1, 17):
            for w in (None, gr.weights(m)):
                value, grad, mag, kappa = gr.reference(name, ti, m, w)
                wl = np.full(m, LD(1) / m) if w is None else w.astype(LD)
                fd = (diffs[:, :m] * wl).sum(1)
                ratio = np.abs(fd - grad) / mag
                worst = max(worst, float(ratio.max()))
                assert (ratio <= 1e-9).all(), (name, ti, m, w is not None, ratio)
                assert (mag >= np.abs(grad)).all() and kappa < 1e4
        value, _, _, _ = gr.reference(name, ti, 17, None)
        want = cl.definition_columns(blocks, theta, u)[2].sum() / 17
        assert abs(value - want) <= 1e-17 * abs(want), (name, ti, value, want)
    print("%s: largest |central difference - reference| / mag = %.3g" % (name, worst))


# ------------------------------------------------------------------------------------------------ 2. the float64 twin
@pytest.mark.parametrize("name", NAMES)
def test_float64_twin_within_a_twentieth_of_the_bound(name):
    """the same algorithm in float64 numpy against the long-double reference, in units of bound_k = 2^-52 kappa mag_k:
    <= 0.05 for every theta, m in {1, 17, 65} (40 where the layout has 40 columns), with and without weights.  This is
    what fixes the GPU tolerance (one bound_k) without looking at the code under test"""
    worst = worst_nokappa = 0.0
    for ti in range(3):
        for m in (1, 17, min(65, cl.COLUMNS[name])):
            for w in (None, gr.weights(m)):
                value, grad, mag, kappa = gr.reference(name, ti, m, w)
                v64, g64, mag64, kappa64 = gr.twin(name, ti, m, w)
                err = np.abs(g64.astype(LD) - grad) / (EPS * mag)
                worst = max(worst, float(err.max()) / kappa)
                worst_nokappa = max(worst_nokappa, float(err.max()))
                assert (err <= 0.05 * kappa).all(), (name, ti, m, w is not None, err / kappa)
                assert abs(v64 - value) <= 1e-12 * abs(value)
                assert np.allclose(mag64, mag.astype(np.float64), rtol=1e-9) and abs(kappa64 - kappa) <= 1e-6 * kappa
    print("%s: twin's largest error = %.3g bound, %.3g units of 2^-52 mag" % (name, worst, worst_nokappa))


# ------------------------------------------------------------------------------------------------ 3. by hand
def _hand_blocks(same_group):
    x = [[1.0], [1.0]] if same_group else [[1.0], [2.0]]
    return [(1, [(cl.GR, [[1.0]], 0)]),
            (2, [(cl.GR, x, 0), (cl.FEXP0, [[0.0], [0.3]], 1)])]


def test_shared_parameter_and_gr_rule_by_hand():
    """3 x 3: a diagonal block and a dense block that share parameter 0.  With the dense block's gr term on two different
    groups its off-diagonal entries are 0 and contribute nothing -- D is theta_0^2 I and theta_1 drops out; on one group the
    block is theta_0^2 [[1, e], [e, 1]], e = exp(-0.3 / theta_1), differentiated by hand.  The reference differentiates the D
    the definition builds, whose entries are float64 roundings (theta_0^2 and e carry up to 2 units of 2^-52 each, the
    2 x 2 inverse magnifies them by 1 / (1 - e^2) < 2); the hand formulas use the exact e: 16 units of 2^-52 mag_k"""
    HAND = 16 * EPS
    theta = np.array([0.7, 0.4])
    u = np.array([[0.3, -0.2, 0.5], [0.1, 0.4, -0.6], [-0.25, 0.15, 0.35]])
    t0, t1 = LD(theta[0]), LD(theta[1])
    ul = u.astype(LD)
    for w in (None, np.array([0.5, 0.0, 1.25])):
        wl = np.full(3, LD(1) / 3) if w is None else w.astype(LD)
        # independent rows
        value, grad, mag, _ = gr.score(_hand_blocks(False), theta, u, w)
        want0 = (wl * ((ul * ul).sum(0) / t0 ** 3 - 3 / t0)).sum()
        assert abs(grad[0] - want0) <= HAND * mag[0] and grad[1] == 0 and mag[1] == 0, (grad, want0)
        # correlated pair
        value, grad, mag, _ = gr.score(_hand_blocks(True), theta, u, w)
        e = np.exp(-LD(0.3) / t1)
        s = ul[1] ** 2 - 2 * e * ul[1] * ul[2] + ul[2] ** 2
        quad = s / (t0 ** 2 * (1 - e ** 2))
        d0 = (ul[0] ** 2 / t0 ** 3 - 1 / t0) + (-2 / t0 + quad / t0)
        de = e / (1 - e ** 2) - LD(0.5) * ((-2 * ul[1] * ul[2]) * (1 - e ** 2) + 2 * e * s) / (t0 ** 2 * (1 - e ** 2) ** 2)
        d1 = de * e * LD(0.3) / t1 ** 2
        assert abs(grad[0] - (wl * d0).sum()) <= HAND * mag[0], (grad[0], (wl * d0).sum())
        assert abs(grad[1] - (wl * d1).sum()) <= HAND * mag[1], (grad[1], (wl * d1).sum())
        ll = (-LD(0.5) * cl.LOG_2PI - np.log(t0) - ul[0] ** 2 / (2 * t0 ** 2)
              - cl.LOG_2PI - LD(0.5) * np.log(t0 ** 4 * (1 - e ** 2)) - quad / 2)
        assert abs(value - (wl * ll).sum()) <= HAND * np.abs(wl * ll).sum()


# ------------------------------------------------------------------------------------------------ 4. ModelMCML wiring
class ScoreBackend(FakeBackend):
    def mvn_ll_grad(self, *a, **k):
        self._rec("mvn_ll_grad", a, k)
        return -1.5, np.array([0.25, -0.5])


def test_theta_score_is_one_stateless_call_at_the_final_estimate():
    d, be0, m = _model("binomial")
    be = ScoreBackend(be0.P, be0.R, be0.Q)
    m._be = be
    fit = m.MCML(d["y"], verbose=False, theta_score=True)
    calls = [c for c in be.calls if c[0] == "mvn_ll_grad"]
    assert len(calls) == 1 and be.calls[-1][0] == "mvn_ll_grad"
    _, a, k = calls[0]
    assert a[0] is m.cov and a[1] is m.data and a[2] is m.eff_range and not k
    P = m.X.shape[1]
    assert np.array_equal(a[3], fit["theta"][P:P + 2]) and np.array_equal(a[3], np.full(2, 0.2))
    assert a[4] is fit["re_samps"] and a[4] is be.u
    assert np.array_equal(fit["theta_score"], [0.25, -0.5]) and np.array_equal(fit.theta_score, [0.25, -0.5])
    assert "Max. |score| of the covariance parameters: 0.5" in str(fit)


def test_without_theta_score_the_backend_is_not_asked():
    d, be, m = _model("binomial")
    assert not hasattr(be, "mvn_ll_grad")                    # touching it would raise
    fit = m.MCML(d["y"], verbose=False)
    assert "theta_score" not in fit and fit.theta_score is None
    assert "score" not in str(fit)
    plain = str(fit)
    be2 = ScoreBackend(be.P, be.R, be.Q)
    m._be = be2
    fit2 = m.MCML(d["y"], verbose=False, theta_score=False)
    assert [c[0] for c in be2.calls] == [c[0] for c in be.calls] and str(fit2) == plain
