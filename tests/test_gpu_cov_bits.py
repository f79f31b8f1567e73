"""The bits of the covariance layer, pinned where its copied code was given one home: the walk over a block's terms
(csrc/cov_entry.h), the small block built, factorised and solved in LDS and the 64 x 16 walk over a lower triangle
(csrc/cov_block.h), which mvn_ll, its score (csrc/mvn_grad.h), the prediction (csrc/predict.hip) and the information of theta
(csrc/theta_info.hip) share.  The reference tests judge each result within a bound; they cannot see a last digit that moves
when a sum is regrouped or a helper evaluates an expression in another order.  Here the SHA-256 of what a call returns is
compared with tests/golden/cov_bits.json, recorded from the library of the commit named there (tests/golden/make_cov_bits.py:
never from the code under test).  tests/golden/dense_la_bits.json pins mvn_ll, mvn_ll_batch and gen_D(chol=True) already.

  gen_D_mixed     Context.gen_D(theta, chol=False) on MIXED (Q = 522): the mirrored build, dimensions 150 / 33 / 289 with and
                  without a border, the diagonal fill
  grad_*          Context.mvn_ll_grad, value and gradient: MIXED with 70 weighted columns (small blocks past one 64-column
                  pass) and 3 unweighted ones, all three block kinds; EDGE32 (the 32 / 33 boundary); TWO_LARGE_A (two large
                  blocks in a row); TEN_SLOTS (a small and a large block of ten slots each: the second pass of the slot window
                  in k_small_grad and k_grad_reduce_large)
  predict_*       Context.predict_re(means=True) on the cases of kriging_reference, summary and means: the diagonal kernel,
                  the small one (65 new points, 70 columns: second tiles both ways), the large path
  tinfo_*         Context.theta_information on the cases of theta_information_reference: k_ti_build_dD on every block kind
                  (mixed, geo150), k_ti_comp with two slots in one block (stepped_wedge_7x8x3) and the sigma row
The input hashes are asserted first: a changed numpy stream fails there instead of comparing different problems.

TEN_SLOTS is held against the long-double reference as well (test_ten_slots_against_the_reference): no layout of LAYOUTS has a
block with more than GRAD_SLOTS = 8 slots, so nothing else runs the second pass of the slot window."""
import hashlib
import json
import os

import numpy as np
import pytest

import cov_layouts as cl
import kriging_reference as kr
import mvn_grad_reference as gr
import theta_information_reference as tr

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cov_bits.json")
ENV = ("GLMMR_MCML_PREDICT_CHUNK", "GLMMR_MCML_PREDICT_PHASES", "GLMMR_MCML_CHOL_GRAPH", "GLMMR_MCML_GEMM", "GLMMR_MCML_ZL")
EPS = 2.0 ** -52
RTOL = 1e-10             # test_gpu_mvn_grad.py's bound on the value


def sha256(*arrays):
    """of the arrays' values as float64 in column-major order, one after the other"""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.asarray(a, dtype=np.float64).tobytes(order="F"))
    return h.hexdigest()


def _layout(name):
    """(blocks, theta, every sample column) of a named layout or of TEN_SLOTS"""
    if name == "TEN_SLOTS":
        return cl.TEN_SLOTS, cl.TEN_SLOTS_THETA, cl.samples(cl.TEN_SLOTS, 70, cl.TEN_SLOTS_SEED)
    return cl.LAYOUTS[name] + (cl.sample_matrix(name),)


def _cov_context(blocks, u=None):
    from glmmrmcml_amd import api
    cov, data = cl.layout(blocks)
    ctx = api.Context(cov, data, np.zeros(cov.shape[0]))
    if u is not None:
        ctx.set_u(u)
    return ctx, (cov, data)


def gen_D_mixed(mp):
    ctx, wire = _cov_context(cl.MIXED)
    with ctx:
        D = ctx.gen_D(cl.MIXED_THETA, chol=False)
    assert D.shape == (522, 522)
    return dict(inputs=sha256(*wire, cl.MIXED_THETA), gen_D=sha256(D))


def grad(name, m, weighted):
    def run(mp):
        blocks, theta, u = _layout(name)
        u = u[:, :m]
        w = gr.weights(m) if weighted else None
        ctx, wire = _cov_context(blocks, u)
        with ctx:
            value, g = ctx.mvn_ll_grad(theta, w)
        return dict(inputs=sha256(*wire, theta, u, [] if w is None else w), value=sha256([value]), grad=sha256(g))
    return run


def predict(key):
    def run(mp):
        c = kr.case(key)
        assert c["chunk"] is None
        ctx, wire = _cov_context(c["blocks"], c["u"])
        with ctx:
            got = ctx.predict_re(c["theta"], c["newdata"], means=True)
        new = [x for x in c["newdata"] if x is not None]
        return dict(inputs=sha256(*wire, c["theta"], c["u"], c["counts"], *new),
                    summary=sha256(got["mean"], got["cond_var"], got["sample_var"]), means=sha256(got["means"]))
    return run


def tinfo(key):
    def run(mp):
        from glmmrmcml_amd import api
        c = tr.case(key)
        y = np.zeros(c["X"].shape[0])                                  # the query does not read y
        with api.Context(c["cov"], c["data"], c["eff_range"], c["Z"], c["X"], y, c["family"], c["link"]) as ctx:
            got = ctx.theta_information(c["beta"], c["var_par"], c["theta"])["information"]
            assert ctx.theta_information_plan()["op"] == c["op"]
        return dict(inputs=sha256(c["Z"], c["X"], c["cov"], c["data"], c["eff_range"], c["beta"], c["theta"], [c["var_par"]]),
                    information=sha256(got))
    return run


CASES = {
    "gen_D_mixed": gen_D_mixed,
    "grad_MIXED_m70_w": grad("MIXED", 70, True),
    "grad_MIXED_m3": grad("MIXED", 3, False),
    "grad_EDGE32_m70": grad("EDGE32", 70, False),
    "grad_TWO_LARGE_A_m17": grad("TWO_LARGE_A", 17, False),
    "grad_TEN_SLOTS_m7_w": grad("TEN_SLOTS", 7, True),
    "grad_TEN_SLOTS_m70": grad("TEN_SLOTS", 70, False),
    "predict_MIXED_m3": predict("MIXED_m3"),
    "predict_MIXED_m70": predict("MIXED_m70"),
    "predict_EDGE32": predict("EDGE32"),
    "tinfo_mixed": tinfo("mixed"),
    "tinfo_geo150": tinfo("geo150"),
    "tinfo_stepped_wedge_7x8x3": tinfo("stepped_wedge_7x8x3"),
    "tinfo_family-gaussian-identity": tinfo("family-gaussian-identity"),
}


def digests(name, mp):
    """{"inputs": .., ...} of a case through the library that is loaded; mp: a pytest.MonkeyPatch"""
    for k in ENV:
        mp.delenv(k, raising=False)
    return CASES[name](mp)


@pytest.mark.parametrize("name", list(CASES))
def test_cov_bits_are_the_recorded_ones(name, monkeypatch):
    with open(FIXTURE) as f:
        want = json.load(f)["cases"][name]
    got = digests(name, monkeypatch)
    assert got["inputs"] == want["inputs"], "the seeded inputs are not the recorded ones (numpy stream changed?)"
    for key in sorted(want):
        print(name, key, got[key])
    for key in sorted(want):
        assert got[key] == want[key], "%s: %s differs from the bits recorded in %s" % (name, key, FIXTURE)
    assert set(got) == set(want)


def ten_slots_ratios():
    """[(m, weighted, worst |grad - ref| / (2^-52 kappa mag_k), |value - ref| / |ref|, a repeated call gives the same bits)]
    through the library that is loaded, m = 7 and 70, weighted and not: test_gpu_mvn_grad.py's criterion"""
    blocks, theta, u70 = _layout("TEN_SLOTS")
    out = []
    for m in (7, 70):
        u = u70[:, :m]
        ctx, _ = _cov_context(blocks, u)
        with ctx:
            for w in (None, gr.weights(m)):
                value, g = ctx.mvn_ll_grad(theta, w)
                again = ctx.mvn_ll_grad(theta, w)
                rv, rg, mag, kappa = gr.score(blocks, theta, u, w)
                ratio = np.abs(g.astype(np.longdouble) - rg) / (EPS * kappa * mag)
                out.append((m, w is not None, float(ratio.max()), float(abs(value - rv) / abs(rv)),
                            bool(again[0] == value and np.array_equal(again[1], g))))
    return out


def test_ten_slots_against_the_reference():
    """ten slots a block, a small and a large one: every gradient entry within 2^-52 kappa mag_k of the long-double reference,
    the value within 1e-10, a repeated call the same bits.  Measured on an MI355X, the library of 7bea038 and the one the
    walk was merged in alike: 0.0045 / 0.0125 of the bound at m = 7 (unweighted / weighted), 0.0037 / 0.0075 at m = 70, the value
    within 2.1e-16"""
    rows = ten_slots_ratios()
    for m, weighted, ratio, rel, same in rows:
        print("TEN_SLOTS m=%d %s: largest |grad - ref| / bound = %.3g, value rel %.2e, repeat identical %s" % (
            m, "weighted" if weighted else "unweighted", ratio, rel, same))
    for m, weighted, ratio, rel, same in rows:
        assert ratio <= 1.0 and rel <= RTOL and same, (m, weighted, ratio, rel, same)
