"""What test_gpu_drivers_dense.py rests on, checked without a GPU: the stored oracle optima of driver_cases.py are interior
local minima of the oracle's objectives, the points said to have no value have none on the oracle, the CPU twins of the
drivers (the library's bobyqa / bobyqa_batch over the oracle's objective, in theta or log theta as drivers.hip runs them)
land on the stored optima, the loop's second iteration responds continuously to what the first hands it, and the
library's fd_hessian is drivers.optimhess to the bit.

Measured here (golden/driver_golden.json keeps every figure): twins against the stored optima, objective gaps 2e-16 to
2e-14 relative; parameters 7e-9 to 1.5e-7 relative on the batch schedule (widths 3 and 8) and 3e-8 to 7e-8 on the
sequential one, except AR's (8.1e-7, where the run meets rho > 1).  The sequential twin runs on 2n + 1 interpolation points
as f_optim does: on minqa's n + 2 it crept along beta_1 (curvature 26 against 4352 for the range) in steps of the final
radius and ended between 4e-8 and 1.9e-6 from the optimum on DG and DP, depending on the rounding of the objective (2e-16
relative noise, ten seeds); on 2n + 1 the same ten seeds end within 4e-7.  u of iteration 2 moves by 1.8e-6 to 2.2e-6 under
a 2e-6 relative change."""
import ctypes as C

import numpy as np
import pytest

import driver_cases as dc


def _theta(name):
    g = dc.golden()
    if name in g["simlik"]:
        return np.array(g["simlik"][name]["x"][dc.case(name)["P"]:])
    return np.array(g["optim"][name]["theta"])


@pytest.mark.parametrize("name", dc.SIMLIK + dc.OPTIM)
def test_stored_optimum_is_an_interior_local_minimum(orc, name):
    th = _theta(name)
    assert np.all(th > 1e-3)
    if name in ("AR", "SW80", "SW95"):
        assert th[-1] < 0.99                                   # the AR1 parameter
    if name in dc.SIMLIK:
        f, x = dc.F_obj(name), np.array(dc.golden()["simlik"][name]["x"])
        assert f(x) == dc.golden()["simlik"][name]["F"]
    else:
        f, x = dc.model(name).D_obj(dc.case(name)["u"]), th
        assert f(x) == dc.golden()["optim"][name]["D"]
    rng = np.random.default_rng(sum(map(ord, name)))
    for _ in range(8):
        assert f(x) <= f(x * (1 + 1e-4 * rng.uniform(-1, 1, x.size)))


def test_points_without_a_value_have_none_on_the_oracle(orc):
    d = dc.case("AR")
    th = dc.ar_first_round_point()
    assert th[2] > 1.15
    with pytest.raises(RuntimeError, match="rc=-3"):
        orc.mvn_ll(d["cov"], d["data"], d["eff_range"], th, d["u"])
    assert dc.F_obj("AR")(np.r_[d["start"][:2], th]) == np.inf


@pytest.mark.parametrize("name", dc.SIMLIK)
@pytest.mark.parametrize("width", dc.WIDTHS)
def test_simlik_twin_lands_on_the_stored_optimum(orc, name, width):
    g = dc.golden()["simlik"][name]
    x, f, nf, calls = dc.simlik_twin(name, width)
    eb, et = dc.par_err(x, g["x"], dc.case(name)["P"])
    print("%s width %d: nf %d, F gap %.2e, beta %.2e, theta %.2e" % (name, width, nf, (f - g["F"]) / abs(g["F"]), eb, et))
    assert f <= g["F"] + dc.F_BOUND * abs(g["F"])
    assert max(eb, et) <= dc.par_bound(name, width)
    stored = max(g["twin"][str(width)]["beta_err"], g["twin"][str(width)]["theta_err"])
    assert dc.par_bound(name, width) == (dc.PAR_BOUND if stored <= dc.PAR_BOUND else 3 * stored)
    if name == "AR":                                           # both schedules step to rho > 1 on their way
        assert any(not np.isfinite(v) for _, v in calls)
    if name == "DG" and width > 1:                             # a round repeats a range under several scales: the memo's case
        z = np.array([c[0][3] for c in calls])
        assert len(np.unique(z)) < len(z)


@pytest.mark.parametrize("name", dc.OPTIM)
def test_theta_step_twin_lands_on_the_stored_optimum(orc, name):
    g = dc.golden()["optim"][name]
    d = dc.case(name)
    th, f, nf, calls = dc.optim_twin(name)
    et = dc.par_err(th, g["theta"], 0)[1]
    print("%s: nf %d, D gap %.2e, theta %.2e" % (name, nf, (f - g["D"]) / abs(g["D"]), et))
    assert f <= g["D"] + dc.F_BOUND * abs(g["D"]) and et <= g["par_bound"]
    bad = [x for x, v in calls if not np.isfinite(v)]
    assert bad and all(x[1] > 1 for x in bad)                  # the sequential run met rho > 1 ...
    with pytest.raises(RuntimeError, match="rc=-3"):           # ... where the oracle's mvn_ll has no value
        orc.mvn_ll(d["cov"], d["data"], d["eff_range"], bad[0], d["u"])


@pytest.mark.parametrize("key", list(dc.LOOP_CASES))
def test_second_iteration_responds_continuously(orc, key):
    """u of iteration 2 under a +-2e-6 relative change of (beta, theta) after iteration 1 -- the size of the difference the
    GPU test allows there: no accept decision changes (a flipped one moves entries of u by 0.1 and more), and u moves by
    what is stored, of the order of the change itself"""
    g = dc.golden()["loop"][key]
    resp, same = dc.loop_response(key, g["after"][0])
    print("%s: u response %.3e (stored %.3e)" % (key, resp, g["u_response"]))
    assert same and g["accepts_unchanged"]
    assert resp <= 1e-5 and abs(resp - g["u_response"]) <= 1e-2 * g["u_response"]


@pytest.mark.parametrize("h", dc.HESS_STEPS)
@pytest.mark.parametrize("bounded", [False, True])
def test_fd_hessian_is_optimhess_to_the_bit(h, bounded):
    """a non-quadratic function; bounded: the last coordinate is closer than h = 1e-2 to its lower bound, so that step is cut"""
    from glmmrmcml_amd import _lib
    from oracle import drivers
    dp = C.POINTER(C.c_double)
    n = 4
    fun = lambda x: float(np.exp(0.3 * x[0] + 0.1 * x[1]) + x[1] ** 3 * x[2] + np.log(x[3]) * x[0] + 1 / (1 + x[2] ** 2))
    cb = dc._OBJ(lambda xp, nn, u: fun(np.array([xp[i] for i in range(nn)])))
    x = np.array([0.7, -0.4, 1.3, 0.05])
    lo = np.array([-np.inf, -np.inf, -np.inf, 0.045]); up = np.full(n, np.inf)
    lo_c = np.maximum(lo, -1e300); up_c = np.full(n, 1e300)
    H = np.zeros((n, n))
    _lib.check(_lib.lib().glmmr_mcml_dbg_fd_hessian(cb, None, n, x.ctypes.data_as(dp), C.c_double(h), int(bounded),
                                                    lo_c.ctypes.data_as(dp) if bounded else None,
                                                    up_c.ctypes.data_as(dp) if bounded else None, H.ctypes.data_as(dp)))
    Ho = drivers.optimhess(fun, x, h, lo if bounded else None, up if bounded else None)
    assert np.array_equal(H, Ho)
