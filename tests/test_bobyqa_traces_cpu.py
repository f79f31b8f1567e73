"""The trajectories of the host optimiser (csrc/optim.hip), pinned where its duplicated rules were merged: the start rule,
the rho schedule, the delta update, the coordinate steps of the initial design, the one-parameter embedding.
test_optim_cpu.py judges optima within tolerances and cannot see a trajectory that moved; here every evaluated point in
order (raw float64), the result, fval and nfev are hashed, and compared with tests/golden/bobyqa_traces.json -- recorded
from the library of the commit named there (tests/golden/make_bobyqa_traces.py: never from the code under test).

The objectives are plain Python floats under +, - and * only: no BLAS, no libm (optim.hip itself uses only sqrt), so the
values are the same IEEE doubles wherever the test runs.  No GPU is needed: the hooks are host code of the library.

  quad{2,3,6}   convex quadratics: sequential, and the batch entry at widths 1 (= the sequential run: asserted), 2 and 8
  rosen         bounded Rosenbrock to rhoend 1e-8: sequential, width 8, width 8 through the round callback, npt = 2n + 1
  novalue       no value where x0 > 0.9, start inside that half plane: sequential and width 4
  one           one parameter above a lower bound of 1e-6 (both embeddings: the sequential entry, widths 1 and 4)
  snap          start within 1e-9 relative of a lower bound (snapped onto it); with rhobeg / rhoend given (no snap)
  tight         finite bounds closer together than the default radius
  npt           2n + 1 interpolation points through glmmr_mcml_dbg_bobyqa_npt
  maxfun        a budget that ends inside the initial design (width 4) and budgets that end mid-run"""
import ctypes as C
import hashlib
import json
import os
import struct

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bobyqa_traces.json")
_dp = C.POINTER(C.c_double)
_OBJ = C.CFUNCTYPE(C.c_double, _dp, C.c_int, C.c_void_p)
_ROUND = C.CFUNCTYPE(C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_void_p)
INF = float("inf")


# ------------------------------------------------------------------------------------------------ objectives
def quad(n):
    """sum_i (i + 1) (x_i - c_i)^2 + 1/2 sum_{i<j} (x_i - c_i)(x_j - c_j) + 3, c_i = 0.25 i - 0.5"""
    def f(x):
        d = [x[i] - (0.25 * i - 0.5) for i in range(n)]
        s = 3.0
        for i in range(n):
            s = s + (i + 1.0) * d[i] * d[i]
            for j in range(i + 1, n):
                s = s + 0.5 * d[i] * d[j]
        return s
    return f


def rosen(x):
    a = x[1] - x[0] * x[0]
    b = 1.0 - x[0]
    return 100.0 * a * a + b * b


def novalue(x):
    if x[0] > 0.9:
        return INF
    a = x[0] - 0.3
    b = x[1] + 0.2
    return a * a + 2.0 * b * b + 0.5 * a * b


def one(x):
    a = x[0] - 0.3
    return a * a + 1.0


def corner(x):
    """minimum at (0.4, 0.7) unconstrained; pulled to the lower bounds when those are above it"""
    a = x[0] - 0.4
    b = x[1] - 0.7
    return 3.0 * a * a + b * b + a * b


# ------------------------------------------------------------------------------------------------ cases
def case(fun, x0, lower=None, upper=None, hook="bobyqa", width=0, rhobeg=0.0, rhoend=0.0, maxfun=0, npt=0):
    return dict(fun=fun, x0=x0, lower=lower, upper=upper, hook=hook, width=width, rhobeg=rhobeg, rhoend=rhoend,
                maxfun=maxfun, npt=npt)


CASES = {}
for _n in (2, 3, 6):
    _x0 = [1.0 + 0.5 * i for i in range(_n)]
    CASES["quad%d_seq" % _n] = case(quad(_n), _x0)
    for _w in (1, 2, 8):
        CASES["quad%d_w%d" % (_n, _w)] = case(quad(_n), _x0, hook="batch", width=_w)
_B = dict(lower=[-2.0, -2.0], upper=[0.5, 2.0])
_NEAR = [1e-6 * (1.0 + 1e-9), 0.5]
CASES.update({
    "quad3_rounds_w8": case(quad(3), [1.0, 1.5, 2.0], hook="rounds", width=8),
    "rosen_seq": case(rosen, [-1.2, 1.0], rhoend=1e-8, **_B),
    "rosen_w8": case(rosen, [-1.2, 1.0], hook="batch", width=8, rhoend=1e-8, **_B),
    "rosen_rounds_w8": case(rosen, [-1.2, 1.0], hook="rounds", width=8, rhoend=1e-8, **_B),
    "rosen_npt5": case(rosen, [-1.2, 1.0], hook="npt", npt=5, rhoend=1e-8, **_B),
    "novalue_seq": case(novalue, [1.0, 1.0]),
    "novalue_w4": case(novalue, [1.0, 1.0], hook="batch", width=4),
    "one_seq": case(one, [1.0], lower=[1e-6], upper=[INF]),
    "one_w1": case(one, [1.0], lower=[1e-6], upper=[INF], hook="batch", width=1),
    "one_w4": case(one, [1.0], lower=[1e-6], upper=[INF], hook="batch", width=4),
    "snap_seq": case(corner, _NEAR, lower=[1e-6, 1e-6], upper=[INF, INF]),
    "snap_w4": case(corner, _NEAR, lower=[1e-6, 1e-6], upper=[INF, INF], hook="batch", width=4),
    "nosnap_seq": case(corner, _NEAR, lower=[1e-6, 1e-6], upper=[INF, INF], rhobeg=0.25, rhoend=1e-7),
    "nosnap_w4": case(corner, _NEAR, lower=[1e-6, 1e-6], upper=[INF, INF], hook="batch", width=4, rhobeg=0.25, rhoend=1e-7),
    "tight_seq": case(corner, [3.0, 2.0], lower=[2.9, 1.95], upper=[3.1, 2.2]),
    "tight_w4": case(corner, [3.0, 2.0], lower=[2.9, 1.95], upper=[3.1, 2.2], hook="batch", width=4),
    "npt7_quad3": case(quad(3), [1.0, 1.5, 2.0], hook="npt", npt=7),
    "npt13_quad6_bounded": case(quad(6), [1.0 + 0.5 * i for i in range(6)], lower=[0.0] * 6, upper=[4.0] * 6, hook="npt", npt=13),
    "maxfun5_inside_design_w4": case(quad(6), [1.0 + 0.5 * i for i in range(6)], hook="batch", width=4, maxfun=5),
    "maxfun20_seq": case(quad(6), [1.0 + 0.5 * i for i in range(6)], maxfun=20),
    "maxfun30_w8": case(quad(6), [1.0 + 0.5 * i for i in range(6)], hook="batch", width=8, maxfun=30),
    "maxfun12_one_w4": case(one, [1.0], lower=[1e-6], upper=[INF], hook="batch", width=4, maxfun=12),
})


def _arr(v):
    return (C.c_double * len(v))(*v)


def trace(name):
    """{"trace": SHA-256 of every evaluated point in order, the result, fval and nfev, "points", "nfev", "rounds"} of a case
    through the library that is loaded"""
    from glmmrmcml_amd import _lib
    L = _lib.lib()
    c = CASES[name]
    n = len(c["x0"])
    h = hashlib.sha256()
    npoints = [0]

    def value(xp):
        x = [xp[i] for i in range(n)]
        h.update(struct.pack("<%dd" % n, *x))
        npoints[0] += 1
        return float(c["fun"](x))

    def cb(xp, nn, user):
        return value(xp)

    def cbr(Xp, nn, k, Fp, user):
        for j in range(k):
            Fp[j] = value([Xp[j * nn + i] for i in range(nn)])
        return 0
    x0 = _arr(c["x0"]); out = (C.c_double * n)(); f = C.c_double(); nf = C.c_int(); rd = C.c_int()
    lo = None if c["lower"] is None else _arr(c["lower"])
    up = None if c["upper"] is None else _arr(c["upper"])
    keep = _ROUND(cbr) if c["hook"] == "rounds" else _OBJ(cb)
    head = (keep, None, n, x0, lo, up, C.c_double(c["rhobeg"]), C.c_double(c["rhoend"]), c["maxfun"])
    if c["hook"] == "bobyqa":
        rc = L.glmmr_mcml_dbg_bobyqa(*head, out, C.byref(f), C.byref(nf))
    elif c["hook"] == "npt":
        rc = L.glmmr_mcml_dbg_bobyqa_npt(*head, c["npt"], out, C.byref(f), C.byref(nf))
    elif c["hook"] == "batch":
        rc = L.glmmr_mcml_dbg_bobyqa_batch(*head, c["width"], out, C.byref(f), C.byref(nf), C.byref(rd))
    else:
        rc = L.glmmr_mcml_dbg_bobyqa_rounds(*head, c["width"], out, C.byref(f), C.byref(nf), C.byref(rd))
    _lib.check(rc)
    h.update(struct.pack("<%dd" % n, *out))
    h.update(struct.pack("<d", f.value))
    h.update(struct.pack("<i", nf.value))
    return dict(trace=h.hexdigest(), points=npoints[0], nfev=nf.value, rounds=rd.value)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("name", list(CASES))
def test_trajectory_is_the_recorded_one(name, recorded):
    got = trace(name)
    print(name, got)
    assert got == recorded[name]


def test_fixture_holds_these_cases_and_width_one_is_the_sequential_run(recorded):
    assert set(recorded) == set(CASES)
    for n in (2, 3, 6):
        seq, w1 = recorded["quad%d_seq" % n], recorded["quad%d_w1" % n]
        assert w1["trace"] == seq["trace"] and w1["rounds"] == w1["nfev"] == seq["nfev"]
    # the round callback sees the points the per-point callback sees
    assert recorded["rosen_rounds_w8"] == recorded["rosen_w8"]
