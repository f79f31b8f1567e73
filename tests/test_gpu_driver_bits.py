"""The bits of the host optimiser layer above the kernels, pinned where its code was moved and its duplicates merged:
csrc/optim.hip, McmlOptim and the theta-round evaluator of csrc/drivers.hip, the parameter map csrc/parspace.h and the
exchange of a round in csrc/comm.hip.  The driver tests judge optima within bounds; they cannot see a trajectory that
moved.  Here the SHA-256 of what a driver returns, and of the whole theta log -- every theta the MVN objective was
evaluated at and its value, in order -- is compared with tests/golden/driver_bits.json, recorded from the library of the
commit named there (tests/golden/make_driver_bits.py: never from the code under test).

  simlik_*   mcml_simlik on DG, DP and AR (driver_cases.py) at theta_batch 0 (8 candidates a round), 3 and 1 (the sequential
             optimiser on 2n + 1 points); DG once more with GLMMR_MCML_THETA_SCALE=0
  optim_*    mcml_optim (l_optim, then the theta-step) on DG at the default width and at theta_batch 1, and on SW80, whose
             theta-step is the sequential optimiser
  hess_*     mcml_hess at step 1e-4 on DG (the pre-pass groups) and MIXED (not dense only), scale switch on and off
  emu8       one rank of an emulated 8-rank job, mcml_full of test_gpu_reduce_path.py: record, then replay (which checks
             its own values against the record)
  full_DG_c8 two mcml_full iterations of LOOP_CASES["DG_c8"]
The Laplace fits and the sequential mcml_optim on a poisson model are pinned by test_gpu_dense_la_bits.py (la_dense_*,
bobyqa).  The input hashes are asserted first: a changed numpy stream fails there instead of comparing different problems."""
import hashlib
import json
import os

import numpy as np
import pytest

import driver_cases as dc
from glmmrmcml_amd import synth

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "driver_bits.json")
ENV = ("GLMMR_MCML_THETA_SCALE", "GLMMR_MCML_THETA_BATCH", "GLMMR_MCML_THETA_SHARD", "GLMMR_MCML_BOBYQA_TRACE")


def sha256(*arrays):
    """of the arrays' values as float64 in column-major order, one after the other"""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.asarray(a, dtype=np.float64).tobytes(order="F"))
    return h.hexdigest()


def _inputs(d):
    return sha256(d["Z"], d["X"], d["y"], d["cov"], d["data"], d["eff_range"], d.get("u", []), d["start"])


def _context(d):
    from glmmrmcml_amd import api
    ctx = api.Context(*dc.args(d), d["family"], d["link"])
    if "u" in d:
        ctx.set_u(d["u"], d["niter"])
    return ctx


def _fit(r):
    return sha256(r["beta"], r["theta"], [r["sigma"]])


def _logged(ctx, call):
    """call() with the theta log on -> (its result, the rows logged)"""
    ctx.theta_log(enable=True)
    r = call()
    return r, ctx.theta_log(enable=False)


def simlik(name, tb, scale=None):
    def run(mp):
        if scale is not None:
            mp.setenv("GLMMR_MCML_THETA_SCALE", scale)
        d = dc.case(name)
        with _context(d) as ctx:
            r, log = _logged(ctx, lambda: ctx.mcml_simlik(d["start"], theta_batch=tb))
        assert log.shape[0] > 1
        return dict(inputs=_inputs(d), result=_fit(r), theta_log=sha256(log))
    return run


def optim(name, tb, mcnr):
    def run(mp):
        d = dc.case(name)
        with _context(d) as ctx:
            r, log = _logged(ctx, lambda: ctx.mcml_optim(d["start"], mcnr=mcnr, theta_batch=tb))
        assert log.shape[0] > 1
        return dict(inputs=_inputs(d), result=_fit(r), theta_log=sha256(log))
    return run


def hess(name, scale):
    def run(mp):
        mp.setenv("GLMMR_MCML_THETA_SCALE", scale)
        d = dc.case(name)
        start = np.r_[dc.golden()["hess"][name]["x"], d["start"][-1]]
        with _context(d) as ctx:
            H, log = _logged(ctx, lambda: ctx.mcml_hess(start, tol=1e-4))
        assert log.shape[0] > 1
        return dict(inputs=_inputs(d), start=sha256(start), H=sha256(H), theta_log=sha256(log))
    return run


def emu8(mp):
    d = dict(synth.geospatial(n=150, seed=9))
    kw = dict(mcnr=True, maxiter=2, warmup=15, tol=1e-12, lambda_=0.3, maxsteps=6, target_accept=0.9, seed=4242,
              chains=8, m=8, maxfun=40)
    with _context(d) as ctx:
        ctx.emulate_world(8, 1)
        rec, log_rec = _logged(ctx, lambda: ctx.mcml_full(d["start"], **kw))
        ctx.emulate_world(8, 2)
        rep, log_rep = _logged(ctx, lambda: ctx.mcml_full(d["start"], **kw))      # fails inside if a value differs
        ctx.emulate_world(1, 0)
    assert log_rec.shape[0] > log_rep.shape[0] > 1              # every rank's share against rank 0's
    return dict(inputs=_inputs(d), record=_fit(rec), record_theta_log=sha256(log_rec), replay=_fit(rep),
                replay_theta_log=sha256(log_rep))


def full(key):
    def run(mp):
        name, chains, seed = dc.LOOP_CASES[key]
        d = {k: v for k, v in dc.case(name).items() if k != "u"}
        start = np.r_[d["beta"], d["theta"], 1.0]
        with _context(d) as ctx:
            r, log = _logged(ctx, lambda: ctx.mcml_full(start, mcnr=True, maxiter=2, tol=1e-12, seed=seed, chains=chains,
                                                        **dc.LOOP))
            u = ctx.get_u()
        assert r["iters"] == 2 and log.shape[0] > 1
        return dict(inputs=_inputs(d), start=sha256(start), result=_fit(r), u=sha256(u), theta_log=sha256(log))
    return run


CASES = {}
for _name in ("DG", "DP", "AR"):
    for _tb in (0, 3, 1):
        CASES["simlik_%s_tb%d" % (_name, _tb)] = simlik(_name, _tb)
CASES.update({
    "simlik_DG_tb0_scale0": simlik("DG", 0, "0"),
    "optim_DG_default": optim("DG", 0, False),
    "optim_DG_tb1": optim("DG", 1, False),
    "optim_SW80": optim("SW80", 0, True),
    "hess_DG_scale1": hess("DG", "1"),
    "hess_DG_scale0": hess("DG", "0"),
    "hess_MIXED_scale1": hess("MIXED", "1"),
    "hess_MIXED_scale0": hess("MIXED", "0"),
    "emu8_record_replay": emu8,
    "full_DG_c8": full("DG_c8"),
})


def digests(name, mp):
    """{"inputs": .., ...} of a case through the library that is loaded; mp: a pytest.MonkeyPatch"""
    for k in ENV:
        mp.delenv(k, raising=False)
    return CASES[name](mp)


@pytest.mark.parametrize("name", list(CASES))
def test_driver_bits_are_the_recorded_ones(name, monkeypatch):
    with open(FIXTURE) as f:
        want = json.load(f)["cases"][name]
    got = digests(name, monkeypatch)
    assert got["inputs"] == want["inputs"], "the seeded inputs are not the recorded ones (numpy stream changed?)"
    for key in sorted(want):
        print(name, key, got[key])
    for key in sorted(want):
        assert got[key] == want[key], "%s: %s differs from the bits recorded in %s" % (name, key, FIXTURE)
    assert set(got) == set(want)
