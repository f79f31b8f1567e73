"""Generates tests/golden/driver_golden.json: what the oracle's drivers (oracle/drivers.py: scipy's optimisers over the C
oracle's objective pieces) make of the cases of tests/driver_cases.py -- the optima of mcml_simlik and mcml_optim, the
Hessians at two steps, the AIC values and two iterations of the loop -- together with what the CPU twins of the
product's drivers (the library's bobyqa / bobyqa_batch over the same oracle objective) measured against those optima.
The oracle's mcml_simlik takes seconds on DG / DP and about a minute on AR, so this runs once and the tests read the file.
No sample matrix is stored: driver_cases.py regenerates them from seeds.

A case and width whose twin misses the stored optimum by more than 1e-6 gets a bound of its own, three times the measured
value (par_bound); every measured value is kept beside it.

Run from the repo root:  python tests/golden/make_driver_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import driver_cases as dc                # noqa: E402
from oracle import drivers               # noqa: E402
from oracle import oracle as orc         # noqa: E402


def _bound(measured):
    worst = max(measured)
    return dc.PAR_BOUND if worst <= dc.PAR_BOUND else 3.0 * worst


def main():
    orc.build()
    out = dict(simlik={}, optim={}, hess={}, aic={}, loop={})
    for name in dc.SIMLIK:
        d = dc.case(name); mod = dc.model(name)
        w = drivers.mcml_simlik(mod, d["u"], d["start"], niter=d["niter"])
        x = np.r_[w["beta"], w["theta"]]
        F = dc.F_obj(name)
        twins = {}
        for width in dc.WIDTHS:
            xt, ft, nf, _ = dc.simlik_twin(name, width)
            eb, et = dc.par_err(xt, x, d["P"])
            twins[str(width)] = dict(beta_err=eb, theta_err=et, F_gap=(ft - F(x)) / abs(F(x)), nf=nf,
                                     par_bound=_bound([eb, et]))
        out["simlik"][name] = dict(x=x.tolist(), F=F(x), sigma=float(w["sigma"]), twin=twins)
        print(name, out["simlik"][name], flush=True)
    for name in dc.OPTIM:
        d = dc.case(name); mod = dc.model(name)
        w = drivers.mcml_optim(mod, d["u"], d["start"], mcnr=True)
        D = mod.D_obj(d["u"])
        th, ft, nf, _ = dc.optim_twin(name)
        et = dc.par_err(th, w["theta"], 0)[1]
        out["optim"][name] = dict(beta=w["beta"].tolist(), theta=w["theta"].tolist(), D=D(w["theta"]),
                                  twin=dict(theta_err=et, F_gap=(ft - D(w["theta"])) / abs(D(w["theta"])), nf=nf),
                                  par_bound=_bound([et]))
        print(name, out["optim"][name], flush=True)
    for name in dc.HESS:
        d = dc.case(name); mod = dc.model(name)
        x = np.array(out["simlik"][name]["x"]) if name in out["simlik"] else d["start"][:-1]
        start = np.r_[x, d["start"][-1]]
        out["hess"][name] = dict(x=x.tolist(), F=dc.F_obj(name)(x),
                                 H={"%g" % h: drivers.mcml_hess(mod, d["u"], start, tol=h).tolist() for h in dc.HESS_STEPS})
        print(name, "hess", np.abs(np.array(out["hess"][name]["H"]["0.0001"])).max(), flush=True)
    for name in dc.AIC:
        d = dc.case(name); mod = dc.model(name)
        x = np.array(out["hess"][name]["x"])
        bp = np.r_[x[:d["P"]], d["start"][-1]] if d["family"] == "gaussian" else x[:d["P"]]
        out["aic"][name] = dict(beta_par=bp.tolist(), cov_par=x[d["P"]:].tolist(),
                                aic=drivers.aic_mcml(mod, d["u"], bp, x[d["P"]:]))
    for key in dc.LOOP_CASES:
        its = dc.loop_oracle(key)
        resp, same = dc.loop_response(key, its[0])
        out["loop"][key] = dict(after=its, u_response=resp, accepts_unchanged=bool(same))
        print(key, out["loop"][key], flush=True)
    with open(dc.GOLDEN, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", dc.GOLDEN, os.path.getsize(dc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
