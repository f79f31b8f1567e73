"""Time of the small-sample query (Context.small_sample, csrc/small_sample.hip: I_beta, I_theta and the P_r, Q_rs, R_rs of the
Kenward-Roger / Satterthwaite corrections) against ModelMCML.small_sample(on="host") (numpy, the n x n definition) at the
headline designs: synth.geospatial(2000), geospatial(5000) (dense operator), synth.stepped_wedge() and synth.longitudinal()
(component operator).

One process, everything on one resident context per design.  Device: 2 untimed calls, then --reps (5) timed calls each of
small_sample, theta_information and information_matrix -- the host wall clock around a single call, which ends in the query's
own download and stream synchronisation, update_L(theta) included.  The figure to read is `extra_ms`: the median of the query
minus the medians of the two queries whose results it contains.  Host: one call, timed where the predicted cost --
(1/3 + 2 R1) n^3 flops of the I_theta part, 2/3 (R1 + 1) n^3 of the solves and 4 R n Q max(n, Q) of the Z (d D) Z' products at
the rate the previous host call reached, (4 + 3 R1) n^2 doubles -- stays inside --host-budget seconds (60) and --host-gb;
otherwise null with the reason and the prediction.  Where both exist, the adjusted covariances are compared.

    python scripts/time_small_sample.py [--reps 5] [--out profiles/small_sample_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_cost(n, Q, R, R1):
    flops = (1.0 / 3.0 + 2.0 * R1) * n ** 3 + 2.0 / 3.0 * (R1 + 1) * n ** 3 + 4.0 * R * n * Q * max(n, Q)
    return flops, (4.0 + 3.0 * R1) * n * n * 8 / 2 ** 30


def timed(fn, reps, label):
    wall = []
    for rep in range(reps + 2):
        t0 = time.perf_counter()
        got = fn()
        dt = 1e3 * (time.perf_counter() - t0)
        print("%s call %d: %.3f ms" % (label, rep, dt), file=sys.stderr, flush=True)
        if rep >= 2:
            wall.append(round(dt, 4))
    return got, dict(wall_ms=wall, median_ms=statistics.median(wall), min_ms=min(wall), max_ms=max(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-budget", type=float, default=60.0, help="seconds a host call may be predicted to take")
    ap.add_argument("--host-gb", type=float, default=24.0, help="GiB of temporaries a host call may need")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "small_sample_timing.json"))
    args = ap.parse_args()
    import torch
    from glmmrmcml_amd import api, synth
    from glmmrmcml_amd.model import ModelMCML, _kenward_roger
    assert torch.cuda.is_available(), "needs the GPU"
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "untimed_calls": 2,
           "host_threads": torch.get_num_threads(), "cases": []}
    cases = [("geospatial(2000)", lambda: synth.geospatial(2000)), ("geospatial(5000)", lambda: synth.geospatial(5000)),
             ("stepped_wedge()", synth.stepped_wedge), ("longitudinal()", synth.longitudinal)]
    rate = None                                                    # flops / s of the last host call
    for name, make in cases:
        d = make()
        n, Q, P, R = d["n"], d["Q"], d["P"], len(d["theta"])
        sigma = float(d["sigma"])
        rec = dict(design=name, n=n, Q=Q, P=P, R=R, family=d["family"], link=d["link"])
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], np.zeros(n), d["family"], d["link"]) as ctx:
            dev, rec["small_sample"] = timed(lambda: ctx.small_sample(d["beta"], sigma, d["theta"]), args.reps, name + " small_sample")
            rec["plan"] = ctx.small_sample_plan()
            _, rec["theta_information"] = timed(lambda: ctx.theta_information(d["beta"], sigma, d["theta"]), args.reps,
                                                name + " theta_information")
            op = "component" if rec["plan"]["op"] == 1 else "dense"
            _, rec["information_matrix"] = timed(lambda: ctx.information_matrix(d["beta"], sigma, d["theta"], operator=op),
                                                 args.reps, name + " information_matrix")
        rec["extra_ms"] = round(rec["small_sample"]["median_ms"] - rec["theta_information"]["median_ms"]
                                - rec["information_matrix"]["median_ms"], 4)
        R1 = R + (1 if (d["family"], d["link"]) == ("gaussian", "identity") else 0)
        flops, gb = host_cost(n, Q, R, R1)
        pred = None if rate is None else flops / rate
        if gb > args.host_gb:
            rec["host"] = dict(seconds=None, reason="%.0f GiB of n x n temporaries, above --host-gb %.0f" % (gb, args.host_gb),
                               predicted_seconds=pred, flops_model=flops)
        elif pred is not None and pred > args.host_budget:
            rec["host"] = dict(seconds=None, reason="predicted %.0f s, above --host-budget %.0f" % (pred, args.host_budget),
                               predicted_seconds=pred, flops_model=flops)
        else:
            m = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["family"], d["link"], d["beta"], d["theta"])
            t0 = time.perf_counter()
            H = m.small_sample(d["theta"], d["beta"], sigma, on="host", type="KR")
            dt = time.perf_counter() - t0
            rate = flops / dt
            rec["host"] = dict(seconds=round(dt, 4), calls=1, flops_model=flops, flop_per_s=rate)
            got = _kenward_roger(dev["information"], dev["theta_information"], dev["P"], dev["Q"], dev["R"], "KR")
            rec["vcov_device_vs_host_rel"] = float(np.max(np.abs(got["vcov"] - H["vcov"])) / np.max(np.abs(H["vcov"])))
            rec["dof_device"], rec["dof_host"] = [float(v) for v in got["dof"]], [float(v) for v in H["dof"]]
            rec["host_over_device"] = round(1e3 * dt / rec["small_sample"]["median_ms"], 1)
            print("%s host: %.3f s" % (name, dt), file=sys.stderr, flush=True)
        out["cases"].append(rec)
    txt = json.dumps(out, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
