"""Time of the GLS information of the covariance parameters, 1/2 tr(Sigma^-1 d_r Sigma Sigma^-1 d_s Sigma), on the host
(ModelMCML.theta_information(on="host"): numpy, the n x n definition) and on the device (Context.theta_information,
csrc/theta_info.hip) at the headline designs: synth.geospatial(2000), geospatial(5000) (dense operator),
synth.stepped_wedge() (component operator, and the dense one beside it) and synth.longitudinal() (component operator; its host
side is not run: the predicted time is reported).

One process, host and device in the same run.  Device: one resident context per design; 2 untimed calls, then --reps (5) timed
calls of the query alone -- a pair of HIP events around the call and the host wall clock around the same window, which ends
in the query's own download and stream synchronisation, the device idle before it (the phases inside are not split); each window is a single
call, update_L(theta) included: what a user waits for.  The first (untimed) call carries the allocations.  The dense operator's
model cost, (7/3 + 4 R) Q^3 flop, is reported beside the time.  Host: one call, timed where the predicted cost --
(1/3 + 2 (R + 1)) n^3 flops at the rate the previous host call reached, and (3 + 2 (R + 1)) n^2 doubles -- stays inside
--host-budget seconds and --host-gb; otherwise null with the reason and the prediction.  Both results are compared
(max |dev - host| / (eps max |host|)) where both exist.

    python scripts/time_theta_information.py [--reps 5] [--out profiles/theta_information_timing.json]
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


def host_cost(n, R1):
    return (1.0 / 3.0 + 2.0 * R1) * n ** 3, (3.0 + 2.0 * R1) * n * n * 8 / 2 ** 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-budget", type=float, default=90.0, help="seconds a host call may be predicted to take")
    ap.add_argument("--host-gb", type=float, default=24.0, help="GiB of temporaries a host call may need")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "theta_information_timing.json"))
    args = ap.parse_args()
    import torch
    from glmmrmcml_amd import api, synth
    from glmmrmcml_amd.model import ModelMCML
    assert torch.cuda.is_available(), "needs the GPU"
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "untimed_calls": 2,
           "host_threads": torch.get_num_threads(), "cases": []}
    cases = [("geospatial(2000)", lambda: synth.geospatial(2000), (None,), True),
             ("geospatial(5000)", lambda: synth.geospatial(5000), (None,), True),
             ("stepped_wedge()", synth.stepped_wedge, (None, "dense"), True),
             ("longitudinal()", synth.longitudinal, (None,), False)]
    rate = None                                                    # flops / s of the last host call
    for name, make, operators, run_host in cases:
        d = make()
        n, Q, P, R = d["n"], d["Q"], d["P"], len(d["theta"])
        sigma = float(d["sigma"])
        rec = dict(design=name, n=n, Q=Q, P=P, R=R, family=d["family"], link=d["link"], device={})
        dev = None
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], np.zeros(n), d["family"], d["link"]) as ctx:
            for op in operators:
                wall, evms = [], []
                for rep in range(args.reps + 2):
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    t0 = time.perf_counter()
                    got = ctx.theta_information(d["beta"], sigma, d["theta"], operator=op)["information"]
                    dt = 1e3 * (time.perf_counter() - t0)
                    e1.record()
                    torch.cuda.synchronize()
                    print("%s device %s call %d: %.3f ms" % (name, op or "auto", rep, dt), file=sys.stderr, flush=True)
                    if rep >= 2:
                        wall.append(round(dt, 4)); evms.append(round(e0.elapsed_time(e1), 4))
                plan = ctx.theta_information_plan()
                r = dict(plan=plan, wall_ms=wall, event_ms=evms, median_ms=statistics.median(wall), min_ms=min(wall),
                         max_ms=max(wall))
                if plan["op"] == 0:
                    r["flop_model"] = (7.0 / 3.0 + 4.0 * R) * float(Q) ** 3
                    r["tflops_at_median"] = round(r["flop_model"] / (1e-3 * r["median_ms"]) / 1e12, 3)
                rec["device"][op or "auto"] = r
                if dev is not None:
                    rec["dense_vs_auto_rel"] = float(np.max(np.abs(got - dev)) / np.max(np.abs(dev)))
                dev = got if dev is None else dev
        R1 = R + (1 if (d["family"], d["link"]) == ("gaussian", "identity") else 0)
        flops, gb = host_cost(n, R1)
        pred = None if rate is None else flops / rate
        if not run_host:
            rec["host"] = dict(seconds=None, reason="not run", predicted_seconds=pred, flops_model=flops, gib=gb)
        elif gb > args.host_gb:
            rec["host"] = dict(seconds=None, reason="%.0f GiB of n x n temporaries, above --host-gb %.0f" % (gb, args.host_gb),
                               predicted_seconds=pred, flops_model=flops)
        elif pred is not None and pred > args.host_budget:
            rec["host"] = dict(seconds=None, reason="predicted %.0f s, above --host-budget %.0f" % (pred, args.host_budget),
                               predicted_seconds=pred, flops_model=flops)
        else:
            m = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["family"], d["link"], d["beta"], d["theta"])
            t0 = time.perf_counter()
            H = m.theta_information(d["theta"], d["beta"], sigma, on="host")["information"]
            dt = time.perf_counter() - t0
            rate = flops / dt
            rec["host"] = dict(seconds=round(dt, 4), calls=1, flops_model=flops, flop_per_s=rate)
            rec["device_vs_host_ratio_to_eps"] = float(np.max(np.abs(dev - H)) / (2.0 ** -52 * np.max(np.abs(H))))
            rec["host_over_device"] = round(1e3 * dt / rec["device"]["auto"]["median_ms"], 1)
            print("%s host: %.3f s" % (name, dt), file=sys.stderr, flush=True)
        out["cases"].append(rec)
    txt = json.dumps(out, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
