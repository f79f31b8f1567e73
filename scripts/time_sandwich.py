"""Time of the cluster-robust sandwich of the fixed effects on the host (ModelMCML.sandwich(on="host"): numpy, dense D
downloaded, two n x n solves) and on the device (Context.sandwich, csrc/sandwich.hip) at synth.stepped_wedge() and
synth.longitudinal(500, 10) (component operator, default clusters), synth.longitudinal() (device only where the host solve
is predicted to take minutes) and synth.geospatial(2000) with cluster = arange(n) % 50 (dense operator).

One process, host and device in the same run.  Device: one resident context per design, L set once; 2 untimed calls, then
--reps (7) timed calls of the query alone -- host wall clock around the call, which ends in its own downloads and stream
synchronisation, the device idle before it; the median and the spread are reported.  The call includes the bread, i.e. the
information query.  Host: one call, timed where the predicted cost -- 2 n Q^2 + 2 n^2 Q + n^3 / 3 + 2 n^2 (P + 1) flops at the
rate the previous host call reached, and 3 n max(n, Q) doubles of temporaries -- stays inside --host-budget seconds and
--host-gb; otherwise null with the reason.  Host threads are torch's (16 on the measuring machine).  Nothing here is a
promise: the numbers are what was measured.

    python scripts/time_sandwich.py [--reps 7] [--out profiles/sandwich_timing.json]
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


def host_cost(n, Q, P):
    return 2.0 * n * Q * Q + 2.0 * n * n * Q + n ** 3 / 3.0 + 2.0 * n * n * (P + 1), 3.0 * n * max(n, Q) * 8 / 2 ** 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-budget", type=float, default=30.0, help="seconds a host call may be predicted to take")
    ap.add_argument("--host-gb", type=float, default=16.0, help="GiB of temporaries a host call may need")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sandwich_timing.json"))
    args = ap.parse_args()
    import torch
    from glmmrmcml_amd import api, synth
    from glmmrmcml_amd.model import ModelMCML
    assert torch.cuda.is_available(), "needs the GPU"
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "untimed_calls": 2,
           "host_threads": torch.get_num_threads(), "cases": []}
    cases = [("stepped_wedge()", synth.stepped_wedge, None),
             ("longitudinal(500, 10)", lambda: synth.longitudinal(500, 10), None),
             ("longitudinal()", synth.longitudinal, None),
             ("geospatial(2000), cluster = arange(n) % 50", lambda: synth.geospatial(2000), 50)]
    rate = None                                                    # flops / s of the last host call
    for name, make, mod in cases:
        d = make()
        n, Q, P = d["n"], d["Q"], d["P"]
        sigma = float(d["sigma"])
        cluster = None if mod is None else (np.arange(n) % mod).astype(np.int32)
        rec = dict(design=name, n=n, Q=Q, P=P, family=d["family"], link=d["link"])
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
            ctx.update_L(d["theta"])
            wall = []
            for rep in range(args.reps + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dev = ctx.sandwich(d["beta"], sigma, cluster=cluster, scores=True)
                dt = 1e3 * (time.perf_counter() - t0)
                print("%s device call %d: %.3f ms" % (name, rep, dt), file=sys.stderr, flush=True)
                if rep >= 2:
                    wall.append(round(dt, 4))
            rec["device"] = dict(plan=ctx.sandwich_plan(), ncluster=dev["ncluster"], wall_ms=wall,
                                 median_ms=statistics.median(wall), min_ms=min(wall), max_ms=max(wall))
            wall = []
            for rep in range(args.reps + 2):                       # the bread alone, for the share of the call it takes
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ctx.information_matrix(d["beta"], sigma)
                if rep >= 2:
                    wall.append(round(1e3 * (time.perf_counter() - t0), 4))
            rec["device"]["information_alone_median_ms"] = statistics.median(wall)
        flops, gb = host_cost(n, Q, P)
        if gb > args.host_gb:
            rec["host"] = dict(seconds=None, reason="%.0f GiB of n x max(n, Q) temporaries, above --host-gb %.0f" % (gb, args.host_gb))
        elif rate is not None and flops / rate > args.host_budget:
            rec["host"] = dict(seconds=None, reason="predicted %.0f s (%.3g flops at the %.3g flop/s of the previous host call), above "
                                                    "--host-budget %.0f" % (flops / rate, flops, rate, args.host_budget))
        else:
            m = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["family"], d["link"], d["beta"], d["theta"])
            t0 = time.perf_counter()
            H = m.sandwich(d["y"], d["theta"], d["beta"], sigma, cluster=cluster, on="host")
            dt = time.perf_counter() - t0
            rate = flops / dt
            rec["host"] = dict(seconds=round(dt, 4), calls=1, flops_model=flops, flop_per_s=rate)
            rec["device_vs_host_max_rel_vcov"] = float(np.max(np.abs(dev["vcov"] - H["vcov"])) / np.max(np.abs(H["vcov"])))
            rec["host_over_device"] = round(1e3 * dt / rec["device"]["median_ms"], 1)
            print("%s host: %.3f s" % (name, dt), file=sys.stderr, flush=True)
        out["cases"].append(rec)
    txt = json.dumps(out, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
