"""Time of the GLS information matrix X' (W^-1 + Z D Z')^-1 X on the host (ModelMCML.information_matrix: numpy, dense D
downloaded, n x n solve) and on the device (Context.information_matrix, csrc/info.hip) at the headline designs:
synth.geospatial(2000), geospatial(5000) (dense operator), synth.stepped_wedge() (component operator, and the dense one
beside it), synth.longitudinal() (component operator; its host side does not fit) and longitudinal(500, 10) for a
host / device pair of that design.

One process, host and device in the same run.  Device: one resident context per design, L set once; 2 untimed calls, then
--reps (7) timed calls of the query alone -- host wall clock around the call, which ends in its own download and stream
synchronisation, the device idle before it; the median and the spread are reported, and each window is a single call: what a
user waits for.  The first (untimed) call carries the allocations.  Host: one call, timed where the predicted cost --
2 n Q^2 + 2 n^2 Q + n^3 / 3 + 2 n^2 P flops at the rate the previous host call reached, and 3 n max(n, Q) doubles of temporaries --
stays inside --host-budget seconds and --host-gb; otherwise null with the reason.  The host side includes the context it makes
for gen_D, as the caller pays it.  Both results are compared (max |dev - host| / (eps max|X'VX|)) where both exist.

    python scripts/time_information.py [--reps 7] [--out profiles/information_timing.json]
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
    return 2.0 * n * Q * Q + 2.0 * n * n * Q + n ** 3 / 3.0 + 2.0 * n * n * P, 3.0 * n * max(n, Q) * 8 / 2 ** 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-budget", type=float, default=60.0, help="seconds a host call may be predicted to take")
    ap.add_argument("--host-gb", type=float, default=16.0, help="GiB of temporaries a host call may need")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "information_timing.json"))
    args = ap.parse_args()
    import torch
    from glmmrmcml_amd import api, synth
    from glmmrmcml_amd.model import ModelMCML, _dhdmu
    assert torch.cuda.is_available(), "needs the GPU"
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "untimed_calls": 2,
           "host_threads": torch.get_num_threads(), "cases": []}
    cases = [("geospatial(2000)", lambda: synth.geospatial(2000), (None,)),
             ("geospatial(5000)", lambda: synth.geospatial(5000), (None,)),
             ("longitudinal(500, 10)", lambda: synth.longitudinal(500, 10), (None,)),
             ("stepped_wedge()", synth.stepped_wedge, (None, "dense")),
             ("longitudinal()", synth.longitudinal, (None,))]
    rate = None                                                    # flops / s of the last host call
    for name, make, operators in cases:
        d = make()
        n, Q, P = d["n"], d["Q"], d["P"]
        sigma = float(d["sigma"])
        rec = dict(design=name, n=n, Q=Q, P=P, family=d["family"], link=d["link"], device={})
        dev = None
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], np.zeros(n), d["family"], d["link"]) as ctx:
            ctx.update_L(d["theta"])
            for op in operators:
                wall = []
                for rep in range(args.reps + 2):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got = ctx.information_matrix(d["beta"], sigma, operator=op)
                    dt = 1e3 * (time.perf_counter() - t0)
                    print("%s device %s call %d: %.3f ms" % (name, op or "auto", rep, dt), file=sys.stderr, flush=True)
                    if rep >= 2:
                        wall.append(round(dt, 4))
                plan = ctx.information_plan()
                rec["device"][op or "auto"] = dict(plan=plan, wall_ms=wall, median_ms=statistics.median(wall), min_ms=min(wall),
                                                   max_ms=max(wall))
                if dev is not None:
                    rec["dense_vs_auto_max_abs"] = float(np.max(np.abs(got - dev)))
                dev = got if dev is None else dev
        flops, gb = host_cost(n, Q, P)
        if gb > args.host_gb:
            rec["host"] = dict(seconds=None, reason="%.0f GiB of n x max(n, Q) temporaries, above --host-gb %.0f" % (gb, args.host_gb))
        elif rate is not None and flops / rate > args.host_budget:
            rec["host"] = dict(seconds=None, reason="predicted %.0f s (%.3g flops at the %.3g flop/s of the previous host call), above "
                                                    "--host-budget %.0f" % (flops / rate, flops, rate, args.host_budget))
        else:
            m = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["family"], d["link"], d["beta"], d["theta"])
            t0 = time.perf_counter()
            H = m.information_matrix(d["theta"], d["beta"], sigma)
            dt = time.perf_counter() - t0
            rate = flops / dt
            w = _dhdmu(d["X"] @ d["beta"], d["family"], d["link"]) * (sigma * sigma if d["family"] == "gaussian" else 1.0)
            xtvx = float(np.max(np.abs(d["X"].T @ (d["X"] / w[:, None]))))
            rec["host"] = dict(seconds=round(dt, 4), calls=1, flops_model=flops, flop_per_s=rate)
            rec["device_vs_host_ratio_to_eps_xtvx"] = float(np.max(np.abs(dev - H)) / (2.0 ** -52 * xtvx))
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
