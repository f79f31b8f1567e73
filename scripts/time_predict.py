"""Time of the conditional prediction of the random effects at new points on the device (Context.predict_re,
csrc/predict.hip) and on the host (ModelMCML.predict(on="host"): numpy float64, the process's threads) at the headline
designs: synth.geospatial(5000) with m = 1024 sample columns and K = 10000 points of a regular grid, and
synth.geospatial(2000) with m = 256 and K = 4000.

One process, host and device in the same run.  Device: one resident context per design, the samples set once; 2 untimed
calls (the first carries the allocations), then --reps (7) timed calls of the query alone, summary only -- host wall clock
around the call, which ends in its own download and stream synchronisation, the device idle before it; median and spread
are reported, each window a single call: what a user waits for.  One more call returns the K x m means too, and one runs
under GLMMR_MCML_PREDICT_PHASES=1, which synchronises the stream after every phase and prints the split (build, factor,
solves, product, summary) on stderr; the split is read back from there (file descriptor 2 goes to a file for that one call).
Host: one call.  The two results are compared entry by entry.

    python scripts/time_predict.py [--reps 7] [--out profiles/predict_timing.json]
"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def grid(K):
    """the first K points of the smallest regular square grid of the unit square that holds K"""
    side = int(np.ceil(K ** 0.5))
    g = (np.arange(side) + 0.5) / side
    return np.array([(a, b) for a in g for b in g])[:K]


def phases(ctx, theta, newdata):
    """the phase line of one call under GLMMR_MCML_PREDICT_PHASES=1"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        os.environ["GLMMR_MCML_PREDICT_PHASES"] = "1"
        try:
            t0 = time.perf_counter()
            ctx.predict_re(theta, newdata)
            dt = 1e3 * (time.perf_counter() - t0)
        finally:
            del os.environ["GLMMR_MCML_PREDICT_PHASES"]
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode(errors="replace")
    found = re.search(r"predict_re phases ms: build (\S+) factor (\S+) solves (\S+) product (\S+) summary (\S+)", text)
    out = dict(zip(("build", "factor", "solves", "product", "summary"), (float(v) for v in found.groups())))
    out["call_ms_synchronised"] = round(dt, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_timing.json"))
    args = ap.parse_args()
    import torch
    from glmmrmcml_amd import api, synth
    from glmmrmcml_amd.model import ModelMCML
    assert torch.cuda.is_available(), "needs the GPU"
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "untimed_calls": 2,
           "host_threads": torch.get_num_threads(), "cases": []}
    for n, m, K in ((5000, 1024, 10000), (2000, 256, 4000)):
        d = synth.geospatial(n)
        name = "geospatial(%d)" % n
        xy = d["data"].reshape(2, n).T
        D = d["theta"][0] * np.exp(-np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1)) / d["theta"][1])
        u = np.asfortranarray(np.linalg.cholesky(D) @ np.random.default_rng(2).standard_normal((n, m)))
        newdata = [grid(K)]
        rec = dict(design=name, Q=n, m=m, K=K)
        with api.Context(d["cov"], d["data"], d["eff_range"]) as ctx:
            ctx.set_u(u)
            wall = []
            for rep in range(args.reps + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dev = ctx.predict_re(d["theta"], newdata)
                dt = 1e3 * (time.perf_counter() - t0)
                print("%s device call %d: %.3f ms" % (name, rep, dt), file=sys.stderr, flush=True)
                if rep >= 2:
                    wall.append(round(dt, 4))
            rec["plan"] = ctx.predict_plan()
            rec["device"] = dict(wall_ms=wall, median_ms=statistics.median(wall), min_ms=min(wall), max_ms=max(wall))
            t0 = time.perf_counter()
            devm = ctx.predict_re(d["theta"], newdata, means=True)
            rec["device"]["with_means_ms"] = round(1e3 * (time.perf_counter() - t0), 4)
            rec["device"]["phases_ms"] = phases(ctx, d["theta"], newdata)
        mod = ModelMCML(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["family"], d["link"], d["beta"], d["theta"])
        fit = dict(theta=np.r_[d["beta"], d["theta"], d["sigma"]], re_samps=u)
        t0 = time.perf_counter()
        host = mod.predict(fit, newdata, on="host")
        dt = time.perf_counter() - t0
        print("%s host: %.3f s" % (name, dt), file=sys.stderr, flush=True)
        rec["host"] = dict(seconds=round(dt, 4), calls=1)
        rec["host_over_device"] = round(1e3 * dt / rec["device"]["median_ms"], 1)
        rec["device_vs_host_max_abs"] = dict(mean=float(np.max(np.abs(dev["mean"] - host["re_mean"]))),
                                             cond_var=float(np.max(np.abs(dev["cond_var"] - host["cond_var"]))),
                                             sample_var=float(np.max(np.abs(dev["sample_var"] - host["sample_var"]))))
        rec["summary_bits_equal_with_and_without_means"] = bool(all(np.array_equal(dev[k], devm[k]) for k in dev))
        out["cases"].append(rec)
    txt = json.dumps(out, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
