"""The analytic score of mvn_ll against the objective and against differencing it: ms per mvn_ll, per mvn_ll_grad and per
central-difference gradient through mvn_ll_batch with 2 R candidates (how a caller gets a gradient without the score).
One process, HIP events on the context's stream, warm, medians of N >= 20 calls.
usage: python scripts/time_mvn_grad.py [N=25] [out=profiles/mvn_grad_timing.json]"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from glmmrmcml_amd import api, synth

N = int(sys.argv[1]) if len(sys.argv) > 1 else 25
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "mvn_grad_timing.json")
assert N >= 20
stream = torch.cuda.Stream()


def median_ms(call, warm=4):
    for _ in range(warm):
        call()
    ms = []
    for _ in range(N):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def case(label, cov, data, eff, theta, u):
    theta = np.asarray(theta, dtype=np.float64)
    R = theta.size
    cand = np.repeat(theta[None, :], 2 * R, axis=0)
    for k in range(R):
        cand[2 * k, k] *= 1 + 1e-5
        cand[2 * k + 1, k] *= 1 - 1e-5
    with api.Context(cov, data, eff, stream=stream.cuda_stream) as ctx:
        ctx.set_u(u)
        value, grad = ctx.mvn_ll_grad(theta)
        ll = ctx.mvn_ll_batch(cand)
        fd = (ll[0::2] - ll[1::2]) / (cand[0::2, :].diagonal() - cand[1::2, :].diagonal())
        out = dict(case=label, Q=int(u.shape[0]), m=int(u.shape[1]), R=int(R),
                   ms_mvn_ll=median_ms(lambda: ctx.mvn_ll(theta)),
                   ms_mvn_ll_grad=median_ms(lambda: ctx.mvn_ll_grad(theta)),
                   ms_central_difference_2R_batch=median_ms(lambda: ctx.mvn_ll_batch(cand)),
                   max_abs_grad=float(np.abs(grad).max()), max_abs_grad_minus_fd=float(np.abs(grad - fd).max()))
    out["grad_over_ll"] = out["ms_mvn_ll_grad"] / out["ms_mvn_ll"]
    print(json.dumps(out), flush=True)
    return out


def samples(Q, m, seed=1):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((Q, m)) * 0.4)


results = []
d = synth.geospatial(5000, seed=1)
for m in (1024, 128):
    results.append(case("geospatial(5000)", d["cov"], d["data"], d["eff_range"], d["theta"], samples(5000, m)))
d = synth.geospatial(2000, seed=1)
results.append(case("geospatial(2000)", d["cov"], d["data"], d["eff_range"], d["theta"], samples(2000, 256)))
d = synth.longitudinal()
results.append(case("config 5 (longitudinal, diagonal D)", d["cov"], d["data"], d["eff_range"], d["theta"], samples(d["Q"], 1024)))
import cov_layouts as cl
cov, data = cl.layout(cl.MIXED)
results.append(case("MIXED", cov, data, np.zeros(cov.shape[0]), cl.MIXED_THETA, samples(cl.total_dim(cl.MIXED), 1024)))
doc = dict(device=torch.cuda.get_device_name(0), calls_per_median=N,
           method="HIP events on the context's stream around each synchronous call, 4 warm calls first", cases=results)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    f.write(json.dumps(doc, indent=1) + "\n")
