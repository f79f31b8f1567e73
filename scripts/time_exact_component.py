"""Time of one hmc_sample call under draws = "hmc" and draws = "exact_component" (csrc/hmc_exact_comp.h) on the two
block-structured headline designs with a gaussian / identity response drawn from the design: synth.longitudinal() (config
5's design: 2000 components of 11 variables) with 1024 columns and synth.stepped_wedge() (config 4's: 40 components of 8
variables, 400 observations each) with 512.

One context per shape, both modes in the same process: after one untimed call of each mode, --reps (5) timed calls of each,
alternating; host wall-clock around the call with the device idle before and after; the median is reported.  The HMC call
is the benchmark's on the same context (the per-step path of the sparse operator): warmup 100, one draw per chain, lambda
0.5, at most 10 steps, target acceptance 0.9.  The component calls also record the HIP-event split of their phases
(right-hand side + factors + mean | draw kernel | transpose | L V).

    python scripts/time_exact_component.py [--reps 5] [--out profiles/exact_component_timing.json]
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

SIGMA = 1.0
COMP = ("exact_component", "exact_component")


def gaussian(d, u):
    """the design with y = X beta + Z u + sigma eps"""
    rng = np.random.default_rng(77)
    y = d["X"] @ d["beta"] + d["Z"] @ u + SIGMA * rng.standard_normal(d["n"])
    return dict(d, y=y, family="gaussian", link="identity", sigma=SIGMA)


def longitudinal():
    from glmmrmcml_amd import synth
    d = synth.longitudinal()
    nsubj = 2000
    rng = np.random.default_rng(5)
    th = d["theta"]
    u = np.concatenate([th[0] * rng.standard_normal(nsubj), th[1] * rng.standard_normal(d["Q"] - nsubj)])
    return gaussian(d, u)


def stepped_wedge():
    from glmmrmcml_amd import synth
    d = synth.stepped_wedge()
    ncl, nt = 40, 8
    rng = np.random.default_rng(4)
    th = d["theta"]
    dt = np.abs(np.arange(nt)[:, None] - np.arange(nt)[None, :])
    Lb = np.linalg.cholesky(th[0] ** 2 * th[1] ** dt)
    u = np.concatenate([Lb @ rng.standard_normal(nt) for _ in range(ncl)])
    return gaussian(d, u)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_component_timing.json"))
    args = ap.parse_args()
    import torch
    from glmmrmcml_amd import api
    assert torch.cuda.is_available(), "needs the GPU"
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "hmc_call": dict(warmup=100, draws_per_chain=1, lambda_=0.5, max_steps=10, target_accept=0.9), "shapes": []}
    for name, make, m in (("longitudinal", longitudinal, 1024), ("stepped_wedge", stepped_wedge, 512)):
        d = make()
        wall = {"hmc": [], "exact_component": []}
        phases = []
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
            ctx.update_L(d["theta"])
            plan = ctx.exact_component_plan()
            assert ctx.sparse_plan(m)["active"] and plan["applicable"], plan
            ctx.exact_component_phases(enable=True)
            for rep in range(args.reps + 1):                    # rep 0: untimed, first-time work of each mode
                for mode in ("hmc", "exact_component"):
                    ctx.set_draws(mode)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ctx.hmc_sample(d["beta"], d["sigma"], 100, m, 0.5, 10, 0.9, seed=7, chains=m, iter_idx=rep + 1)
                    torch.cuda.synchronize()
                    dt = 1e3 * (time.perf_counter() - t0)
                    assert (ctx.last_kernels() == COMP) == (mode == "exact_component"), ctx.last_kernels()
                    print("%s m=%d %s call %d: %.2f ms" % (name, m, mode, rep, dt), file=sys.stderr, flush=True)
                    if rep > 0:
                        wall[mode].append(round(dt, 3))
                        if mode == "exact_component":
                            phases.append(ctx.exact_component_phases(enable=True))
        med = {k: statistics.median(v) for k, v in wall.items()}
        split = {k: round(statistics.median(p[k] for p in phases), 4) for k in phases[0]}
        out["shapes"].append(dict(design=name, n=d["n"], Q=d["Q"], columns=m, plan=plan, wall_ms=wall, median_ms=med,
                                  hmc_over_exact_component=round(med["hmc"] / med["exact_component"], 2),
                                  exact_component_phase_ms_median=split))
    txt = json.dumps(out, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
