"""A/B timing of the component-local trajectory path (csrc/hmc_traj.h) against the per-step path, in one process.

Configs 4 and 5 at bench.py's settings (other_configs: HMC warm-up 100 + 1 draw per chain, <= 10 leapfrog steps,
optimiser budget 40, seed 7): one untimed mcml_full iteration, then three timed iterations per path in the order step,
component, step, component -- both paths on the same context, so the same device, clocks and allocations.  Reported per
block: api.phase_ms()["sample"] and wall time per iteration.  Prints one JSON object (profiles/component_traj_ab.json).

    python scripts/time_component_traj.py [--configs cfg4,cfg5] [--iters 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg4,cfg5")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from glmmrmcml_amd import api, synth
    assert torch.cuda.is_available(), "needs the GPU"
    specs = {"cfg4": (lambda: synth.stepped_wedge(40, 8, 50), 512, 0.5), "cfg5": (lambda: synth.longitudinal(2000, 10), 1024, 0.5)}
    out = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "order": ["step", "component", "step", "component"]}
    for key in args.configs.split(","):
        gen, m, lam = specs[key]
        d = gen()
        kw = dict(mcnr=True, m=m, warmup=100, tol=0.0, verbose=False, lambda_=lam, maxsteps=10, target_accept=0.9, seed=7,
                  chains=m, maxfun=40)
        blocks = []
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
            for mode in ("step", "component"):                  # untimed: first-time work of both paths
                ctx.set_trajectory(mode)
                ctx.mcml_full(d["start"], maxiter=1, **kw)
            plan = ctx.component_plan(m)
            for mode in out["order"]:
                ctx.set_trajectory(mode)
                api.phase_ms(enable=True, reset=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = ctx.mcml_full(d["start"], maxiter=args.iters, **kw)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                ph = api.phase_ms(enable=False)
                blocks.append(dict(mode=mode, kernels=ctx.last_kernels()[0], sample_ms_per_iter=round(ph["sample"] / args.iters, 3),
                                   wall_ms_per_iter=round(1e3 * dt / args.iters, 3), accept_rate=round(r["accept_rate"], 4),
                                   leapfrog_total=int(r["leapfrog_total"])))
        best = {mo: min(b["sample_ms_per_iter"] for b in blocks if b["mode"] == mo) for mo in ("step", "component")}
        mean = {mo: sum(b["sample_ms_per_iter"] for b in blocks if b["mode"] == mo) / 2 for mo in ("step", "component")}
        out[key] = dict(plan=plan, blocks=blocks, sample_ms_best=best, sample_ms_mean={k: round(v, 3) for k, v in mean.items()},
                        component_over_step=round(mean["component"] / mean["step"], 4))
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
