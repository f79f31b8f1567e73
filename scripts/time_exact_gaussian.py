"""Time of one hmc_sample call under draws = "hmc" and draws = "exact" (csrc/hmc_exact.h) at the two gaussian / identity
headline shapes: synth.geospatial(2000) with 256 columns and synth.geospatial(5000) with 1024.

One context per shape, both modes in the same process: after one untimed call of each mode, --reps (5) timed calls of each,
alternating; host wall-clock around the call with the device idle before and after; the median is reported.  The HMC call
is the benchmark's: warmup 100, one draw per chain, lambda 5, at most 10 steps, target acceptance 0.9.  The exact calls also
record the HIP-event split of their phases (M build, factorisation, right-hand side and fill, transposed solve, L V), and
the forward solve trsm_left_lower is timed at the transposed solve's shape for comparison.

    python scripts/time_exact_gaussian.py [--shapes 2000:256,5000:1024] [--reps 5] [--out profiles/exact_gaussian_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2000:256,5000:1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_gaussian_timing.json"))
    args = ap.parse_args()
    import torch
    from glmmrmcml_amd import _lib, api, synth
    assert torch.cuda.is_available(), "needs the GPU"
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "hmc_call": dict(warmup=100, draws_per_chain=1, lambda_=5.0, max_steps=10, target_accept=0.9), "shapes": []}
    for spec in args.shapes.split(","):
        n, m = (int(v) for v in spec.split(":"))
        d = synth.geospatial(n, seed=1)
        wall = {"hmc": [], "exact": []}
        phases = []
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
            ctx.update_L(d["theta"])
            ctx.exact_phases(enable=True)
            for rep in range(args.reps + 1):                    # rep 0: untimed, first-time work of each mode
                for mode in ("hmc", "exact"):
                    ctx.set_draws(mode)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ctx.hmc_sample(d["beta"], d["sigma"], 100, m, 5.0, 10, 0.9, seed=7, chains=m, iter_idx=rep + 1)
                    torch.cuda.synchronize()
                    dt = 1e3 * (time.perf_counter() - t0)
                    assert (ctx.last_kernels() == ("exact", "exact")) == (mode == "exact")
                    print("n=%d m=%d %s call %d: %.2f ms" % (n, m, mode, rep, dt), file=sys.stderr, flush=True)
                    if rep > 0:
                        wall[mode].append(round(dt, 3))
                        if mode == "exact":
                            phases.append(ctx.exact_phases(enable=True))
            fwd = C.c_double()
            _lib.check(_lib.lib().glmmr_mcml_dbg_trsm_compare(ctx._h, m, args.reps, None, C.byref(fwd)))
            trans = C.c_double()
            _lib.check(_lib.lib().glmmr_mcml_dbg_trsm_compare(ctx._h, m, args.reps, C.byref(trans), None))
        med = {k: statistics.median(v) for k, v in wall.items()}
        split = {k: round(statistics.median(p[k] for p in phases), 3) for k in phases[0]}
        out["shapes"].append(dict(n=n, Q=n, columns=m, wall_ms=wall, median_ms=med,
                                  hmc_over_exact=round(med["hmc"] / med["exact"], 2), exact_phase_ms_median=split,
                                  solve_ms_at_this_shape=dict(forward_trsm_left_lower=round(fwd.value, 3),
                                                              transposed_trsm_left_lower_trans=round(trans.value, 3))))
    txt = json.dumps(out, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
