"""Wall-clock timing of the Laplace fit on the component operator (csrc/component.hip) against the dense operator.

Shapes: config 5, synth.longitudinal(2000, 10) (n = 20000, Q = 22000, 2000 components of 11 variables), and config 4,
synth.stepped_wedge(40, 8, 50) (n = 16000, Q = 320, 40 components of 8 variables and 400 observations).  The timed call is
Context.mcml_la(start, nr=True, maxiter=1, maxfun=20): one Newton step, la_optim_cov and la_optim_bcov with 20 objective
evaluations each.

A worker (--worker) is ONE process on one build of the library: after an untimed call of each operator it alternates
dense / component, --reps times, on the same context -- a library without the switch (the parent commit's) runs dense
only.  The driver runs a worker on the parent commit's library (--parent-lib, loaded through GLMMR_MCML_LIB: the dense
figures that are reported) and one on this tree's library, each under a time limit of its own, and prints one JSON
object (profiles/la_component_timing.json).

    python scripts/time_la_component.py --parent-lib PATH [--configs cfg5,cfg4] [--reps 3] [--limit 560] [--out FILE]

--wide times the third operator, "component_wide" (k_lac_factor_wg), by the same protocol in ONE worker on this tree's
library (profiles/la_component_wide_timing.json): config 4 with dense / component / component_wide alternating -- the
baseline is "component", the parent commit's kernel, in the same process -- and synth.cluster_rct(100, 40, 10) (n = 40000,
Q = 4100, 100 components of 41 variables and 400 observations: above the cap of "component") with dense / component_wide.

    python scripts/time_la_component.py --wide [--reps 3] [--limit 560] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(args):
    import numpy as np
    import torch
    from glmmrmcml_amd import _lib, api, synth
    assert torch.cuda.is_available(), "needs the GPU"
    has_switch = hasattr(_lib.lib(), "glmmr_mcml_ctx_set_la_operator")
    specs = {"cfg5": lambda: synth.longitudinal(2000, 10), "cfg4": lambda: synth.stepped_wedge(40, 8, 50),
             "cfg4_wide": lambda: synth.stepped_wedge(40, 8, 50), "rct41_wide": lambda: synth.cluster_rct(100, 40, 10)}
    modes_of = {"cfg4_wide": ["dense", "component", "component_wide"], "rct41_wide": ["dense", "component_wide"]}
    out = {"device": torch.cuda.get_device_name(0), "library": _lib.LIB_PATH, "has_switch": has_switch, "reps": args.reps}
    for key in args.configs.split(","):
        d = specs[key]()
        modes = modes_of.get(key, ["dense", "component"]) if has_switch else ["dense"]
        calls, fits = [], {}
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
            for rep in range(args.reps + 1):                    # rep 0: untimed, first-time work of each operator
                for mode in modes:
                    if has_switch:
                        ctx.set_la_operator(mode)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r = ctx.mcml_la(d["start"], nr=True, maxiter=1, maxfun=20)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    fits[mode] = r
                    print("%s %s call %d: %.1f ms" % (key, mode, rep, 1e3 * dt), file=sys.stderr, flush=True)
                    if rep > 0:
                        rec = dict(mode=mode, wall_ms=round(1e3 * dt, 3))
                        if has_switch:
                            p = ctx.la_plan()
                            assert p["operator"] == mode, p
                            rec.update(launches=p["launches"], dense_bytes=p["dense_bytes"], waves=p.get("waves"))
                        calls.append(rec)
            res = dict(n=int(d["n"]), Q=int(d["Q"]), calls=calls)
            if has_switch:
                p = ctx.la_plan()
                res["plan"] = dict(ncomp=p["ncomp"], max_vars=p["max_vars"], max_rows=p["max_rows"])
        for mode in modes:
            ms = sorted(c["wall_ms"] for c in calls if c["mode"] == mode)
            res[mode + "_ms"] = ms
            res[mode + "_ms_median"] = ms[len(ms) // 2]
            res[mode + "_fit"] = dict(beta=fits[mode]["beta"].tolist(), theta=fits[mode]["theta"].tolist())
        for mode in modes[1:]:                                   # faster and different is not faster
            a, b = fits["dense"], fits[mode]
            res[mode + "_vs_dense_max_abs_diff"] = dict(beta=float(np.abs(a["beta"] - b["beta"]).max()),
                                                        theta=float(np.abs(a["theta"] - b["theta"]).max()),
                                                        u=float(np.abs(a["u"] - b["u"]).max()))
        out[key] = res
    print("WORKER " + json.dumps(out))


def run_worker(args, lib):
    env = dict(os.environ)
    if lib:
        env["GLMMR_MCML_LIB"] = os.path.abspath(lib)
    else:
        env.pop("GLMMR_MCML_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--configs", args.configs, "--reps", str(args.reps)]
    p = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, text=True, timeout=args.limit)   # stderr: the progress lines
    if p.returncode != 0:
        raise SystemExit("worker failed (%d)" % p.returncode)
    return json.loads(next(l for l in p.stdout.splitlines() if l.startswith("WORKER "))[7:])


def wide(args):
    args.configs = "cfg4_wide,rct41_wide"
    br = run_worker(args, None)
    out = {"device": br["device"], "call": "Context.mcml_la(start, nr=True, maxiter=1, maxfun=20)", "reps": args.reps,
           "clock": "host wall clock around the call, device synchronised before and after",
           "order": "one process: one untimed call of each operator, then the operators alternating on one context"}
    for key in args.configs.split(","):
        r = br[key]
        modes = [m for m in ("dense", "component", "component_wide") if m + "_ms" in r]
        e = dict(n=r["n"], Q=r["Q"], plan=r["plan"])
        for m in modes:
            e[m + "_ms"] = r[m + "_ms"]
            e[m + "_ms_median"] = r[m + "_ms_median"]
            e[m + "_waves"] = sorted({c["waves"] for c in r["calls"] if c["mode"] == m})
            e[m + "_launches_per_call"] = [c["launches"] for c in r["calls"] if c["mode"] == m]
            e[m + "_dense_bytes"] = [c["dense_bytes"] for c in r["calls"] if c["mode"] == m]
        base = "component" if "component" in modes else "dense"
        e["baseline"] = base
        e[base + "_over_component_wide"] = round(r[base + "_ms_median"] / r["component_wide_ms_median"], 2)
        # faster beyond the run-to-run spread: the slowest repetition of the one under the fastest of the other
        e["component_wide_faster_beyond_spread"] = max(r["component_wide_ms"]) < min(r[base + "_ms"])
        for m in modes[1:]:
            e[m + "_vs_dense_max_abs_diff"] = r[m + "_vs_dense_max_abs_diff"]
        out[key] = e
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg5,cfg4")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libglmmr_mcml_hip.so built from the parent commit")
    ap.add_argument("--limit", type=int, default=560, help="seconds a worker may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--wide", action="store_true", help="time component_wide on this tree's library alone")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if args.wide:
        return wide(args)
    if not args.parent_lib:
        raise SystemExit("--parent-lib: the dense figures come from the parent commit's library")
    parent = run_worker(args, args.parent_lib)                    # a failure or a time limit ends the run here
    assert not parent["has_switch"], "--parent-lib has the switch: not the parent commit's library"
    branch = run_worker(args, None)
    out = {"device": branch["device"], "call": "Context.mcml_la(start, nr=True, maxiter=1, maxfun=20)", "reps": args.reps,
           "clock": "host wall clock around the call, device synchronised before and after",
           "order": "per process: one untimed call of each operator, then dense / component alternating"}
    for key in args.configs.split(","):
        pa, br = parent[key], branch[key]
        out[key] = dict(n=br["n"], Q=br["Q"], plan=br["plan"],
                        dense_parent_ms=pa["dense_ms"], dense_branch_ms=br["dense_ms"], component_ms=br["component_ms"],
                        dense_parent_ms_median=pa["dense_ms_median"], component_ms_median=br["component_ms_median"],
                        dense_over_component=round(pa["dense_ms_median"] / br["component_ms_median"], 2),
                        component_launches_per_call=[c["launches"] for c in br["calls"] if c["mode"] == "component"],
                        component_dense_bytes=[c["dense_bytes"] for c in br["calls"] if c["mode"] == "component"],
                        dense_bytes=[c["dense_bytes"] for c in br["calls"] if c["mode"] == "dense"],
                        component_vs_dense_max_abs_diff=br["component_vs_dense_max_abs_diff"])
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
