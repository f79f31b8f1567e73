"""Runs the CPU oracle (oracle/nuts.py) over a whole population of chains, 16 worker processes, and evaluates
tests/nuts_cases.packed_widths() on the oracle's own leapfrog counts: which column counts the device run of that
population would be packed to, and whether a checkpoint inside a doubling would re-pack it.

    python scripts/nuts_repack_search.py --case rct_200            # one case of the table
    python scripts/nuts_repack_search.py --search dense            # candidates for the `repack` case: every hit is printed
    python scripts/nuts_repack_search.py --search sparse
    python scripts/nuts_repack_search.py --case repack --golden    # write tests/golden/nuts_repack_nleap.json

No GPU is needed."""
import argparse
import itertools
import json
import multiprocessing as mp
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

_W = {}


def _init(case):
    import nuts_cases as nc
    from oracle import oracle as orc
    nc.CASES["_pop"] = case
    d = nc.design("_pop")
    _W.update(nc=nc, d=d, inp=nc.oracle_inputs(orc, d))


def _chain(c):
    _, tr = _W["nc"].oracle_chain("_pop", _W["d"], _W["inp"], c)
    return tr["depth"].tolist(), tr["nleap"].tolist()


def population(case):
    """(depth, nleap), each C x transitions, of the oracle's chains 0 .. C-1"""
    with mp.get_context("spawn").Pool(16, initializer=_init, initargs=(case,)) as pool:
        out = pool.map(_chain, range(case["C"]), chunksize=1)
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def report(case):
    import nuts_cases as nc
    t0 = time.time()
    depth, nleap = population(case)
    widths, repacks = nc.packed_widths(nleap, case["C"], case["cm"])
    print("  %.1f s; depth max %d, depths in the widest transition %s" % (
        time.time() - t0, depth.max(), sorted(set(depth[:, np.argmax([len(set(depth[:, t])) for t in range(depth.shape[1])])]))))
    print("  widths %s" % sorted(widths, reverse=True))
    print("  re-packs (transition, doubling, leaves, chains before, chains after): %s" % repacks)
    print("  batched leapfrogs %d" % nc.expected_batched_leapfrogs(nleap))
    return nleap, repacks


def main():
    import nuts_cases as nc
    from oracle import oracle as orc
    orc.build()
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--search", choices=("dense", "sparse"))
    ap.add_argument("--golden", action="store_true")
    ap.add_argument("--max-populations", type=int, default=50)
    a = ap.parse_args()
    if a.case:
        case = dict(nc.CASES[a.case])
        print(a.case)
        nleap, _ = report(case)
        if a.golden:
            g = {}
            if os.path.exists(nc.GOLDEN_REPACK):
                with open(nc.GOLDEN_REPACK) as f:
                    g = json.load(f)
            g[a.case] = dict(C=case["C"], transitions=int(nleap.shape[1]), nleap=nleap.tolist())
            with open(nc.GOLDEN_REPACK, "w") as f:
                json.dump(g, f, separators=(",", ":"), sort_keys=True)
                f.write("\n")
            print("wrote", nc.GOLDEN_REPACK)
    if a.search:
        # dense poisson-log / gamma-log designs with large spatial variance first, then the sparse designs
        # (chains 0 .. C-1 of a population are the population of C chains: one run of 300 serves every C up to 300)
        dense = [dict(gen="dense", kw=dict(family=f, link="log", Q=300, theta=th, seed=s), vp=vp, cm=False)
                 for s, th, (f, vp) in itertools.product((5, 6, 7), ((2.0, 0.3), (1.0, 0.2)), (("poisson", 1.0), ("gamma", 2.0)))]
        gauss = [dict(gen="geospatial", kw=dict(n=300, seed=s, theta=th), vp=1.0, cm=False)
                 for s, th in itertools.product((20240601, 1, 2), ((0.25, 0.1), (2.0, 0.3)))]
        sparse = [dict(gen=g, kw=dict(kw, seed=s), vp=1.0, cm=True)
                  for s, (g, kw) in itertools.product((20240602, 1, 2, 3), (("cluster_rct", dict(ncl=6, nt=4, nind=5, family="poisson")),
                                                                            ("stepped_wedge", dict(ncl=6, nt=4, nind=30))))]
        n, found = 0, []
        todo = list(itertools.product(dense + gauss, (0.95, 0.8))) if a.search == "dense" else list(itertools.product(sparse, (0.95, 0.99)))
        for base, delta in todo:
            if n >= a.max_populations:
                break
            n += 1
            case = dict(base, C=300, warm=14, draws=2, metric="diag_e", adapt_delta=delta)
            print("population %d: %s %s adapt_delta=%g" % (n, case["gen"], case["kw"], delta), flush=True)
            nleap, _ = report(case)
            for C in (128, 160, 200, 256, 300):
                rp = nc.packed_widths(nleap[:C], C, case["cm"])[1]
                if rp:
                    print("  FOUND with C=%d: %s" % (C, rp), flush=True)
                    found.append((case["gen"], case["kw"], delta, C, rp))
        print("%d populations, re-packs inside a doubling in: %s" % (n, found))


if __name__ == "__main__":
    main()
