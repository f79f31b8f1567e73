"""Cases, chain selection and trace arithmetic for the NUTS packing tests (no test in here).

tests/test_nuts_cases_cpu.py calibrates the cases on the CPU oracle alone (oracle/nuts.py); tests/test_gpu_nuts_packing.py
runs them on the device.  The cases are the smallest shapes at which csrc/nuts.h leaves the regime that
tests/test_gpu_nuts.py pins (4 chains, Q <= 96): more chains than one 64-wide wave, one 128-wide MFMA column tile or one
256-thread workgroup, more rows than one 256-row partial-sum chunk, and doublings deep enough (32 leaves and more) for the
checkpoints inside a doubling.

Only families whose log density is finite at every uniform(-2, 2) start are used (poisson-log, binomial-logit,
gaussian-identity, gamma-log, beta-logit, binomial-probit): the sampler does not reproduce Stan's retry on a non-finite
start.

A chain's draws depend on (seed, global chain id) only, so the oracle checks any single chain of a large run on its own.

The `repack` cases were found by scripts/nuts_repack_search.py, which runs the oracle over whole populations and
evaluates packed_widths() on the oracle's own leapfrog counts; tests/golden/nuts_repack_nleap.json holds the oracle's
population leapfrog counts of the chosen cases.  A re-pack inside a doubling needs chains that stop within a doubling
of 32 leaves or more while others go on.  On the dense designs that did not happen: over thirty populations of 128 to 300
chains (poisson-log and gamma-log at Q = 300 with theta (1.0, 0.2) and (2.0, 0.3), design seeds 5, 6, 7, adapt_delta 0.8,
0.9, 0.95) held no re-pack, nor do the dense cases of the table; where the stops were listed, no chain at all stopped
inside a doubling of 32 leaves -- a chain that starts a deep doubling there completes it.  Two of 16 populations of the sparse designs (Q = 30 and 24, adapt_delta 0.95 and 0.99) did, and they are the cases.  NOT
COVERED: a re-pack inside a doubling on the dense operator, where it changes the column count of the products (on
the sparse one both cases re-pack within one wave of 64 columns: the slots move, the width does not).

A re-pack is a choice of the batch's layout and leaves no mark on any chain's results, so the run reports how often
it packed (diag `packs`) and the test compares that with the count these functions derive from the traces."""
import json
import os

import numpy as np

from glmmrmcml_amd import synth

SEED, ITER_IDX, MAX_DEPTH = 20240607, 3, 8
SK_NUSE = 16                                   # csrc/dgemm_skinny.h: columns up to which the streamed products are used
EDGES = (0, 15, 16, 63, 64, 127, 128, 255, 256)
GOLDEN_REPACK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nuts_repack_nleap.json")

# gen / kw: the design (dense: tests/test_gpu_dense_products.design); vp: the family's variance parameter; cm: chain-major
# state (sparse ZL operator); widths: packed widths the device run must visit; streamed: it must also come down to
# SK_NUSE columns or fewer (dense only); min_depth: what the oracle's calibration run must reach
CASES = {
    # C > 256, 2 partial-sum chunks, Cw 300 -> 256 -> 128 -> streamed
    "dense_300x300": dict(gen="geospatial", kw=dict(n=300), vp=1.0, C=300, warm=14, draws=2, metric="diag_e", cm=False,
                          adapt_delta=0.8, widths=(300, 256, 128), streamed=True, min_depth=6, groups=True),
    # ragged second chunk (1 row), partly filled second tile, metric window and step-size re-search while packed
    "dense_pois_257x200": dict(gen="dense", kw=dict(family="poisson", link="log", Q=257, theta=(1.0, 0.2)), vp=1.0, C=200,
                               warm=24, draws=2, metric="diag_e", cm=False, adapt_delta=0.8, widths=(200, 128),
                               streamed=True, min_depth=6, groups=False),
    # 16 < C < 128: MFMA -> streamed inside a transition
    "dense_96x40": dict(gen="geospatial", kw=dict(n=96), vp=0.9, C=40, warm=14, draws=2, metric="unit_e", cm=False,
                        adapt_delta=0.8, widths=(40,), streamed=True, min_depth=3, groups=False),
    # chain-major product form, Cw 200 -> 192 / 128 / 64, Q = 30 (ragged second slow tile)
    "rct_200": dict(gen="cluster_rct", kw=dict(ncl=6, nt=4, nind=5, family="poisson"), vp=1.0, C=200, warm=14, draws=2,
                    metric="diag_e", cm=True, adapt_delta=0.8, widths=(200, 192, 128, 64), streamed=False, min_depth=6,
                    groups=True),
    # chain-major factored form, long-row backward kernel, C > 256 (two fast blocks); seed 20240608: with 20240607 the
    # population reaches depth 6, the calibration chains (edges and 1..8) only 5
    "sw_300": dict(gen="stepped_wedge", kw=dict(ncl=6, nt=4, nind=30), vp=1.0, C=300, warm=24, draws=2, metric="diag_e",
                   cm=True, adapt_delta=0.8, seed=20240608, widths=(300, 256), streamed=False, min_depth=6, groups=False),
    # a checkpoint inside a doubling re-packs (scripts/nuts_repack_search.py): 4 -> 3 chains after 64 leaves of doubling 7
    "repack": dict(gen="cluster_rct", kw=dict(ncl=6, nt=4, nind=5, family="poisson"), vp=1.0, C=128, warm=14, draws=2,
                   metric="diag_e", cm=True, adapt_delta=0.99, widths=(128, 64), streamed=False, min_depth=6, groups=False,
                   repack=1),
    # two of them, 2 -> 1 chains after 16 and after 32 leaves of doubling 6, C > 256
    "repack_300": dict(gen="cluster_rct", kw=dict(ncl=6, nt=4, nind=5, family="poisson", seed=3), vp=1.0, C=300, warm=14,
                       draws=2, metric="diag_e", cm=True, adapt_delta=0.95, widths=(300, 256, 64), streamed=False,
                       min_depth=6, groups=False, repack=2),
}

# twin deviations D (tests/test_nuts_cases_cpu.py): the oracle against itself with ZL multiplied entrywise by
# 1 + 1e-14 N(0, 1), worst over the edge chains and chains 1..8.  eps relative, accept absolute, draws relative to
# max(1, |draw|max).  The 24-transition cases pass a metric window and a second step-size search, which amplify a last-digit
# difference by orders of magnitude more than 14 transitions do (dense_pois_257x200 most of all)
TWIN_D = {
    "dense_300x300": dict(eps=3.72e-10, accept=1.29e-10, draws=2.75e-10),
    "dense_pois_257x200": dict(eps=3.12e-06, accept=3.46e-05, draws=2.25e-05),
    "dense_96x40": dict(eps=2.26e-12, accept=1.15e-12, draws=2.58e-12),
    "rct_200": dict(eps=4.09e-11, accept=6.75e-11, draws=4.98e-11),
    "sw_300": dict(eps=4.60e-09, accept=3.80e-08, draws=3.14e-08),
    "repack": dict(eps=1.33e-12, accept=2.85e-13, draws=1.09e-12),
    "repack_300": dict(eps=3.11e-12, accept=1.06e-12, draws=2.45e-12),
}


def design(name):
    c = CASES[name]
    if c["gen"] == "dense":
        import test_gpu_dense_products as dp
        kw = dict(c["kw"])
        return dp.design(kw.pop("family"), kw.pop("link"), kw.pop("Q"), **kw)
    return getattr(synth, c["gen"])(**c["kw"])


def oracle_inputs(orc, d):
    """(ZL, X beta, family / link code, L) as the oracle takes them"""
    Lo = orc.gen_D(d["cov"], d["data"], d["eff_range"], d["theta"], chol=True)
    return np.asfortranarray(d["Z"] @ Lo), d["X"] @ d["beta"], orc.flink(d["family"], d["link"]), Lo


def twin(ZL):
    """the same operator with every entry perturbed in its last digits (fixed generator)"""
    return np.asfortranarray(ZL * (1.0 + 1e-14 * np.random.default_rng(SEED).standard_normal(ZL.shape)))


def oracle_chain(name, d, inp, chain, ZL=None):
    """one chain of the case on the oracle: (draws of u = L gamma, Q x draws; trace dict)"""
    from oracle import nuts
    c = CASES[name]
    ZL0, xb, fl, Lo = inp
    so, tr, _ = nuts.nuts_chain(xb, ZL0 if ZL is None else ZL, d["y"], c["vp"], fl, c["warm"], c["draws"], c.get("seed", SEED),
                                chain_id=chain, iter_idx=ITER_IDX, max_treedepth=MAX_DEPTH, adapt_delta=c["adapt_delta"],
                                metric=c["metric"])
    return Lo @ so, tr


def deviations(eps, acc, u, eps_ref, acc_ref, u_ref):
    """(eps relative, accept absolute, draws relative to max(1, |draw|max)) of one chain"""
    return (float(np.abs(np.asarray(eps) / np.asarray(eps_ref) - 1).max()), float(np.abs(np.asarray(acc) - np.asarray(acc_ref)).max()),
            float(np.abs(u - u_ref).max() / max(1.0, np.abs(u_ref).max())))


def tolerances(name):
    """max(t0, 30 D): t0 is the tolerance of tests/test_gpu_nuts.py (1e-8 / 1e-8 / 1e-6 before 20 warm-up transitions,
    1e-5 / 1e-5 / 1e-3 at 24), D the recorded twin deviation.  The device differs from the oracle in every product and
    reduction of a leapfrog step, not in one operand: a Q = 300 dot product's own rounding bound is about 3e-14, three
    times the twin's perturbation; the remaining order of magnitude is margin."""
    t0 = (1e-8, 1e-8, 1e-6) if CASES[name]["warm"] < 20 else (1e-5, 1e-5, 1e-3)
    D = TWIN_D[name]
    return tuple(max(t, 30 * D[k]) for t, k in zip(t0, ("eps", "accept", "draws")))


def edge_chains(C):
    return sorted({e for e in EDGES + (C - 1,) if e < C})


def compared_chains(C, depth, nleap):
    """the chains the oracle is run on: the edges of waves, column tiles and workgroups, and the four chains with the
    largest total leapfrog count in the device trace (ties to the lowest id) -- those live longest in packed columns.
    At most 14 chains.  The rule is fixed here, not tuned per case."""
    tot = np.asarray(nleap).reshape(C, -1).sum(1)
    top = sorted(range(C), key=lambda c: (-int(tot[c]), c))[:4]
    return sorted(set(edge_chains(C)) | set(top))


def _leaves(L, j):
    """leaves every chain takes in doubling j of a transition in which it takes L leapfrog steps in all"""
    return np.clip(np.asarray(L, dtype=np.int64) - ((1 << j) - 1), 0, 1 << j)


def _width(nact, C, cm):
    """NutsRun::pack"""
    g = 64 if cm else 128
    cw = -(-nact // g) * g
    if not cm and nact <= SK_NUSE:
        cw = nact
    return min(cw, C)


def packed_widths(nleap, C, cm, max_depth=MAX_DEPTH):
    """every column count Cw the products ran at, and every re-pack inside a doubling, from the leapfrog counts of the
    whole population (C x transitions), following NutsRun::pack and the checkpoints of NutsRun::transition.
    Returns (set of widths, list of (transition, doubling, leaves so far, chains before, chains after))"""
    nleap = np.asarray(nleap).reshape(C, -1)
    widths, repacks = {C}, []                                  # the step-size search and every transition open with all chains
    for t in range(nleap.shape[1]):
        nact = C
        for j in range(max_depth):
            k = _leaves(nleap[:, t], j)
            if j > 0:
                nact = int((k >= 1).sum())                     # the chains still growing after the last doubling
                if nact == 0:
                    break
            widths.add(_width(nact, C, cm))
            for m in range(16, 1 << j, 16):                    # checkpoint after leaf m (m < 2^j)
                na = int((k > m).sum())
                if na == 0:
                    break
                if 4 * na <= 3 * nact:
                    repacks.append((t, j, m, nact, na))
                    nact = na
                    widths.add(_width(nact, C, cm))
    return widths, repacks


def doublings_started(nleap, max_depth=MAX_DEPTH):
    """doublings the batch starts, all transitions: the first of every transition, and each one some chain takes a leaf in"""
    nleap = np.asarray(nleap)
    nleap = nleap.reshape(nleap.shape[0], -1)
    return sum(1 for t in range(nleap.shape[1]) for j in range(max_depth) if j == 0 or int(_leaves(nleap[:, t], j).max()) >= 1)


def expected_batched_leapfrogs(nleap, max_depth=MAX_DEPTH):
    """leapfrog steps the batch takes: every doubling that starts (some chain takes a leaf in it) runs until its
    longest chain has stopped, seen at the next checkpoint (every 16 leaves), or to its end"""
    nleap = np.asarray(nleap)
    nleap = nleap.reshape(nleap.shape[0], -1)
    total = 0
    for t in range(nleap.shape[1]):
        for j in range(max_depth):
            K = int(_leaves(nleap[:, t], j).max())
            if K < 1:
                break
            total += min(1 << j, 16 * -(-K // 16))
    return total


def golden_repack(name):
    """the oracle's leapfrog counts (C x transitions) of the whole population of a `repack` case"""
    with open(GOLDEN_REPACK) as f:
        return np.array(json.load(f)[name]["nleap"])
