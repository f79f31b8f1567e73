"""GPU parity of the No-U-Turn sampler (csrc/nuts.h) against oracle/nuts.py where the chains pack, chunk and re-pack:
more chains than a wave, a column tile or a workgroup hold, more rows than one partial-sum chunk, and doublings deep
enough for the checkpoints inside them (cases and arithmetic: tests/nuts_cases.py; calibration on the CPU:
tests/test_nuts_cases_cpu.py).

Per case one run with all chains.  From its own traces: the packed widths the run went through (the regime the case
is named for), the batch's leapfrog count and how often it packed (diag `packs`: a re-pack leaves no other mark).  Against the oracle, chain by chain on nuts_cases.compared_chains: identical
tree depths and leapfrog counts, step size, acceptance statistic and draws within nuts_cases.tolerances.  Against the
few-chain path that tests/test_gpu_nuts.py pins: the same chains again in groups of 16."""
import functools

import numpy as np
import pytest

import nuts_cases as nc

pytestmark = pytest.mark.gpu

NAMES = list(nc.CASES)


def _sample(name, d, chains, offset):
    from glmmrmcml_amd import api
    c = nc.CASES[name]
    with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
        ctx.update_L(d["theta"])
        diag, tr = ctx.nuts_sample(d["beta"], c["vp"], c["warm"], c["draws"] * chains, c.get("seed", nc.SEED), chains=chains,
                                   chain_offset=offset, iter_idx=nc.ITER_IDX, max_treedepth=nc.MAX_DEPTH,
                                   adapt_delta=c["adapt_delta"], want_trace=True, metric=c["metric"])
        u = ctx.get_u()
        kernels = ctx.last_kernels()
    assert u.shape == (d["Q"], chains * c["draws"])
    return diag, tr, u, kernels


@functools.lru_cache(maxsize=None)
def _run(name):
    """the case's one run with all C chains (shared, not modified, by the tests below)"""
    d = nc.design(name)
    return (d,) + _sample(name, d, nc.CASES[name]["C"], 0)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """the oracle on the compared chains of the case: {chain: (draws of u, trace)}"""
    from oracle import oracle as orc
    orc.build()
    d, _, tr, _, _ = _run(name)
    inp = nc.oracle_inputs(orc, d)
    return {c: nc.oracle_chain(name, d, inp, c) for c in nc.compared_chains(nc.CASES[name]["C"], tr["depth"], tr["nleap"])}


@pytest.mark.parametrize("name", NAMES)
def test_run_visits_the_packed_widths_the_case_is_named_for(name):
    c = nc.CASES[name]
    _, _, tr, _, kernels = _run(name)
    assert (kernels[0] == "sparse") == c["cm"], kernels                     # chain-major state <=> sparse operator
    widths, repacks = nc.packed_widths(tr["nleap"], c["C"], c["cm"])
    print("%s: widths %s, %d re-packs inside a doubling %s" % (name, sorted(widths, reverse=True), len(repacks), repacks))
    assert set(c["widths"]) <= widths, sorted(widths)
    if c["streamed"]:
        assert min(widths) <= nc.SK_NUSE, sorted(widths)
    if c.get("repack"):
        assert len(repacks) >= 1
        assert np.array_equal(tr["nleap"], nc.golden_repack(name))        # the oracle's whole population
    assert tr["depth"].max() >= c["min_depth"]


@pytest.mark.parametrize("name", NAMES)
def test_compared_chains_match_oracle_transition_by_transition(name):
    c = nc.CASES[name]
    _, diag, tr, u, _ = _run(name)
    dpc = c["draws"]
    tol = nc.tolerances(name)
    chains = nc.compared_chains(c["C"], tr["depth"], tr["nleap"])
    want = set(nc.edge_chains(c["C"]))
    assert want <= set(chains) and len(chains) <= 14
    worst = np.zeros(3)
    ndiv = nhit = 0
    failed = []
    for ch, (uo, to) in sorted(_oracle(name).items()):
        assert np.array_equal(tr["depth"][ch], to["depth"]), (ch, tr["depth"][ch], to["depth"])
        assert np.array_equal(tr["nleap"][ch], to["nleap"]), (ch, tr["nleap"][ch], to["nleap"])
        dev = nc.deviations(tr["eps"][ch], tr["accept"][ch], u[:, ch * dpc:(ch + 1) * dpc], to["eps"], to["accept"], uo)
        worst = np.maximum(worst, dev)
        if not all(v < t for v, t in zip(dev, tol)):
            failed.append((ch, dev))
        ndiv += to["ndiv"]; nhit += to["nhit"]
    print("%s: chains %s worst eps %.2e (tol %.1e) accept %.2e (%.1e) draws %.2e (%.1e)" % (
        name, chains, worst[0], tol[0], worst[1], tol[1], worst[2], tol[2]))
    assert not failed, (failed, tol)
    # the compared chains' divergences and depth hits are part of the totals
    assert ndiv <= diag["divergent"] and nhit <= diag["treedepth_hits"]


@pytest.mark.parametrize("name", [n for n in NAMES if nc.CASES[n]["groups"]])
def test_whole_population_equals_groups_of_16(name):
    """every chain of the full run against the same chain in a batch of 16 (the streamed products on the dense
    operator, a single partly filled wave on the sparse one): identical integer traces, draws within the tolerance"""
    c = nc.CASES[name]
    d, _, tr, u, _ = _run(name)
    dpc, tol = c["draws"], nc.tolerances(name)
    worst = np.zeros(3)
    for g in range(-(-c["C"] // 16)):
        lo, n = 16 * g, min(16, c["C"] - 16 * g)
        _, trg, ug, _ = _sample(name, d, n, lo)
        assert np.array_equal(trg["depth"], tr["depth"][lo:lo + n]), g
        assert np.array_equal(trg["nleap"], tr["nleap"][lo:lo + n]), g
        for i in range(n):
            ch = lo + i
            dev = nc.deviations(tr["eps"][ch], tr["accept"][ch], u[:, ch * dpc:(ch + 1) * dpc], trg["eps"][i], trg["accept"][i],
                                ug[:, i * dpc:(i + 1) * dpc])
            worst = np.maximum(worst, dev)
            assert all(v < t for v, t in zip(dev, tol)), (ch, dev, tol)
    print("%s: full run against groups of 16, worst eps %.2e accept %.2e draws %.2e" % ((name,) + tuple(worst)))


@pytest.mark.parametrize("name", NAMES)
def test_diag_counts(name):
    c = nc.CASES[name]
    _, diag, tr, _, _ = _run(name)
    transitions = c["warm"] + c["draws"]
    assert tr["nleap"].shape == (c["C"], transitions)
    assert diag["batched_leapfrogs"] == nc.expected_batched_leapfrogs(tr["nleap"])
    assert diag["stepsize_search_leapfrogs"] > 0
    # NutsRun::pack runs once per round of a step-size search (one leapfrog step each), once per doubling, and once per
    # re-pack at a checkpoint inside a doubling
    repacks = nc.packed_widths(tr["nleap"], c["C"], c["cm"])[1]
    assert diag["packs"] == diag["stepsize_search_leapfrogs"] + nc.doublings_started(tr["nleap"]) + len(repacks)
    assert 0 <= diag["treedepth_hits"] <= c["C"] * transitions
    assert 0 <= diag["divergent"] <= c["C"] * transitions
    # only a tree of full depth can be a hit (one that has not turned at its last check)
    assert diag["treedepth_hits"] <= int((tr["depth"] == nc.MAX_DEPTH).sum())
