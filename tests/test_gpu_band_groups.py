"""The whole-band form of the banded HMC products with groups of one, two and three bands per workgroup
(csrc/band_plan.h deals whole bands into balanced groups), against the CPU oracle.

n = Q = 1000: 13 bands, the last of 40 rows -- the smallest size at which the whole-band form is chosen with
singles, pairs and triples in play.  3713 chains are 30 column tiles, the last a single column: 8 groups, singletons
and pairs (the mirror pairing made 7).  5400 chains are 43 column tiles: 5 groups of 2-3 bands.  Grouping changes no
arithmetic -- a band's sum is one ordered K loop whatever group it sits in, and a chain's draws depend on (seed,
chain id) only -- so the chains the two runs share are the same bits.

Tolerances are test_gpu_dense_products' own: log_prob / log_grad 1e-10 relative; chains: identical accept flags,
probabilities within 1e-9, samples within 1e-8 relative."""
import numpy as np
import pytest

from test_gpu_dense_products import (check_chains, check_log_prob_grad, context, design, run_chains, run_log_prob_grad,
                                     tile_columns)

pytestmark = pytest.mark.gpu

Q = 1000


def _assert_groups(plans, gn, nwg):
    for p in plans:
        assert p["used"] and p["built"] and p["paired"] and p["nred"] == 0 and p["nslots"] == 0, p
        assert p["nbands"] == 13 and p["gn"] == gn and p["nwg"] == nwg, p


@pytest.mark.parametrize("family,link", [("poisson", "log"), ("gaussian", "identity")])
def test_log_prob_grad_singles_and_pairs(orc, family, link):
    d = design(family, link, Q)
    V, lp, G, kinds, plans = run_log_prob_grad(d, 3713)
    assert kinds == ("band", "band")
    _assert_groups(plans, 30, 8)
    check_log_prob_grad(orc, d, lp, G, V, cols=tile_columns(3713))


@pytest.fixture(scope="module")
def chain_runs():
    """poisson-log chains at both counts: (design, {chains: (u, flags, probs)})"""
    d = design("poisson", "log", Q)
    runs = {}
    for C, gn, nwg in ((3713, 30, 8), (5400, 43, 5)):
        with context(d) as ctx:
            runs[C] = run_chains(ctx, d, C)
            assert ctx.last_kernels() == ("band", "band")
            _assert_groups((ctx.band_plan(C, "fwd"), ctx.band_plan(C, "bwd")), gn, nwg)
    return d, runs


def test_chains_pairs_and_triples(orc, chain_runs):
    d, runs = chain_runs
    u, flags, probs = runs[5400]
    check_chains(orc, d, u, flags, probs, [0, 127, 3712, 5399])


def test_grouping_changes_no_arithmetic(chain_runs):
    _, runs = chain_runs
    (u0, f0, p0), (u1, f1, p1) = runs[3713], runs[5400]
    assert np.array_equal(u0, u1[:, :3713])
    assert np.array_equal(f0, f1[:3713]) and np.array_equal(p0, p1[:3713])
