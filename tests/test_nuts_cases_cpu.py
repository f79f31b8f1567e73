"""Calibration of the NUTS packing cases (tests/nuts_cases.py) on the CPU oracle alone.

Every case is run on the edge chains and chains 1..8, once as it is and once on a twin whose ZL is multiplied entrywise
by 1 + 1e-14 N(0, 1).  The integer traces (tree depth, leapfrog count) of every such chain must be identical between
the two: a case in which a perturbation of the last digits flips a tree decision cannot be compared with the device
transition by transition, and is a bad input (change its seed, not the rule).  The deviations of step size, acceptance
statistic and draws between the two are what rounding alone does to the case; nuts_cases.TWIN_D records them and
tests/test_gpu_nuts_packing.py takes its tolerances from there.

The arithmetic that predicts the device's packing from leapfrog counts (packed_widths, expected_batched_leapfrogs,
compared_chains) is pinned on hand-made counts, and the recorded population of the `repack` case must hold a re-pack
inside a doubling."""
import functools

import numpy as np
import pytest

import nuts_cases as nc

NAMES = list(nc.CASES)


@functools.lru_cache(maxsize=None)
def _calibration(name):
    from oracle import oracle as orc
    orc.build()
    C = nc.CASES[name]["C"]
    d = nc.design(name)
    inp = nc.oracle_inputs(orc, d)
    ZLt = nc.twin(inp[0])
    chains = sorted(set(nc.edge_chains(C)) | {c for c in range(1, 9) if c < C})
    out = {}
    for c in chains:
        out[c] = (nc.oracle_chain(name, d, inp, c), nc.oracle_chain(name, d, inp, c, ZL=ZLt))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_integer_traces_survive_a_perturbation_of_the_last_digits(name):
    for c, ((_, a), (_, b)) in _calibration(name).items():
        assert np.array_equal(a["depth"], b["depth"]), (c, a["depth"], b["depth"])
        assert np.array_equal(a["nleap"], b["nleap"]), (c, a["nleap"], b["nleap"])
        assert a["ndiv"] == b["ndiv"] and a["nhit"] == b["nhit"]


@pytest.mark.parametrize("name", NAMES)
def test_cases_reach_their_depths(name):
    depth = np.array([a["depth"] for (_, a), _ in _calibration(name).values()])
    assert depth.max() >= nc.CASES[name]["min_depth"], depth.max()
    assert depth.max() <= nc.MAX_DEPTH
    assert max(len(set(depth[:, t])) for t in range(depth.shape[1])) >= 3     # chains stop at different doublings


@pytest.mark.parametrize("name", NAMES)
def test_twin_deviations_stay_within_twice_the_recorded_ones(name):
    D = np.zeros(3)
    for (ua, a), (ub, b) in _calibration(name).values():
        D = np.maximum(D, nc.deviations(b["eps"], b["accept"], ub, a["eps"], a["accept"], ua))
    print("%s twin deviations: eps %.2e accept %.2e draws %.2e" % ((name,) + tuple(D)))
    rec = nc.TWIN_D[name]
    assert D[0] < 2 * rec["eps"] and D[1] < 2 * rec["accept"] and D[2] < 2 * rec["draws"], (tuple(D), rec)


def test_compared_chains_rule():
    nleap = np.ones((300, 3), dtype=int)
    nleap[[7, 200, 201, 299], :] = 5
    nleap[40, 0] = 13                                        # ties: 7, 200, 201, 299 at 15 against 40 at 15 -> lowest ids
    got = nc.compared_chains(300, None, nleap)
    assert got == sorted({0, 15, 16, 63, 64, 127, 128, 255, 256, 299, 7, 40, 200, 201})
    assert len(got) <= 14
    assert nc.compared_chains(40, None, np.arange(40)[:, None]) == [0, 15, 16, 36, 37, 38, 39]


def test_packed_widths_on_hand_made_counts():
    # one transition, 300 chains: 100 stop after the first doubling (1 leaf), 72 after the second (3), 112 after the
    # third (7), 16 go on to doubling 5 (31 + 32 = 63 leaves)
    L = np.r_[np.full(100, 1), np.full(72, 3), np.full(112, 7), np.full(16, 63)][:, None]
    w, rp = nc.packed_widths(L, 300, cm=False)
    assert w == {300, 256, 128, 16} and rp == []             # 300 | 200 -> 256 | 128 -> 128 | 16 streamed
    w, rp = nc.packed_widths(L, 300, cm=True)
    assert w == {300, 256, 128, 64} and rp == []             # waves of 64: 200 -> 256, 128 -> 128, 16 -> 64
    # doubling 5 (32 leaves): of 40 chains that start it, 12 stop within its first 16 leaves: 4 * 28 <= 3 * 40, re-pack
    L = np.r_[np.full(88, 31), np.full(12, 31 + 9), np.full(28, 63)][:, None]
    w, rp = nc.packed_widths(L, 128, cm=False)
    assert rp == [(0, 5, 16, 40, 28)] and w == {128}
    # 9 stop: 4 * 31 > 3 * 40, no re-pack
    L = np.r_[np.full(88, 31), np.full(9, 31 + 9), np.full(31, 63)][:, None]
    assert nc.packed_widths(L, 128, cm=False)[1] == []
    # a chain that stops exactly at the checkpoint (16 leaves taken) no longer counts
    L = np.r_[np.full(88, 31), np.full(12, 31 + 16), np.full(28, 63)][:, None]
    assert nc.packed_widths(L, 128, cm=False)[1] == [(0, 5, 16, 40, 28)]
    # doubling 6: two checkpoints can re-pack one after the other, the second against the re-packed count
    L = np.r_[np.full(64, 63), np.full(16, 63 + 5), np.full(12, 63 + 20), np.full(36, 127)][:, None]
    assert nc.packed_widths(L, 128, cm=False)[1] == [(0, 6, 16, 64, 48), (0, 6, 32, 48, 36)]


def test_expected_batched_leapfrogs_on_hand_made_counts():
    # the batch runs 1 + 2 + 4 leaves, then doubling 3 to its end (8 < 16: no checkpoint inside)
    assert nc.expected_batched_leapfrogs(np.array([[1], [3], [7 + 2]])) == 15
    # doubling 5: the longest chain takes 9 of 32 leaves, the checkpoint after 16 sees nobody left
    assert nc.expected_batched_leapfrogs(np.array([[31 + 9], [3]])) == 31 + 16
    # 17 leaves: seen at the end of the doubling (32 is no checkpoint); doubling 6 with 33 leaves: 48
    assert nc.expected_batched_leapfrogs(np.array([[31 + 17]])) == 63
    assert nc.expected_batched_leapfrogs(np.array([[63 + 33]])) == 63 + 48
    # a tree of full depth does not start another doubling; transitions add up
    assert nc.expected_batched_leapfrogs(np.array([[255, 1]])) == 256
    assert nc.expected_batched_leapfrogs(np.array([[7]]), max_depth=3) == 7
    # doublings started: every transition opens doubling 0; a later one counts when some chain takes a leaf in it
    assert nc.doublings_started(np.array([[1], [3], [7 + 2]])) == 4 and nc.doublings_started(np.array([[31 + 9], [3]])) == 6
    assert nc.doublings_started(np.array([[255, 1]])) == 9 and nc.doublings_started(np.array([[7]]), max_depth=3) == 3


@pytest.mark.parametrize("name", [n for n in NAMES if nc.CASES[n].get("repack")])
def test_recorded_repack_population_holds_a_repack_inside_a_doubling(name):
    c = nc.CASES[name]
    nleap = nc.golden_repack(name)
    assert c["C"] >= 128 and nleap.shape == (c["C"], c["warm"] + c["draws"])
    widths, repacks = nc.packed_widths(nleap, c["C"], c["cm"])
    assert len(repacks) == c["repack"] and all(j >= 5 and 0 < 4 * na <= 3 * nb for _, j, _, nb, na in repacks)
    assert set(c["widths"]) <= widths
    # the recorded counts are the oracle's: the chains of the calibration run reproduce their rows
    for ch, ((_, a), _) in _calibration(name).items():
        assert np.array_equal(a["nleap"], nleap[ch]), ch
