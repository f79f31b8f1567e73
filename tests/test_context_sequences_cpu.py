"""The inputs of the context sequences (context_sequences.py) have the properties their cases are named for, checked
with the oracle and numpy alone: if one does not, the input is changed, not the assertion."""
import numpy as np
import pytest

import context_sequences as cs
import test_gpu_dense_products as dp


def _factorises(orc, d, theta):
    try:
        L = orc.gen_D(d["cov"], d["data"], d["eff_range"], np.asarray(theta, dtype=float), chol=True)
    except RuntimeError:
        return False
    return bool(np.all(np.isfinite(L)) and np.all(np.diag(L) > 0))


def test_every_good_theta_factorises_and_every_bad_one_is_refused(orc):
    for which, (d, good, bad) in cs.bad_thetas().items():
        assert _factorises(orc, d, good), which
        assert not _factorises(orc, d, bad), which
        with pytest.raises(RuntimeError):
            orc.mvn_ll(d["cov"], d["data"], d["eff_range"], bad, np.ones((d["Q"], 2)))
    d = cs.s1_design()
    for theta in (cs.THETA, cs.THETA2, cs.THETA3):
        assert _factorises(orc, d, theta) and _factorises(orc, cs.s3_design(), theta), theta
    for name, (d, theta2, _) in cs.s2_designs().items():
        assert _factorises(orc, d, d["theta"]) and _factorises(orc, d, theta2), name
    assert not _factorises(orc, cs.s3_design(), (-0.05, 0.1))


@pytest.fixture(scope="module")
def factors(orc):
    return cs.s1_factors(dp.oracle_L(orc, cs.s1_design()))


def test_band_ranges_restatement():
    A = np.zeros((170, 100))
    A[3, 40] = A[79, 70] = 1.0          # band 0: K tiles 1 and 2
    A[165, 99] = -2.0                   # band 2 (10 rows): the last, partial K tile
    assert cs.band_ranges(A) == [(1, 3), (0, 0), (3, 4)]


def test_the_structures_have_pairwise_different_ranges(factors):
    for direction in ("fwd", "bwd"):
        kr = {k: cs.band_ranges(factors[k] if direction == "fwd" else factors[k].T) for k in ("LA", "LB", "LD")}
        assert len(kr["LA"]) == 5                                         # 333 rows: four whole bands and 13 rows
        assert kr["LA"] != kr["LB"] and kr["LB"] != kr["LD"] and kr["LA"] != kr["LD"], (direction, kr)
        # LB: bands start at a later K tile than LA's
        assert any(b[0] > a[0] for a, b in zip(kr["LA"], kr["LB"])) if direction == "fwd" else \
            any(b[1] < a[1] for a, b in zip(kr["LA"], kr["LB"])), (direction, kr)
        assert [r == (0, 0) for r in kr["LD"]].count(True) == 1, (direction, kr["LD"])
        assert (0, 0) not in kr["LA"] and (0, 0) not in kr["LB"]
        for k in ("LA", "LB", "LD"):
            assert cs.band_rule(factors[k] if direction == "fwd" else factors[k].T), (direction, k)


def test_LC_fails_the_four_fifths_rule(factors):
    LC = factors["LC"]
    assert np.count_nonzero(np.triu(LC, 1)) > 0 and np.array_equal(np.tril(LC), np.tril(factors["LA"]))
    assert not cs.band_rule(LC) and not cs.band_rule(LC.T)
    full = [(0, -(-LC.shape[1] // cs.BK))] * 5
    assert cs.band_ranges(LC) == full and cs.band_ranges(LC.T) == full


def test_the_whole_band_shape_keeps_its_properties(orc):
    """Q = 2000: LA and LB differ in every direction and both pass the rule (test_s1_whole_band_form)"""
    F = cs.s1_factors(dp.oracle_L(orc, cs.s1_design(2000)))
    for A, B in ((F["LA"], F["LB"]), (F["LA"].T, F["LB"].T)):
        assert cs.band_ranges(A) != cs.band_ranges(B) and cs.band_rule(A) and cs.band_rule(B)


def test_the_sparse_designs_choose_the_forms_the_sequences_name():
    for name, (d, _, factored) in cs.s2_designs().items():
        nnz, nz, nl, form = cs.sparse_form(d)
        assert form == factored, (name, nnz, nz, nl)
        assert nz == np.count_nonzero(d["Z"]) and nnz >= nz
        dims = [dim for _, dim in cs.cov_blocks(d["cov"])]
        assert sum(dims) == d["Q"] and max(dims) <= 32, name            # small blocks: the sparse operator is possible
    g = cs.s2_designs()["gaussian"][0]
    assert (g["family"], g["link"]) == ("gaussian", "identity") and np.all(np.isfinite(g["y"]))


def test_same_is_bit_equality():
    a = dict(u=np.array([0.0, np.nan]), k=("band", "band"), d=dict(x=1.5))
    assert cs.same(a, dict(u=np.array([0.0, np.nan]), k=("band", "band"), d=dict(x=1.5)))
    assert not cs.same(a, dict(u=np.array([-0.0, np.nan]), k=("band", "band"), d=dict(x=1.5)))
    assert cs.diff(a, dict(u=np.array([0.0, np.nan]), k=("band", "dlds"), d=dict(x=1.5))) == ["/k"]
    assert not cs.same(1.0, 1.0 + 2.0 ** -52)
