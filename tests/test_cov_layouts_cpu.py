"""The CPU oracle on covariance layouts with more than one kind of block (tests/cov_layouts.py), against the
numpy definition written from the formula table of csrc/covspec.h: D entry by entry, its Cholesky factor, and
mvn_ll; and the three functions nothing else evaluates -- fexp0 (2), sqexp (4), sqexp0 (14) -- against numbers
written down by hand.  This pins the oracle independently of the kernels that tests/test_gpu_cov_layouts.py
compares with it."""
import numpy as np
import pytest

import cov_layouts as cl

NAMES = sorted(cl.LAYOUTS)
M_CPU = 70


def _wire(name):
    cov, data = cl.layout(cl.LAYOUTS[name][0])
    return cov, data, np.zeros(cov.shape[0])


def test_layouts_are_what_they_are_named_for():
    assert cl.starts(cl.MIXED) == [0, 1, 2, 3, 153, 158, 191, 223, 226, 233] and cl.total_dim(cl.MIXED) == 522
    assert [b[0] for b in cl.MIXED] == [1, 1, 1, 150, 5, 33, 32, 3, 7, 289]
    assert [cl.kind(b) for b in cl.MIXED] == ["diag"] * 3 + ["large", "small", "large", "small", "diag", "small", "large"]
    assert len(cl.MIXED_THETA) >= 8
    cov, data = cl.layout(cl.MIXED)
    assert cov.dtype == np.int32 and cov.flags.f_contiguous and cov.shape == (15, 5)
    assert data.size == sum(b[0] * sum(np.asarray(x).reshape(b[0], -1).shape[1] for _, x, _ in b[1]) for b in cl.MIXED)
    par = cov[:, 4]
    assert len(set(par[:3])) == 1                                       # the three 1 x 1 blocks share a parameter
    assert sum(par == 1) >= 3 and sum(par == 5) == 2                    # shared between blocks of different kinds
    assert [cov[cov[:, 0] == 9, 3].tolist(), cov[cov[:, 0] == 9, 2].tolist()] == [[1, 2, 1], [cl.GR, cl.FEXP, cl.AR1]]
    assert cl.starts(cl.TWO_LARGE_A) == [0, 300] and cl.starts(cl.TWO_LARGE_B) == [0, 161]
    assert [b[0] for b in cl.EDGE32] == [32, 33]


@pytest.mark.parametrize("name", NAMES + ["TEN_SLOTS"])
def test_from_wire_is_the_inverse_of_layout(name):
    blocks = cl.TEN_SLOTS if name == "TEN_SLOTS" else cl.LAYOUTS[name][0]
    back = cl.from_wire(*cl.layout(blocks))
    assert len(back) == len(blocks)
    for (dim, terms), (bdim, bterms) in zip(blocks, back):
        assert bdim == dim and len(bterms) == len(terms)
        for (fn, x, pi), (bfn, bx, bpi) in zip(terms, bterms):
            assert (bfn, bpi) == (fn, pi)
            assert np.array_equal(bx, np.asarray(x, dtype=np.float64).reshape(dim, -1))


def test_ten_slots_is_what_it_is_named_for():
    """two blocks of 6 and 40, a small and a large one, ten parameter slots each on the same ten parameters; both factorise in
    float64, with the condition numbers the layout's comment states; the score's reference evaluates it"""
    import mvn_grad_reference as gr
    blocks, theta = cl.TEN_SLOTS, cl.TEN_SLOTS_THETA
    assert "TEN_SLOTS" not in cl.LAYOUTS
    assert [b[0] for b in blocks] == [6, 40] and [cl.kind(b) for b in blocks] == ["small", "large"]
    cov, _ = cl.layout(blocks)
    for b in (0, 1):
        rows = cov[cov[:, 0] == b]
        assert rows[:, 2].tolist() == [cl.FEXP] * 5 and rows[:, 3].tolist() == [1] * 5 and rows[:, 4].tolist() == [0, 2, 4, 6, 8]
    assert theta.tolist() == [1.1, 0.9, 0.8, 1.3, 1.2, 0.7, 0.9, 1.1, 1.05, 0.6]
    for block, kappa in zip(blocks, (4.0, 24.4)):
        D = cl.block_matrix(block, theta)[0]
        L = cl.cholesky(D)
        assert np.abs(L @ L.T - D).max() < 1e-14 * np.abs(D).max() * block[0]
        print("TEN_SLOTS block of %d: kappa_2 = %.3f" % (block[0], np.linalg.cond(D, 2)))
        assert abs(np.linalg.cond(D, 2) - kappa) < 0.05
    u = cl.samples(blocks, 70, cl.TEN_SLOTS_SEED)
    assert u.shape == (46, 70)
    for w in (None, gr.weights(70)):
        value, grad, mag, kappa = gr.score(blocks, theta, u, w)
        assert np.isfinite(float(value)) and grad.shape == (10,) and np.all(np.isfinite(grad.astype(float))) and np.all(mag > 0)
        assert abs(kappa - 24.4) < 0.05


@pytest.mark.parametrize("name", NAMES)
def test_blocks_are_well_conditioned(name):
    """a condition on the inputs: every tolerance below assumes it"""
    for theta in cl.thetas(name):
        for block in cl.LAYOUTS[name][0]:
            D = cl.block_matrix(block, theta)[0]
            assert np.linalg.cond(D, 2) <= 1e4, (name, block[0])


def _worst(D, want, bound):
    """largest |D - want| as a multiple of the entrywise bound, and where"""
    ratio = np.abs(D - want) / np.where(bound > 0, bound, 1.0)
    at = np.unravel_index(ratio.argmax(), ratio.shape)
    return float(ratio[at]), tuple(int(i) for i in at)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_gen_D_is_the_definition(orc, name):
    """entry by entry within 2^-52 (8 + 2 sum_k |a_k|) |D_ij| of the definition (float64 numpy), and within the
    derived bound of its long-double value (cov_layouts.dense_definition: an exact reference needs 4.5 |a| for the
    squared arguments; against it the first bound is exceeded 1.34 times on far-apart points of the 300-dim sqexp
    block, by rounding alone)"""
    cov, data, eff = _wire(name)
    for ti, theta in enumerate(cl.thetas(name)):
        ref = cl.reference(name, ti)
        D = orc.gen_D(cov, data, eff, theta)
        worst, at = _worst(D, ref["D"], ref["bound"])
        assert worst <= 1.0, (name, ti, "definition", at, worst)
        worst, at = _worst(D, ref["exact"], ref["derived"])
        assert worst <= 1.0, (name, ti, "long-double value", at, worst)
        assert np.array_equal(D == 0, ref["D"] == 0)                    # nothing outside the blocks
        L = orc.gen_D(cov, data, eff, theta, chol=True)
        assert np.abs(L - ref["L"]).max() < 1e-10 * np.abs(ref["L"]).max()
        assert np.abs(L @ L.T - D).max() < 1e-13 * max(1.0, np.abs(D).max()) * D.shape[0]
        assert np.array_equal(np.triu(L, 1), np.zeros_like(L))
        assert np.array_equal(L == 0, np.tril(ref["D"] == 0) | np.triu(np.ones_like(L, dtype=bool), 1))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_mvn_ll_is_the_definition(orc, name):
    """1e-12 relative: condition number (<= 1e4) x unit roundoff, with margin"""
    cov, data, eff = _wire(name)
    blocks = cl.LAYOUTS[name][0]
    for m in (1, min(M_CPU, cl.COLUMNS[name])):
        u = cl.sample_matrix(name)[:, :m]
        for ti, theta in enumerate(cl.thetas(name)):
            want = cl.reference_ll(name, ti, m)
            got = orc.mvn_ll(cov, data, eff, theta, u)
            assert abs(got - want) <= 1e-12 * abs(want), (name, m, ti, got, want)
    # definition() itself, as the helper's callers see it
    Ds, val = cl.definition(blocks, cl.LAYOUTS[name][1], cl.sample_matrix(name)[:, :3])
    assert len(Ds) == len(blocks) and abs(val - cl.reference_ll(name, 0, 3)) <= 1e-15 * abs(val)


# e^-k, written down (not computed here)
E1, E2, E3, E4, E5 = 0.36787944117144233, 0.1353352832366127, 0.049787068367863944, 0.01831563888873418, 0.006737946999085467
E9, E16, E25 = 0.00012340980408667956, 1.1253517471925912e-07, 1.3887943864964021e-11


def _toeplitz(first):
    n = len(first)
    return np.array([[first[abs(i - j)] for j in range(n)] for i in range(n)])


@pytest.mark.parametrize("fn,theta,first", [
    (cl.FEXP0, [2.5], [1.0, E1, E2, E3, E4, E5]),                                   # exp(-d / t)
    (cl.SQEXP, [2.0, 2.5], [2.0, 2 * E1, 2 * E4, 2 * E9, 2 * E16, 2 * E25]),        # t0 exp(-d^2 / t1^2)
    (cl.SQEXP0, [2.5], [1.0, E1, E4, E9, E16, E25]),                                # exp(-d^2 / t^2)
])
def test_functions_2_4_14_by_hand(orc, fn, theta, first):
    """six points k (1.5, 2), k = 0..5: the distances are exactly 2.5 |i - j|, so with a range of 2.5 the exponent
    arguments are the integers |i - j| (their squares for the squared functions)"""
    xy = np.outer(np.arange(6.0), [1.5, 2.0])
    blocks = [(6, [(fn, xy, 0)])]
    cov, data = cl.layout(blocks)
    want = _toeplitz(first)
    D = orc.gen_D(cov, data, np.zeros(1), theta)
    assert np.allclose(D, want, rtol=2.0 ** -50, atol=0)
    assert np.allclose(cl.block_matrix(blocks[0], theta)[0], want, rtol=2.0 ** -50, atol=0)
    # the functions through the factorisation and the solve as well
    u = np.zeros(6); u[0] = 2.0
    _, val = cl.definition(blocks, theta, u)
    assert abs(orc.mvn_ll(cov, data, np.zeros(1), theta, u) - val) <= 1e-12 * abs(val)
