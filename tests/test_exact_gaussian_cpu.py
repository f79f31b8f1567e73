"""Pins the float64 twin of the exact conditional draws (tests/exact_gaussian_twin.py), which the GPU test holds the device
path to at 1e-10: M mu* = b to 1e-12 relative, and the twin within 1e-12 max|U| of an extended-precision (np.longdouble,
hand-rolled factor and solves) evaluation at every shape and column count the GPU test uses.  Measured gap: 3.5e-16 ...
4.2e-15 at these shapes, cond(M) <= 450."""
import numpy as np
import pytest

import exact_gaussian_twin as tw


@pytest.fixture(scope="module")
def cases(orc):
    """every shape once: the design, its factor L from the oracle, the normals of the widest column set"""
    out = {}
    for name, make in tw.SHAPES.items():
        d = make()
        L = orc.gen_D(d["cov"], d["data"], d["eff_range"], d["theta"], chol=True)
        out[name] = (d, L)
    return out


@pytest.mark.parametrize("name", list(tw.SHAPES))
def test_twin_solves_the_normal_equations_and_matches_extended_precision(orc, cases, name):
    d, L = cases[name]
    Q = d["Q"]
    M, b, _ = tw.system(d["Z"], L, d["X"], d["y"], d["beta"], d["sigma"])
    assert np.linalg.cond(M) < 1e4                      # the bound below is for a well-conditioned M
    for chains, nsamp in tw.COLUMNS:
        z = tw.normals(orc, Q, 20240601, chains, nsamp, chain_offset=3, iter_idx=2)
        assert z.shape == (Q, tw.layout(chains, nsamp)[2])
        U, mu = tw.twin(d["Z"], L, d["X"], d["y"], d["beta"], d["sigma"], z)
        res = np.abs(M @ mu - b).max()
        print("%s, %d columns: |M mu* - b| / |b| = %.2e" % (name, z.shape[1], res / np.abs(b).max()))
        assert res <= 1e-12 * np.abs(b).max()
        Ux, mux = tw.twin_extended(d["Z"], L, d["X"], d["y"], d["beta"], d["sigma"], z)
        gap = float(np.abs(U - Ux).max() / np.abs(Ux).max())
        print("%s, %d columns: twin vs extended precision %.2e" % (name, z.shape[1], gap))
        assert gap <= 1e-12
        assert float(np.abs(mu - mux).max()) <= 1e-12 * float(np.abs(mux).max())


def test_normals_follow_the_hmc_column_layout(orc):
    """C > 1: column j = chain * d + draw; C = 1: chain 0, draw j; a chain offset shifts the chain id"""
    z = tw.normals(orc, 5, 9, 4, 8, chain_offset=2, iter_idx=1)       # d = 2
    assert z.shape == (5, 8)
    assert z[3, 5] == orc.normal(9, 3, 2 + 2, 1, 16 + 8)
    z1 = tw.normals(orc, 5, 9, 1, 3)
    assert z1.shape == (5, 4) and z1[2, 3] == orc.normal(9, 2, 0, 3, 8)
    both = tw.normals(orc, 5, 9, 4, 4)
    assert np.array_equal(both[:, 2:], tw.normals(orc, 5, 9, 2, 2, chain_offset=2))
