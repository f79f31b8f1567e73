"""The designs of test_gpu_exact_component.py, checked on the CPU before the kernels see them, at sigma 0.8 and 0.2 with L from
the oracle: M = I + ZL' ZL / sigma^2 has no entry outside the blocks of the connected components of ZL's coupling graph, the
components have the counts the design functions return, cond(M) < 1e4, the dense float64 twin (tests/exact_gaussian_twin.py)
is within 1e-12 of its extended-precision form, and a per-component numpy evaluation mu*_c + chol(M_c)^-T z_c -- what
csrc/hmc_exact_comp.h computes -- is within 1e-12 of the twin.  Measured: the per-component evaluation 1.2e-16 ... 7.2e-16 of
max|U| from the twin, the twin within 4.6e-15 of extended precision, cond(M) <= 65.  A design that fails here does not test
the kernel."""
import numpy as np
import pytest

import exact_gaussian_twin as tw
from test_gpu_exact_component import DESIGNS, MEAN_DESIGNS, make
from test_la_component_wide_designs_cpu import components

NAMES = list(DESIGNS) + [n for n in MEAN_DESIGNS if n not in DESIGNS]
CHAINS, NSAMP = 5, 10                 # ten columns of normals: the properties do not depend on the column count


@pytest.fixture(scope="module")
def cases(orc):
    out = {}

    def get(name):
        if name not in out:
            d, counts = make(name)
            L = orc.gen_D(d["cov"], d["data"], d["eff_range"], d["theta"], chol=True)
            z = tw.normals(orc, d["Q"], 20240601, CHAINS, NSAMP, chain_offset=3, iter_idx=2)
            out[name] = (d, counts, L, z)
        return out[name]
    return get


@pytest.mark.parametrize("sigma", [0.8, 0.2])
@pytest.mark.parametrize("name", NAMES)
def test_component_evaluation_is_the_dense_draw(cases, name, sigma):
    d, (ncomp, max_vars, max_rows), L, z = cases(name)
    assert d["family"] == "gaussian" and d["link"] == "identity"
    M, b, ZL = tw.system(d["Z"], L, d["X"], d["y"], d["beta"], sigma)
    lab = components(ZL)
    roots, sizes = np.unique(lab, return_counts=True)
    rows = [int(np.count_nonzero((ZL[:, lab == r] != 0).any(axis=1))) for r in roots]
    assert (len(roots), int(sizes.max()), max(rows)) == (ncomp, max_vars, max_rows)
    assert not M[lab[:, None] != lab[None, :]].any()
    cond = np.linalg.cond(M)
    assert cond < 1e4
    U, mu = tw.twin(d["Z"], L, d["X"], d["y"], d["beta"], sigma, z)
    Ux, _ = tw.twin_extended(d["Z"], L, d["X"], d["y"], d["beta"], sigma, z)
    gap = float(np.abs(U - Ux).max() / np.abs(Ux).max())
    assert gap <= 1e-12
    V = np.empty_like(z)
    for r in roots:
        idx = np.nonzero(lab == r)[0]                    # ascending: the order the component plan keeps
        Mc = M[np.ix_(idx, idx)]
        Rc = np.linalg.cholesky(Mc)
        V[idx] = np.linalg.solve(Mc, b[idx])[:, None] + np.linalg.solve(Rc.T, z[idx])
    err = float(np.abs(L @ V - U).max() / np.abs(U).max())
    print("%s sigma %.1f: cond %.1f, twin vs extended %.2e, per component vs twin %.2e" % (name, sigma, cond, gap, err))
    assert err <= 1e-12
