"""The designs of test_gpu_la_component_wide.py sections 1 and 2, checked on the CPU with oracle/la.py before the kernel
sees them: M = ZL' W ZL + I has no entry outside the blocks of the connected components of ZL's coupling graph, the
components have the counts the GPU test asserts, sum_c slogdet(M_c) equals slogdet(M) to 1e-13 relative, and the Newton
step is finite.  A design that fails here does not test the component operator."""
import numpy as np
import pytest

from test_gpu_la_component import _oracle
from test_gpu_la_component_wide import ABOVE, ABOVE_IDS, wide_design

DESIGNS = ABOVE + [("paired_ar1", "poisson", "log"), ("paired_ar1", "binomial", "logit")]


def components(ZL):
    """labels of the connected components of the graph that joins the variables of every row of ZL"""
    Q = ZL.shape[1]
    parent = list(range(Q))

    def find(q):
        while parent[q] != q:
            parent[q] = parent[parent[q]]
            q = parent[q]
        return q

    for row in ZL:
        nz = np.nonzero(row)[0]
        for j in nz[1:]:
            a, b = find(int(nz[0])), find(int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.array([find(q) for q in range(Q)])


@pytest.mark.parametrize("name,family,link", DESIGNS, ids=ABOVE_IDS + ["paired_ar1-poisson-log", "paired_ar1-binomial-logit"])
def test_design_is_block_diagonal_over_its_components(orc, name, family, link):
    d, (ncomp, max_vars, max_rows) = wide_design(name, family, link)
    m = _oracle(d)
    m.v = np.random.default_rng(23).normal(size=d["Q"]) * 0.2
    m.update_W(True)
    lab = components(m.ZL)
    roots, sizes = np.unique(lab, return_counts=True)
    rows = [int(np.count_nonzero((m.ZL[:, lab == r] != 0).any(axis=1))) for r in roots]
    assert (len(roots), int(sizes.max()), max(rows)) == (ncomp, max_vars, max_rows)
    M = m.ZL.T @ (m.W[:, None] * m.ZL) + np.eye(d["Q"])
    assert not M[lab[:, None] != lab[None, :]].any()
    sign, whole = np.linalg.slogdet(M)
    parts = [np.linalg.slogdet(M[np.ix_(lab == r, lab == r)]) for r in roots]
    assert sign == 1 and all(s == 1 for s, _ in parts)
    assert sum(v for _, v in parts) == pytest.approx(whole, rel=1e-13)
    m.mcnr_b()
    assert np.all(np.isfinite(m.v)) and np.all(np.isfinite(m.beta)) and np.isfinite(m.sigma)
