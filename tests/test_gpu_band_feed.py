"""The two forms of the banded HMC product kernel (csrc/dgemm_band.h) against each other, bit for bit: the 8-wave
kernel, whose waves each load and multiply, and the feeder form -- four MFMA waves with a 80 x 32 strip each, fed by
four DMA waves.  Every output element is accumulated by one wave over K in the same order by the same instruction in
both, so the results must be the same bits; each is also held to the 1e-12 |A||B| bound of test_gpu_dgemm against numpy.

Shapes: the smallest at which the whole-band plan is chosen (pairs of bands x column tiles >= 205 workgroups) with a
last band of 10 rows, a last column tile of 96 columns and K no multiple of 32; a narrow band with K loops of 1, 2 and
3 tiles and whole empty bands (nk = 0 items: the epilogue alone); the streamed plan's shapes -- one tile with one row /
column / K column over, runs cut inside bands with raw accumulator tiles through k_band_reduce."""
import ctypes as C

import numpy as np
import pytest

from glmmrmcml_amd import api, synth

pytestmark = pytest.mark.gpu

dp = C.POINTER(C.c_double)
FORM_8WAVE, FORM_FEED = 0, 1


def _band_form(A, B, form):
    """(A @ B through the given form of the kernel, K tiles multiplied, whether the plan was whole-band)"""
    from glmmrmcml_amd import _lib
    L = _lib.lib()
    M, K = A.shape
    N = B.shape[1]
    A = np.asfortranarray(A); B = np.asfortranarray(B); out = np.full((M, N), np.nan, order="F")
    tiles = C.c_int(); whole = C.c_int(-1)
    _lib.check(L.glmmr_mcml_dbg_dgemm_band_form(M, N, K, A.ctypes.data_as(dp), M, B.ctypes.data_as(dp), K,
                                                out.ctypes.data_as(dp), M, C.byref(tiles), form, C.byref(whole)))
    return out, tiles.value, whole.value


def _check_forms(A, B, whole_band):
    old, t0, w0 = _band_form(A, B, FORM_8WAVE)
    new, t1, w1 = _band_form(A, B, FORM_FEED)
    assert (w0, w1) == (int(whole_band),) * 2 and t0 == t1
    bound = 1e-12 * (np.abs(A) @ np.abs(B)) + 1e-300
    want = A @ B
    assert np.all(np.abs(old - want) <= bound)
    assert np.all(np.abs(new - want) <= bound)
    assert np.array_equal(old, new)
    return new, t1


@pytest.fixture(scope="module")
def whole_band_operands():
    rng = np.random.default_rng(1690)
    return rng.normal(size=(1690, 1690)), rng.normal(size=(1690, 2400))


def test_lower_triangular_whole_band(whole_band_operands):
    """22 bands (the last of 10 rows) x 19 column tiles (the last of 96 columns), groups of one or two bands, band 0
    with a 3-tile K loop"""
    A, B = whole_band_operands
    _, tiles = _check_forms(np.tril(A), B, whole_band=True)
    assert tiles < 0.6 * 22 * 53


def test_upper_triangular_whole_band(whole_band_operands):
    """the backward product's operand"""
    A, B = whole_band_operands
    _check_forms(np.triu(A), B, whole_band=True)


def test_narrow_band_and_empty_bands():
    """40 bands x 11 column tiles, several bands per group; a diagonal band of half-width 20; two whole bands of
    zeros: items without a K tile, whose epilogue still has to write exact zeros.  An 80-row band of that operand
    spans 120 columns, 4 or 5 K tiles (2 for the last band of 10 rows); the K loops of 1, 2 and 3 tiles (a ring that
    never fills, fills exactly, wraps once) come from three bands cut down to that many tiles' columns."""
    rng = np.random.default_rng(3130)
    M = K = 3130
    N = 1403
    A = rng.normal(size=(M, K))
    i, k = np.indices((M, K))
    A[np.abs(k - i) > 20] = 0.0
    A[800:960, :] = 0.0
    for band, (c0, c1) in ((5, (416, 448)), (6, (480, 544)), (7, (544, 640))):
        A[80 * band:80 * band + 80, :c0] = 0.0
        A[80 * band:80 * band + 80, c1:] = 0.0
    nk = []
    for r0 in range(0, M, 80):
        cols = np.flatnonzero(np.any(A[r0:r0 + 80] != 0.0, axis=0))
        nk.append(0 if cols.size == 0 else cols[-1] // 32 - cols[0] // 32 + 1)
    assert nk[5:8] == [1, 2, 3] and nk[10:12] == [0, 0] and nk[-1] == 2 and set(nk) == {0, 1, 2, 3, 4, 5}
    got, tiles = _check_forms(A, rng.normal(size=(K, N)), whole_band=True)
    assert tiles == sum(nk)
    assert np.all(got[800:960, :] == 0.0)


@pytest.mark.parametrize("M,N,K", [(81, 129, 33), (333, 77, 250), (2500, 128, 2500)])
def test_streamed_shapes(M, N, K):
    rng = np.random.default_rng(M + N + K)
    _check_forms(np.tril(rng.normal(size=(M, K))), rng.normal(size=(K, N)), whole_band=False)


def test_sampler_is_bit_identical_with_either_form(monkeypatch):
    """the real epilogues: 2400 gaussian-identity chains at n = 1690, 3 proposals of 10 leapfrog steps, with the
    default form and with GLMMR_MCML_BAND_FEED=0"""
    d = synth.geospatial(1690)
    runs = []
    for sw in (None, "0"):
        if sw is None:
            monkeypatch.delenv("GLMMR_MCML_BAND_FEED", raising=False)
        else:
            monkeypatch.setenv("GLMMR_MCML_BAND_FEED", sw)
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
            ctx.update_L(d["theta"])
            # one draw per chain behind 2 warm-up proposals; lambda / e is far above max_steps = 10 for any step size
            diag = ctx.hmc_sample(d["beta"], d["sigma"], 2, 2400, 100.0, 10, 0.9, seed=17, chains=2400)
            assert ctx.last_kernels() == ("band", "band")
            assert ctx.band_plan(2400, "fwd")["paired"] and ctx.band_plan(2400, "bwd")["paired"]
            runs.append((ctx.get_u(), diag))
    monkeypatch.delenv("GLMMR_MCML_BAND_FEED", raising=False)
    (u0, d0), (u1, d1) = runs
    assert np.isfinite(u0).all() and d0["leapfrog_total"] > 0
    assert np.array_equal(u0, u1)
    assert d0["accept_rate"] == d1["accept_rate"]
    assert (d0["max_steps_used"], d0["leapfrog_total"]) == (d1["max_steps_used"], d1["leapfrog_total"])
