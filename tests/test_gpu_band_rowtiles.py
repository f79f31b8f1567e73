"""Row-tile extents of the banded HMC product kernel (csrc/dgemm_band.h, csrc/band_plan.h): inside a band's K-tile range
the MFMA waves issue, per 16-row tile, only the K substeps between the row tile's first and last nonzero.  Skipping
exact zeros changes no sum, so with the rule on (default) and off (GLMMR_MCML_BAND_ROWTILES=0: every K tile whole, the
earlier behaviour) the results must be the same bits -- in the 8-wave and in the feeder form, on whole-band and on
streamed plans, through the plain and through both sampler epilogues.  Each product is also held to the 1e-12 |A||B|
bound of test_gpu_dgemm against numpy, the extents the device scan recorded are compared with a numpy scan of the
operand, and the issued-MFMA count of the n = 200 triangular operands with its closed form."""
import ctypes as C

import numpy as np
import pytest

from glmmrmcml_amd import api, synth

pytestmark = pytest.mark.gpu

FORM_8WAVE, FORM_FEED = 0, 1
SWITCH = "GLMMR_MCML_BAND_ROWTILES"


def _band_ext(A, B, form):
    """(A @ B through the given form, extents (bands, 5, 2), MFMAs per 16-column strip the launch issued)"""
    from glmmrmcml_amd import _lib
    L = _lib.lib()
    M, K = A.shape
    N = B.shape[1]
    A = np.asfortranarray(A); B = np.asfortranarray(B); out = np.full((M, N), np.nan, order="F")
    ext = np.full(((M + 79) // 80, 5, 2), -1, dtype=np.int32)
    issued = C.c_longlong(-1)
    _lib.check(L.glmmr_mcml_dbg_dgemm_band_ext(M, N, K, A.ctypes.data, M, B.ctypes.data, K, out.ctypes.data, M, form,
                                               ext.ctypes.data, int(ext.size), C.byref(issued)))
    return out, ext, issued.value


def _scan(A):
    """numpy restatement of the device scan: (extents (bands, 5, 2), K tiles of 32 over the bands)"""
    M, K = A.shape
    nb = (M + 79) // 80
    ext = np.zeros((nb, 5, 2), dtype=np.int32)
    tiles = 0
    for b in range(nb):
        cols = np.flatnonzero(np.any(A[80 * b:80 * b + 80] != 0.0, axis=0))
        tiles += 0 if cols.size == 0 else cols[-1] // 32 - cols[0] // 32 + 1
        for i in range(5):
            c = np.flatnonzero(np.any(A[80 * b + 16 * i:min(80 * b + 16 * i + 16, M)] != 0.0, axis=0))
            if c.size:
                ext[b, i] = (c[0] // 4, c[-1] // 4 + 1)
    return ext, int(tiles)


def _check(monkeypatch, A, B):
    """switch on against off in both forms -> (extents, MFMAs issued with the rule on, K tiles)"""
    want_ext, tiles = _scan(A)
    want = A @ B
    bound = 1e-12 * (np.abs(A) @ np.abs(B)) + 1e-300
    got = {}
    for sw in ("1", "0"):
        monkeypatch.setenv(SWITCH, sw)
        for form in (FORM_8WAVE, FORM_FEED):
            out, ext, issued = _band_ext(A, B, form)
            assert np.array_equal(ext, want_ext)
            assert issued == (int((want_ext[:, :, 1] - want_ext[:, :, 0]).sum()) if sw == "1" else 40 * tiles)
            assert np.all(np.abs(out - want) <= bound)
            got[sw, form] = out
    monkeypatch.delenv(SWITCH, raising=False)
    for form in (FORM_8WAVE, FORM_FEED):
        assert np.array_equal(got["1", form], got["0", form])
    assert np.array_equal(got["1", FORM_8WAVE], got["1", FORM_FEED])
    return want_ext, int((want_ext[:, :, 1] - want_ext[:, :, 0]).sum()), tiles


@pytest.fixture(scope="module")
def operands():
    rng = np.random.default_rng(200)
    return rng.normal(size=(200, 200)), rng.normal(size=(200, 130))


@pytest.mark.parametrize("N", [128, 130])
def test_lower_triangular(monkeypatch, operands, N):
    """bands 0, 1 and 2: the diagonal at both alignments to the K tiles and a last band of 40 rows (2.5 row tiles)"""
    A, B = operands
    ext, issued, tiles = _check(monkeypatch, np.tril(A), B[:, :N])
    assert issued == 60 + 160 + (44 + 48 + 50) and tiles == 3 + 5 + 7
    assert np.array_equal(ext[2, 3:], np.zeros((2, 2)))


@pytest.mark.parametrize("N", [128, 130])
def test_upper_triangular(monkeypatch, operands, N):
    """the backward operand: every row tile starts 4 substeps after the one above it, K is padded 200 -> 224 and the
    last K tile holds two substeps"""
    A, B = operands
    ext, issued, tiles = _check(monkeypatch, np.triu(A), B[:, :N])
    assert issued == sum(50 - 4 * t for t in range(13)) and tiles == 7 + 5 + 2


def test_one_live_row_tile(monkeypatch, operands):
    """M = 176: the last band has one row tile with rows and four without"""
    A, B = operands
    for T in (np.tril(A[:176, :176]), np.triu(A[:176, :176])):
        ext, _, _ = _check(monkeypatch, T, B[:176])
        assert ext[2, 0, 1] > ext[2, 0, 0] and np.array_equal(ext[2, 1:], np.zeros((4, 2)))


def test_block_operand(monkeypatch):
    """no triangle: band 0's row tiles differ at both ends and none of its K tiles is interior; row tile 2 of band 0 holds
    one entry; a zero row and zero columns lie inside band 1's extents; band 2 is empty; band 3 is dense in columns
    37 .. 210 (interior tiles 2 .. 5 between two edge tiles); band 4 has 13 rows"""
    rng = np.random.default_rng(333)
    M, K, N = 333, 250, 130
    A = rng.normal(size=(M, K))
    r, c = np.indices((M, K))
    t = r // 16
    keep = (c >= 3 * t + r % 5) & (c < 40 + 7 * t + r % 3) & ~((c >= 50) & (c < 58))
    keep[32:48] = False; keep[40, 77] = True
    keep[100] = False
    keep[160:240] = False
    keep[240:320] = (c[240:320] >= 37) & (c[240:320] <= 210)
    A[~keep] = 0.0
    ext, issued, tiles = _check(monkeypatch, A, rng.normal(size=(K, N)))
    assert len(set(ext[0, :, 0])) > 2 and len(set(ext[0, :, 1])) > 2 and tuple(ext[0, 2]) == (19, 20)
    assert np.array_equal(ext[2], np.zeros((5, 2))) and np.array_equal(ext[3], [[9, 53]] * 5)
    assert issued < 40 * tiles


def test_streamed_runs_cut_inside_edge_regions(monkeypatch):
    """one column tile at M = K = 2500: runs of several K tiles, a band's run ends where the next one's begins -- inside
    the diagonal's edge region for some -- and the pieces go through k_band_reduce"""
    rng = np.random.default_rng(2500)
    A = rng.normal(size=(2500, 2500)); B = rng.normal(size=(2500, 128))
    _check(monkeypatch, np.tril(A), B)
    _check(monkeypatch, np.triu(A), B)


def test_whole_band_plan(monkeypatch, operands):
    """the same n = 200 triangles on the whole-band plan (2 groups x 103 column tiles >= 205 workgroups)"""
    A, _ = operands
    B = np.random.default_rng(13186).normal(size=(200, 13186))
    _check(monkeypatch, np.tril(A), B)
    _check(monkeypatch, np.triu(A), B)


def test_sampler_is_bit_identical_with_and_without(monkeypatch):
    """both sampler epilogues: 130 gaussian-identity chains at n = Q = 200, 3 proposals of up to 10 leapfrog steps"""
    d = synth.geospatial(200)
    runs = []
    for sw in (None, "0"):
        if sw is None:
            monkeypatch.delenv(SWITCH, raising=False)
        else:
            monkeypatch.setenv(SWITCH, sw)
        with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
            ctx.update_L(d["theta"])
            ctx.profile(True)
            diag, flags, probs = ctx.hmc_sample(d["beta"], d["sigma"], 2, 130, 100.0, 10, 0.9, seed=17, chains=130,
                                                want_trace=True)
            assert ctx.last_kernels() == ("band", "band")
            prof = ctx.profile(False)
            fwd = ctx.band_extents("fwd"); bwd = ctx.band_extents("bwd")
            runs.append((ctx.get_u(), flags, probs, diag, prof))
    monkeypatch.delenv(SWITCH, raising=False)
    # the host copy of the extents: the triangular closed forms, and the flops the profile reports are the issued ones
    assert fwd[1:] == (60 + 160 + 142, 40 * 15) and bwd[1:] == (sum(50 - 4 * t for t in range(13)), 40 * 14)
    assert np.array_equal(fwd[0], _scan(np.tril(np.ones((200, 200))))[0])
    assert np.array_equal(bwd[0], _scan(np.triu(np.ones((200, 200))))[0])
    (u0, f0, p0, d0, pr0), (u1, f1, p1, d1, pr1) = runs
    assert (pr0["fwd_flops"], pr0["bwd_flops"]) == (2048.0 * fwd[1] * 130 / 16, 2048.0 * bwd[1] * 130 / 16)
    assert (pr1["fwd_flops"], pr1["bwd_flops"]) == (2048.0 * fwd[2] * 130 / 16, 2048.0 * bwd[2] * 130 / 16)
    assert pr0["dense_flops"] == pr1["dense_flops"] == 2.0 * 200 * 200 * 130
    assert np.isfinite(u0).all() and d0["leapfrog_total"] > 0
    assert u0.tobytes() == u1.tobytes() and f0.tobytes() == f1.tobytes() and p0.tobytes() == p1.tobytes()
    assert d0 == d1
