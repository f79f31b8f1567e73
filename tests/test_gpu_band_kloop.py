"""The K loop of the banded HMC product kernel (csrc/dgemm_band.h) where a misplaced operand read or wait shows first:
short items, the ring's wrap, the guard behind an item's last tile, edge tiles at both ends of a K range.  The MFMA waves
issue the reads of the next K substep between the MFMAs of the current one, and the first reads of the next tile behind
the barrier between the MFMAs of the last substep; every accumulator still sees the same MFMAs in the same order with
the same operands, so the bits are those of the library of the commit named in tests/golden/band_kloop_bits.json
(tests/golden/make_band_kloop_bits.py: recorded from that library, never from the code under test).

Cases, each through both forms of the kernel (hook _band_form of test_gpu_band_feed.py):
  * a banded operand, M = 1090 (13 whole bands and one of 50 rows), K = 390 (12 K tiles and 6 columns), on the
    whole-band plan (N = 3840: 7 mirror pairs x 30 column tiles x 5 >= 4 x 256, band_plan.h; 14 bands in 8 groups of one
    to three).  Band b's nonzeros lie in LEN[b % 7] = 0, 1, 2, 3, 4, 5, 7 K tiles; the first and the last nonzero column
    of every 16-row tile lie strictly inside a K tile, at a column that depends on the row tile, so the K range of a
    band begins and ends with edge tiles; row tile 2 of every odd band is empty (an extent without a substep), and the
    bands without a K tile make items that are and are not preceded by a prefetch of their ring stages;
  * the same operand at N = 77: the streamed plan, runs cut inside bands;
  * the streamed shapes (81, 129, 33) and (333, 77, 250) of test_gpu_band_bits.py with the operand UPPER triangular, the
    backward product's shape (recorded there lower triangular only);
  * the sampler through the real epilogues: synth.geospatial(640, seed=1), 1024 chains, 3 warm-up proposals and one
    draw, 10 leapfrog steps.
Next to every digest the product is held to |C - A B| <= gamma_K |A| |B| elementwise against numpy, gamma_K =
K u / (1 - K u), u = 2^-53: the bound of a K-term inner product in any order of summation (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.1), K being the number of terms, so nothing in it is measured."""
import json
import os

import numpy as np
import pytest

from glmmrmcml_amd import api, synth
from test_gpu_band_bits import FORMS, sha256
from test_gpu_band_feed import _band_form

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "band_kloop_bits.json")
M_BANDED, K_BANDED = 1090, 390
LEN = (0, 1, 2, 3, 4, 5, 7)                 # K tiles of band b: LEN[b % 7]
FIRST = (0, 3, 7, 10, 8, 2, 6)              # first K tile of band b: FIRST[b % 7]; 6 + 7 = 13 reaches the ragged last tile


def banded_operand():
    """A (1090 x 390): see the module docstring; (A, K tiles per band)"""
    rng = np.random.default_rng(1090)
    A = np.zeros((M_BANDED, K_BANDED))
    nk = []
    for band, r0 in enumerate(range(0, M_BANDED, 80)):
        n, t0 = LEN[band % 7], FIRST[band % 7]
        nk.append(n)
        if n == 0:
            continue
        for i in range(5):
            rows = slice(r0 + 16 * i, min(r0 + 16 * i + 16, M_BANDED))
            if rows.start >= M_BANDED or (band % 2 == 1 and i == 2):
                continue
            # strictly inside the first and the last tile of the range (the ragged tile 12 has columns 384 .. 389)
            c0 = 32 * t0 + 1 + 3 * i
            last = t0 + n - 1
            c1 = 32 * last + (30 - 3 * i if last < 12 else 4 - i % 4)
            assert 32 * t0 < c0 <= c1 < min(32 * last + 31, K_BANDED - 1)
            A[rows, c0:c1 + 1] = rng.normal(size=(rows.stop - rows.start, c1 + 1 - c0))
            A[rows.start, c0] = A[rows.start, c1] = 1.0        # the ends of the extent are nonzeros, whatever was drawn
    return A, nk


def _banded(N):
    A, _ = banded_operand()
    return A, np.random.default_rng(N).normal(size=(K_BANDED, N))


def _upper(M, N, K):
    rng = np.random.default_rng(M + N + K)
    return np.triu(rng.normal(size=(M, K))), rng.normal(size=(K, N))


# name -> (operands, whether the plan is the whole-band one)
CASES = {
    "banded_whole_band_1090_3840_390": (lambda: _banded(3840), True),
    "banded_streamed_1090_77_390": (lambda: _banded(77), False),
    "streamed_upper_81_129_33": (lambda: _upper(81, 129, 33), False),
    "streamed_upper_333_77_250": (lambda: _upper(333, 77, 250), False),
}


def digests(name):
    """{"inputs": .., "form_8wave": .., "form_feed": ..} of a case through the library that is loaded"""
    A, B = CASES[name][0]()
    out = {"inputs": sha256(A, B)}
    for key, form in FORMS:
        out[key] = sha256(_band_form(A, B, form)[0])
    return out


def sampler_run():
    """{"u": SHA-256, "accept_rate": .., "leapfrog_total": ..} of the sampler case through the library that is loaded"""
    d = synth.geospatial(640, seed=1)
    with api.Context(d["cov"], d["data"], d["eff_range"], d["Z"], d["X"], d["y"], d["family"], d["link"]) as ctx:
        ctx.update_L(d["theta"])
        # one draw per chain behind 3 warm-up proposals; lambda / e is far above max_steps = 10 for any step size
        diag = ctx.hmc_sample(d["beta"], d["sigma"], 3, 1024, 100.0, 10, 0.9, seed=17, chains=1024)
        assert ctx.profile(enable=False)["operator"] == "banded"
        assert ctx.last_kernels() == ("band", "band")
        u = ctx.get_u()
    assert np.isfinite(u).all() and diag["leapfrog_total"] > 0
    return {"u": sha256(u), "accept_rate": float(diag["accept_rate"]), "leapfrog_total": int(diag["leapfrog_total"])}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_banded_operand_has_the_items_it_is_built_for():
    A, nk = banded_operand()
    assert len(nk) == 14 and nk == [LEN[b % 7] for b in range(14)] and M_BANDED - 13 * 80 == 50
    for band, r0 in enumerate(range(0, M_BANDED, 80)):
        cols = np.flatnonzero(np.any(A[r0:r0 + 80] != 0.0, axis=0))
        assert (0 if cols.size == 0 else cols[-1] // 32 - cols[0] // 32 + 1) == nk[band]
        for i in range(5):
            c = np.flatnonzero(np.any(A[r0 + 16 * i:min(r0 + 16 * i + 16, M_BANDED)] != 0.0, axis=0))
            if c.size:      # first and last nonzero column strictly inside a K tile
                assert c[0] % 32 != 0 and c[-1] % 32 != 31 and c[-1] != K_BANDED - 1
    assert A[:, 384:].any()         # the ragged tile is reached


@pytest.mark.parametrize("name", list(CASES))
def test_output_bits_are_the_recorded_ones(name, recorded):
    want = recorded["cases"][name]
    make, whole_band = CASES[name]
    A, B = make()
    assert sha256(A, B) == want["inputs"], "the seeded operands are not the recorded ones (numpy stream changed?)"
    K = A.shape[1]
    u = 2.0 ** -53
    bound = K * u / (1.0 - K * u) * (np.abs(A) @ np.abs(B))
    ref = A @ B
    for key, form in FORMS:
        got, _, whole = _band_form(A, B, form)
        assert whole == int(whole_band), "%s: plan is %s" % (name, "whole-band" if whole else "streamed")
        err = np.abs(got - ref)
        print(name, key, sha256(got), "max |C - AB| / (gamma_K |A||B|) = %.3g" % np.max(err / (bound + 1e-300)))
        assert np.all(err <= bound)
        assert sha256(got) == want[key], "%s: %s differs from the bits recorded in %s" % (name, key, FIXTURE)


def test_sampler_bits_are_the_recorded_ones(recorded):
    got = sampler_run()
    print(got)
    assert got == recorded["sampler"]
