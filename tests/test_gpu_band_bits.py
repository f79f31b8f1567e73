"""The bits of the banded HMC product kernel (csrc/dgemm_band.h), pinned.  test_gpu_band_feed.py compares the kernel's
two forms with each other, which cannot see a change that moves both together (they are two instantiations of one
pipeline); here the SHA-256 of each form's output on three seeded operands is compared with tests/golden/band_bits.json,
recorded from the library of the commit named there (tests/golden/make_band_bits.py: never from the code under test).

Operands: test_gpu_band_feed's streamed shapes (81, 129, 33) -- one tile with one row / column / K column over -- and
(333, 77, 250) -- runs cut inside bands, raw accumulator tiles through k_band_reduce --, and its lower-triangular
1690 x 1690 x 2400 whole-band operand (last band of 10 rows, last column tile of 96 columns, groups of one or two bands).
The input hashes are asserted first: a changed numpy stream fails there instead of comparing different problems."""
import hashlib
import json
import os

import numpy as np
import pytest

from test_gpu_band_feed import FORM_8WAVE, FORM_FEED, _band_form

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "band_bits.json")
FORMS = (("form_8wave", FORM_8WAVE), ("form_feed", FORM_FEED))


def _streamed(M, N, K):
    rng = np.random.default_rng(M + N + K)
    return np.tril(rng.normal(size=(M, K))), rng.normal(size=(K, N))


def _whole_band():
    rng = np.random.default_rng(1690)
    A, B = rng.normal(size=(1690, 1690)), rng.normal(size=(1690, 2400))
    return np.tril(A), B


CASES = {
    "streamed_81_129_33": lambda: _streamed(81, 129, 33),
    "streamed_333_77_250": lambda: _streamed(333, 77, 250),
    "whole_band_lower_1690_2400": _whole_band,
}


def sha256(*arrays):
    """of the arrays' float64 values in column-major order, one after the other"""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.asarray(a, dtype=np.float64).tobytes(order="F"))
    return h.hexdigest()


def digests(name):
    """{"inputs": .., "form_8wave": .., "form_feed": ..} of a case through the library that is loaded"""
    A, B = CASES[name]()
    out = {"inputs": sha256(A, B)}
    for key, form in FORMS:
        out[key] = sha256(_band_form(A, B, form)[0])
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_output_bits_are_the_recorded_ones(name):
    with open(FIXTURE) as f:
        want = json.load(f)["cases"][name]
    A, B = CASES[name]()
    assert sha256(A, B) == want["inputs"], "the seeded operands are not the recorded ones (numpy stream changed?)"
    for key, form in FORMS:
        got = sha256(_band_form(A, B, form)[0])
        print(name, key, got)
        assert got == want[key], "%s: %s differs from the bits recorded in %s" % (name, key, FIXTURE)
