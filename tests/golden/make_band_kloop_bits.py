"""Generates tests/golden/band_kloop_bits.json: SHA-256 of the banded product kernel's outputs (both forms) on the
seeded operands of tests/test_gpu_band_kloop.py, and the sampler case's state digest and diagnostics.

The fixture pins the bits of a REFERENCE build, so run it on the GPU with GLMMR_MCML_LIB pointing at the library built
from the commit to pin to -- the parent of a change to csrc/dgemm_band.h, never the code under test:

    GLMMR_MCML_LIB=/path/to/parent/libglmmr_mcml_hip.so python tests/golden/make_band_kloop_bits.py "<commit it was built from>"
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import test_gpu_band_kloop as kl          # noqa: E402


def main():
    assert os.environ.get("GLMMR_MCML_LIB"), "point GLMMR_MCML_LIB at the reference build (see the docstring)"
    out = {"recorded_from": sys.argv[1], "hash": "SHA-256 of the float64 values in column-major order; inputs: A then B",
           "cases": {name: kl.digests(name) for name in kl.CASES}, "sampler": kl.sampler_run()}
    with open(os.path.join(HERE, "band_kloop_bits.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
