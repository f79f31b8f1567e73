"""Generates tests/golden/cov_bits.json: SHA-256 of what gen_D, mvn_ll_grad, predict_re and theta_information return on the
cases of tests/test_gpu_cov_bits.py, and of the cases' seeded inputs.

The fixture pins the bits of a REFERENCE build, so run it on the GPU with GLMMR_MCML_LIB pointing at the library built
from the commit to pin to -- the parent of a change to the covariance entries, the small-block factorisation in LDS or the
walk over a block's lower triangle, never the code under test:

    GLMMR_MCML_LIB=/path/to/parent/libglmmr_mcml_hip.so python tests/golden/make_cov_bits.py "<commit it was built from>"

The reference library's figures on TEN_SLOTS against the long-double reference (test_ten_slots_against_the_reference) are
printed first: were it outside the bound, its digests would pin a bug.
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import test_gpu_cov_bits as cb       # noqa: E402


def main():
    assert os.environ.get("GLMMR_MCML_LIB"), "point GLMMR_MCML_LIB at the reference build (see the docstring)"
    for m, weighted, ratio, rel, same in cb.ten_slots_ratios():
        print("TEN_SLOTS m=%d %s: largest |grad - ref| / bound = %.3g, value rel %.2e, repeat identical %s" % (
            m, "weighted" if weighted else "unweighted", ratio, rel, same))
        if not (ratio <= 1.0 and rel <= cb.RTOL and same):
            print("THE REFERENCE BUILD MISSES THE BOUND ON TEN_SLOTS: do not pin its TEN_SLOTS digests")
    cases = {}
    for name in cb.CASES:
        with pytest.MonkeyPatch.context() as mp:
            cases[name] = cb.digests(name, mp)
    out = {"recorded_from": sys.argv[1],
           "hash": "SHA-256 of the values as float64 in column-major order, one array after the other",
           "cases": cases}
    with open(os.path.join(HERE, "cov_bits.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
