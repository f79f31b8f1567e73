"""Generates tests/golden/query_bits.json: SHA-256 of what the information query, the sandwich and the component-wise exact
draws return on the cases of tests/test_gpu_query_bits.py, and of the cases' seeded inputs.

The fixture pins the bits of a REFERENCE build, so run it on the GPU with GLMMR_MCML_LIB pointing at the library built
from the commit to pin to -- the parent of a change to the component solves, the Gram reduction, the queries' tail or the
factor scratch, never the code under test:

    GLMMR_MCML_LIB=/path/to/parent/libglmmr_mcml_hip.so python tests/golden/make_query_bits.py "<commit it was built from>"
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import test_gpu_query_bits as qb       # noqa: E402


def main():
    assert os.environ.get("GLMMR_MCML_LIB"), "point GLMMR_MCML_LIB at the reference build (see the docstring)"
    cases = {}
    for name in qb.CASES:
        with pytest.MonkeyPatch.context() as mp:
            cases[name] = qb.digests(name, mp)
    out = {"recorded_from": sys.argv[1],
           "hash": "SHA-256 of the values as float64 in column-major order, one array after the other",
           "cases": cases}
    with open(os.path.join(HERE, "query_bits.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
