"""Generates tests/golden/bobyqa_traces.json: SHA-256 of the optimiser's trajectory -- every evaluated point in order, the
result, fval, nfev -- on the cases of tests/test_bobyqa_traces_cpu.py.  Host code only: no GPU is needed.

The fixture pins the bits of a REFERENCE build, so run it with GLMMR_MCML_LIB pointing at the library built from the
commit to pin to -- the parent of a change to csrc/optim.hip, never the code under test:

    GLMMR_MCML_LIB=/path/to/parent/libglmmr_mcml_hip.so python tests/golden/make_bobyqa_traces.py "<commit it was built from>"
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import test_bobyqa_traces_cpu as bt       # noqa: E402


def main():
    assert os.environ.get("GLMMR_MCML_LIB"), "point GLMMR_MCML_LIB at the reference build (see the docstring)"
    out = {"recorded_from": sys.argv[1],
           "hash": "SHA-256 of the points, the result and fval as little-endian float64, then nfev as int32",
           "cases": {name: bt.trace(name) for name in bt.CASES}}
    with open(os.path.join(HERE, "bobyqa_traces.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
