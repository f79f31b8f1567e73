"""include/glmmr_mcml_small_sample.h, the header of the small-sample query that include/glmmr_mcml_c.h includes: the library
exports what it declares and the loader (glmmrmcml_amd/_lib.py) gives each function the prototype the header states.  No GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "include", "glmmr_mcml_c.h")
SS = os.path.join(ROOT, "include", "glmmr_mcml_small_sample.h")
OTHERS = ("glmmr_mcml_info.h", "glmmr_mcml_predict.h", "glmmr_mcml_sandwich.h", "glmmr_mcml_band.h", "glmmr_mcml_theta_info.h")


def _declarations(path):
    """{name: number of parameters}, by a parser of the test's own"""
    hdr = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    found = re.findall(r"^(?:const char\*|long long|int)\s+(glmmr_mcml_\w+)\(([^()]*)\);", hdr, flags=re.M)
    return {name: 0 if params.strip() == "void" else params.count(",") + 1 for name, params in found}


def test_the_main_header_includes_it_inside_its_extern_c_block_after_theta_info():
    text = open(MAIN).read()
    at = text.index('#include "glmmr_mcml_small_sample.h"')
    assert text.index('extern "C" {') < at < text.rindex("#ifdef __cplusplus")
    assert text.index('#include "glmmr_mcml_theta_info.h"') < at
    own = open(SS).read()
    assert "GLMMR_MCML_C_H" in own and "#error" in own                   # refuses to be included on its own


def test_declared_exported_and_prototyped():
    from glmmrmcml_amd import _lib
    decl = _declarations(SS)
    assert decl == {"glmmr_mcml_ctx_small_sample": 13, "glmmr_mcml_small_sample": 14, "glmmr_mcml_dbg_small_sample_plan": 2}
    assert not set(decl) & set(_declarations(MAIN))                    # declared once
    for other in OTHERS:
        assert not set(decl) & set(_declarations(os.path.join(ROOT, "include", other)))
    assert set(decl) <= set(_lib.prototypes(_lib.header_text()))
    assert "glmmr_mcml_small_sample.h" in _lib.__doc__
    L = _lib.lib()
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    want = {"glmmr_mcml_ctx_small_sample": [vp, vp, d, vp, i, vp, i, vp, i, vp, vp, vp, vp],
            "glmmr_mcml_small_sample": [vp, vp, vp, i, d, i, vp, i, vp, i, vp, vp, vp, vp],
            "glmmr_mcml_dbg_small_sample_plan": [vp, vp]}
    for name, argtypes in want.items():
        fn = getattr(L, name)
        assert fn.restype is i and list(fn.argtypes) == argtypes, (name, fn.restype, fn.argtypes)


def test_null_arguments_are_refused_without_a_device():
    from glmmrmcml_amd import _lib
    L = _lib.lib()
    out = (C.c_longlong * 8)()
    assert L.glmmr_mcml_dbg_small_sample_plan(None, out) == -1
    assert L.glmmr_mcml_ctx_small_sample(None, None, 1.0, None, 0, None, 1, None, 1, None, None, None, None) == -1
    assert b"small_sample" in L.glmmr_mcml_last_error()
    assert L.glmmr_mcml_small_sample(None, None, None, 0, 1.0, 0, None, 1, None, 1, None, None, None, None) == -1
    assert b"small_sample" in L.glmmr_mcml_last_error()
