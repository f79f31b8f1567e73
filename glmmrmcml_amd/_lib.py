"""Loads the in-tree HIP library and gives every function of include/glmmr_mcml_c.h (and of the headers of the same
directory it includes: glmmr_mcml_info.h, glmmr_mcml_predict.h, glmmr_mcml_sandwich.h, glmmr_mcml_band.h,
glmmr_mcml_theta_info.h, glmmr_mcml_small_sample.h) its prototype.  There is no CPU
fallback: if the library (or the header the prototypes are read from) is missing, or no MI355X is visible when a compute
entry point is called, the call fails loudly."""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# GLMMR_MCML_LIB: developer override for A/B timing of two builds of the same library
LIB_PATH = os.environ.get("GLMMR_MCML_LIB") or os.path.join(_HERE, "libglmmr_mcml_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "glmmr_mcml_c.h")
_lib = None


class McmlError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("glmmr_mcml error %d: %s" % (code, msg))
        self.code = code


# The header is regular: a return type, the name, a parameter list without parentheses.  Scalars cross as their exact C type;
# every pointer, and the three callback typedefs, as c_void_p -- which takes byref(), arrays, ndarray.ctypes.data_as(),
# bytes, None and CFUNCTYPE instances alike, so a call site names no pointer type.
_RETURNS = {"int": C.c_int, "long long": C.c_longlong, "const char*": C.c_char_p}
_SCALARS = {"int": C.c_int, "double": C.c_double, "long long": C.c_longlong, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32}
_CALLBACKS = ("glmmr_mcml_objective", "glmmr_mcml_batch_objective", "glmmr_mcml_parts_objective")
_DECL = re.compile(r"(?<=[;{}]) ?([\w ]+?\*?) ?\b(glmmr_mcml_\w+) ?\(([^()]*)\) ?;")
_INCLUDE = re.compile(r'^\s*#\s*include\s+"(glmmr_mcml_\w+\.h)"', re.M)


def header_text():
    """the public header followed by the text of each header of its directory it includes (one level: they include none)"""
    with open(HEADER_PATH) as f:
        text = f.read()
    for name in _INCLUDE.findall(text):
        with open(os.path.join(os.path.dirname(HEADER_PATH), name)) as f:
            text += "\n" + f.read()
    return text


def prototypes(header):
    """{name: (restype, [argtypes])} of every function the text of the public header declares"""
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)                      # comments,
    text = " ".join(re.sub(r"^\s*#.*$", "", text, flags=re.M).split())       # preprocessor lines, line structure
    out = {}
    for ret, name, params in _DECL.findall(text):
        if ret not in _RETURNS:
            raise ImportError("%s: no ctypes type for the return type '%s' of %s" % (HEADER_PATH, ret, name))
        args = []
        for p in (q.strip() for q in params.split(",")):
            kind = p.rpartition(" ")[0]                       # without the parameter's name
            if "*" in p or kind in _CALLBACKS:
                args.append(C.c_void_p)
            elif kind in _SCALARS:
                args.append(_SCALARS[kind])
            elif p != "void":
                raise ImportError("%s: no ctypes type for parameter '%s' of %s" % (HEADER_PATH, p, name))
        out[name] = (_RETURNS[ret], args)
    return out


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950); glmmrmcml_amd has no CPU fallback" % LIB_PATH)
        if not os.path.exists(HEADER_PATH):
            raise ImportError("%s is missing: the prototypes of %s are read from it" % (HEADER_PATH, LIB_PATH))
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in prototypes(header_text()).items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise McmlError(rc, lib().glmmr_mcml_last_error().decode(errors="replace"))
