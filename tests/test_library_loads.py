"""CPU-side check that the C-ABI library loads and exports every symbol that
include/glmmr_mcml_c.h declares (no compute without a GPU)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "glmmr_mcml_c.h")).read()
    return sorted(set(re.findall(r"\b(glmmr_mcml_\w+)\s*\(", hdr)))


def test_exports_every_declared_symbol():
    from glmmrmcml_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = _lib.lib()
    syms = _declared_symbols()
    assert len(syms) >= 3
    missing = [s for s in syms if not hasattr(L, s)]
    assert not missing, missing


def _declarations():
    """{name: number of parameters} of every function the header declares, by a parser of the test's own"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "glmmr_mcml_c.h")).read(), flags=re.S)
    found = re.findall(r"^(?:const char\*|long long|int)\s+(glmmr_mcml_\w+)\(([^()]*)\);", hdr, flags=re.M)
    return {name: 0 if params.strip() == "void" else params.count(",") + 1 for name, params in found}


def test_every_declared_function_has_its_prototype():
    """_lib.lib() reads restype / argtypes of every function from the header: a 64-bit scalar or return that no call site
    wraps is then still passed whole.  The expected lists below are written out from the header by hand"""
    import ctypes as C
    from glmmrmcml_amd import _lib
    L = _lib.lib()
    decl = _declarations()
    assert sorted(decl) == _declared_symbols() and len(decl) == 95
    for name, nparams in decl.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nparams, (name, fn.argtypes, nparams)
    vp, i, d, ll, u64, u32 = C.c_void_p, C.c_int, C.c_double, C.c_longlong, C.c_uint64, C.c_uint32
    want = {
        "glmmr_mcml_ctx_hmc_sample": (i, [vp, vp, d, vp, u64, u32, vp, vp, vp, vp, vp, vp]),
        "glmmr_mcml_ctx_full": (i, [vp, vp, i, i, i, i, i, d, i, d, i, i, i, d, vp, vp, vp, vp, vp, vp, vp]),
        "glmmr_mcml_dbg_normals": (i, [u64, u32, u32, u32, i, vp]),
        "glmmr_mcml_dbg_copy_roundtrip": (i, [vp, ll, vp, ll, ll, ll]),
        "glmmr_mcml_dbg_dgemm_at": (i, [i, i, i, vp, i, vp, i, d, d, vp, i, i]),
        "glmmr_mcml_set_default_trajectory": (i, [i]),
        "glmmr_mcml_dbg_traj_launches": (ll, []),
        "glmmr_mcml_last_error": (C.c_char_p, []),
        "glmmr_mcml_dbg_bobyqa": (i, [vp, vp, i, vp, vp, vp, d, d, i, vp, vp, vp]),       # a callback typedef crosses as void*
    }
    for name, (restype, argtypes) in want.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, (name, fn.restype, fn.argtypes)


def test_a_type_the_loader_does_not_know_is_refused():
    from glmmrmcml_amd import _lib
    for bad in ("int glmmr_mcml_x(float v);", "float glmmr_mcml_x(int v);"):
        with pytest.raises(ImportError, match="glmmr_mcml_x"):
            _lib.prototypes("typedef struct s s;\n" + bad)


# the three opt-in modes: (entry points' suffix, environment variable, names in the order of their codes); mode 0 first
MODES = [("trajectory", "GLMMR_MCML_TRAJ", ("step", "component")),
         ("draws", "GLMMR_MCML_DRAWS", ("hmc", "exact", "exact_component")),
         ("la_operator", "GLMMR_MCML_LA", ("dense", "component", "component_wide"))]
ENV_CASES = [(kind, env, value, value if value in names else names[0])
             for kind, env, names in MODES for value in (None,) + names + ("no-such-mode",)]


@pytest.mark.parametrize("kind,env,value,want", ENV_CASES, ids=["%s=%s" % (c[1], c[2]) for c in ENV_CASES])
def test_mode_default_from_the_environment(kind, env, value, want):
    """the variable is read once per process, so every case has a fresh interpreter: the named mode, or mode 0 for no
    value and for one that names no mode.  Host-only entry points: no GPU is needed"""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from glmmrmcml_amd import api\n"
            "print(api.get_default_%s())\n" % (ROOT, kind))
    envp = {k: v for k, v in os.environ.items() if k != env}
    if value is not None:
        envp[env] = value
    r = subprocess.run([sys.executable, "-c", code], check=True, env=envp, capture_output=True, text=True, timeout=120)
    assert r.stdout.strip().splitlines()[-1] == want, (r.stdout, r.stderr)


@pytest.mark.parametrize("kind,env,names", MODES, ids=[m[0] for m in MODES])
def test_mode_default_round_trip_and_refusals(kind, env, names):
    from glmmrmcml_amd import _lib, api
    L = _lib.lib()
    get, put = getattr(api, "get_default_" + kind), getattr(api, "set_default_" + kind)
    before = get()
    try:
        for code, name in enumerate(names):
            put(name)
            assert get() == name and getattr(L, "glmmr_mcml_get_default_" + kind)() == code
        held = get()
        for code in (-1, len(names)):
            rc = getattr(L, "glmmr_mcml_set_default_" + kind)(code)
            assert rc != 0 and get() == held
            msg = L.glmmr_mcml_last_error().decode()
            assert "set_default_" + kind in msg and all("%d (" % c in msg and n in msg for c, n in enumerate(names)), msg
        assert getattr(L, "glmmr_mcml_ctx_set_" + kind)(None, 0) != 0 and L.glmmr_mcml_last_error()       # no context
        with pytest.raises(KeyError):
            put("no-such-mode")
        assert get() == held
    finally:
        put(before)
    assert get() == before


def test_compute_without_gpu_fails_loudly():
    import ctypes as C
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from glmmrmcml_amd import _lib
    L = _lib.lib()
    ms = C.c_double()
    rc = L.glmmr_mcml_dbg_dgemm_bench(64, 64, 64, 0, 1, -1, C.byref(ms))
    assert rc != 0
    with pytest.raises(_lib.McmlError):
        _lib.check(rc)


def test_phase_clock_is_host_only():
    """glmmr_mcml_dbg_phase_ms touches no device: enable / read / reset work on a host without a GPU and start at zero"""
    from glmmrmcml_amd import api
    api.phase_ms(enable=True, reset=True)
    got = api.phase_ms(enable=False)
    assert set(got) == {"sample", "beta_step", "theta_step", "refresh"} and all(v == 0.0 for v in got.values())
