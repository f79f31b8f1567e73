"""Candidates of a theta-step that differ in a pure scale parameter share one factorisation (csrc/theta_scale.h).
Host logic only: a stand-alone driver under AddressSanitizer + UBSan checks the exponents proved from a covariance
specification and the grouping (tests/host_theta_scale_driver.cpp); the library's own batch optimiser, driven through
its C ABI on the numpy MVN objective of test_optim_cpu.py, shows what the grouping saves under the benchmark's budget."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_optim_cpu import _mvn_objective

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int)
PARTS = C.CFUNCTYPE(C.c_int, dp, C.c_int, C.c_int, dp, dp, ip, C.c_void_p)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_theta_scale_under_asan_ubsan(tmp_path):
    csrc = os.path.join(ROOT, "glmmrmcml_amd", "csrc")
    exe = str(tmp_path / "host_theta_scale_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + csrc,
           "-I" + os.path.join(ROOT, "include"),
           "-x", "c++", os.path.join(csrc, "common.hip"), "-x", "c++", os.path.join(ROOT, "tests", "host_theta_scale_driver.cpp"),
           "-o", exe, "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "fails=0" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def _mvn_parts(Q, m, seed):
    """the two scalars of test_optim_cpu._mvn_objective (same draws): th -> (logdet D, || inv(L) U ||^2) or None"""
    import scipy.linalg as sla
    rng = np.random.default_rng(seed)
    xy = rng.uniform(size=(Q, 2))
    dist = np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1))
    U = np.linalg.cholesky(0.25 * np.exp(-dist / 0.1)) @ rng.standard_normal((Q, m))

    def parts(th):
        try:
            Lc = np.linalg.cholesky(th[0] * np.exp(-dist / th[1]))
        except np.linalg.LinAlgError:
            return None
        z = sla.solve_triangular(Lc, U, lower=True)
        return 2.0 * np.log(np.diag(Lc)).sum(), float((z * z).sum())
    return parts


def _run(parts, Q, m, start, grouped):
    from glmmrmcml_amd import _lib
    L = _lib.lib()
    rounds = []

    def cb(X, n, k, logdet, sumsq, status, user):
        pts = np.array([[X[j * n + i] for i in range(n)] for j in range(k)])
        rounds.append(pts)
        for j in range(k):
            r = parts(np.exp(pts[j]))
            status[j] = 0 if r is not None else 1
            logdet[j], sumsq[j] = r if r is not None else (0.0, 0.0)
        return 0
    cbk = PARTS(cb)
    z0 = np.log(np.asarray(start, float)); lo = np.full(2, np.log(1e-6)); up = np.full(2, np.inf)
    exps = (C.c_int * 2)(1, 0)
    out = np.zeros(2); f = C.c_double(); nf = C.c_int(); rd = C.c_int(); nfact = C.c_longlong()
    rc = L.glmmr_mcml_dbg_theta_scale_rounds(cbk, None, 2, exps, Q, m, int(grouped), z0.ctypes.data_as(dp),
                                             lo.ctypes.data_as(dp), up.ctypes.data_as(dp), C.c_double(0.25),
                                             C.c_double(1e-7), 40, 8, out.ctypes.data_as(dp), C.byref(f), C.byref(nf),
                                             C.byref(rd), C.byref(nfact))
    _lib.check(rc)
    return out, f.value, nf.value, rd.value, nfact.value, rounds


def test_grouped_rounds_under_the_bench_budget():
    """d_optim_sharded's settings (width 8, budget 40, rhobeg 0.25, over log theta) at Q = 200, m = 64, 3 sample seeds x 2
    starts: the first round is the same set of points with or without the grouping (they do not depend on the values),
    the grouped run factorises at most 34 matrices for its 40 candidates (the optimiser alone reaches 28-32 here), and
    the value reached is the ungrouped run's"""
    Q, m = 200, 64
    for seed in (5, 6, 7):
        parts = _mvn_parts(Q, m, seed)
        f_ref = _mvn_objective(Q=Q, m=m, seed=seed)
        ld, ss = parts(np.array([0.3, 0.12]))
        mine = -(-0.5 * Q * np.log(2 * np.pi) - 0.5 * ld - 0.5 * ss / m)
        assert abs(mine - f_ref(np.array([0.3, 0.12]))) <= 1e-12 * abs(mine)          # the same objective
        for start in ([0.25, 0.1], [0.4, 0.15]):
            zg, fg, nfg, rdg, nfactg, rg = _run(parts, Q, m, start, True)
            zu, fu, nfu, rdu, nfactu, ru = _run(parts, Q, m, start, False)
            print("seed %d start %s: grouped %d factorisations of %d candidates in %d rounds, plain %d of %d; f %.15g vs %.15g"
                  % (seed, start, nfactg, nfg, rdg, nfactu, nfu, fg, fu))
            assert nfactu == nfu <= 40 and nfg <= 40
            # first round: the representatives are, in order, the first point of every distinct range of the plain round
            first, keys = [], set()
            for pt in ru[0]:
                if pt[1].tobytes() not in keys:
                    keys.add(pt[1].tobytes()); first.append(pt)
            assert len(rg[0]) == len(first) < len(ru[0]) and all(a.tobytes() == b.tobytes() for a, b in zip(rg[0], first))
            assert nfactg == sum(len(r) for r in rg) <= 34, nfactg
            assert np.isfinite(fg) and abs(fg - fu) <= 1e-6 * abs(fu)
