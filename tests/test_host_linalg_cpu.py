"""The small host solves of csrc/host_linalg.h -- gj_inverse (the beta-step's and the optimiser's Gauss-Jordan inverse),
ge_solve (mcnr_b's elimination) and spd_inverse (the Laplace Hessian's Cholesky inverse) -- compiled as plain C++ into
tests/host_linalg_driver.cpp under AddressSanitizer + UBSan and compared with numpy to 1e-12 relative (the matrices are
well conditioned, kappa_2 < 20: numpy's own error is below 1e-14).  What gj_inverse refuses: an exactly singular matrix at
either tolerance the library passes (0: the beta-step, 1e-14: the optimiser), and at 1e-14 alone a matrix whose best pivot
is 1e-15 of its largest entry.  What the matrices are is asserted with numpy before the driver sees them."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 5)
RTOL = 1e-12


def swap_matrix(N):
    """the rows of a diagonally dominant matrix in reverse order: every column's largest entry lies off the diagonal (N > 1)"""
    rng = np.random.default_rng(100 + N)
    A = (rng.uniform(-1, 1, size=(N, N)) + 2.0 * N * np.eye(N))[::-1].copy()
    assert N == 1 or abs(A[0, 0]) < np.abs(A[1:, 0]).max()
    return A


def plain_matrix(N):
    rng = np.random.default_rng(200 + N)
    return rng.uniform(-1, 1, size=(N, N)) + N * np.eye(N)


def spd_matrix(N):
    B = np.random.default_rng(300 + N).standard_normal((N, N))
    return B @ B.T / N + np.eye(N)


def singular_matrix(N):
    """exactly singular in floating point too: a zero column stays zero under row operations"""
    A = plain_matrix(N)
    A[:, N // 2] = 0.0
    return A


def tiny_pivot_matrix(N):
    """(diagonal matrix with one entry of 1e-15 among ones, whether 1e-14 refuses it): no rounding on the way to that
    pivot.  N = 1: the entry is itself the largest, so it is accepted at both tolerances"""
    d = np.ones(N)
    d[N // 2] = 1e-15
    return np.diag(d), N > 1


def _fmt(*arrays):
    return " ".join("%.17g" % x for a in arrays for x in np.asarray(a, dtype=np.float64).ravel(order="F"))


def _cases():
    """name -> (line for the driver, expected: None = refused, else the array)"""
    out = {}
    for N in SIZES:
        for kind, A in (("swap", swap_matrix(N)), ("plain", plain_matrix(N))):
            assert np.linalg.cond(A) < 20, (kind, N, np.linalg.cond(A))
            for tol in (0.0, 1e-14):
                out["gj_%s_%d_tol%g" % (kind, N, tol)] = ("gj %d %.17g %s" % (N, tol, _fmt(A)), np.linalg.inv(A))
            b = np.random.default_rng(400 + N).standard_normal(N)
            out["ge_%s_%d" % (kind, N)] = ("ge %d %s" % (N, _fmt(A, b)), np.linalg.solve(A, b))
        H = spd_matrix(N)
        assert np.linalg.cond(H) < 20 and np.all(np.linalg.eigvalsh(H) > 0)
        out["spd_%d" % N] = ("spd %d %s" % (N, _fmt(H)), np.linalg.inv(H))
        S = singular_matrix(N)
        assert np.linalg.matrix_rank(S) == N - 1 and np.linalg.det(S) == 0.0
        for tol in (0.0, 1e-14):
            out["gj_singular_%d_tol%g" % (N, tol)] = ("gj %d %.17g %s" % (N, tol, _fmt(S)), None)
        out["ge_singular_%d" % N] = ("ge %d %s" % (N, _fmt(S, np.ones(N))), None)
        T, refused = tiny_pivot_matrix(N)
        assert np.abs(T).min(where=T != 0, initial=np.inf) == 1e-15 and (np.abs(T).max() == 1.0) == refused
        out["gj_tiny_%d_tol0" % N] = ("gj %d 0 %s" % (N, _fmt(T)), np.linalg.inv(T))
        out["gj_tiny_%d_tol1e-14" % N] = ("gj %d 1e-14 %s" % (N, _fmt(T)), None if refused else np.linalg.inv(T))
    out["spd_indefinite_2"] = ("spd 2 %s" % _fmt(np.array([[1.0, 2.0], [2.0, 1.0]])), None)
    out["spd_semidefinite_2"] = ("spd 2 %s" % _fmt(np.array([[1.0, 1.0], [1.0, 1.0]])), None)
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_host_solves_under_asan_ubsan_against_numpy(tmp_path):
    csrc = os.path.join(ROOT, "glmmrmcml_amd", "csrc")
    exe = str(tmp_path / "host_linalg_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + csrc, os.path.join(ROOT, "tests", "host_linalg_driver.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    cases = _cases()
    path = tmp_path / "cases.txt"
    path.write_text("".join("%s %s\n" % (name, line) for name, (line, _) in cases.items()))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    got = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if len(w) >= 2 and w[0] in cases:
            got[w[0]] = None if w[1] == "refused" else np.array([float(x) for x in w[2:]])
    assert "cases=%d" % len(cases) in r.stdout and set(got) == set(cases)
    for name, (_, want) in cases.items():
        if want is None:
            assert got[name] is None, (name, "was not refused")
            continue
        assert got[name] is not None, (name, "was refused")
        g = got[name].reshape(want.shape, order="F")
        err = np.abs(g - want).max() / np.abs(want).max()
        print(name, err)
        assert err <= RTOL, (name, err)
