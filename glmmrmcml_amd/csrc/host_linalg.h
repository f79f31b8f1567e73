// host_linalg.h -- the small dense solves the host does (N = a handful of fixed effects or optimiser variables): plain
// C++, column-major N x N in a std::vector, no device code.  Each returns false where the matrix is refused; the caller
// words the error.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace mcml {

// in-place inverse by Gauss-Jordan with partial pivoting; false (A left half-eliminated) if a column's best pivot is not
// above rel_tol * max|A|: rel_tol = 0 refuses exact zeros and NaN only
inline bool gj_inverse(std::vector<double>& A, int N, double rel_tol)
{
    std::vector<double> B((size_t)N * N, 0.0);
    for (int i = 0; i < N; ++i) B[i + (size_t)i * N] = 1.0;
    double amax = 0;
    for (double v : A) amax = std::max(amax, std::fabs(v));
    for (int c = 0; c < N; ++c) {
        int p = c; double best = std::fabs(A[c + (size_t)c * N]);
        for (int i = c + 1; i < N; ++i) if (std::fabs(A[i + (size_t)c * N]) > best) { best = std::fabs(A[i + (size_t)c * N]); p = i; }
        if (!(best > rel_tol * amax)) return false;
        if (p != c) for (int j = 0; j < N; ++j) { std::swap(A[c + (size_t)j * N], A[p + (size_t)j * N]); std::swap(B[c + (size_t)j * N], B[p + (size_t)j * N]); }
        double d = A[c + (size_t)c * N];
        for (int j = 0; j < N; ++j) { A[c + (size_t)j * N] /= d; B[c + (size_t)j * N] /= d; }
        for (int i = 0; i < N; ++i) if (i != c) {
            double f = A[i + (size_t)c * N];
            if (f != 0.0) for (int j = 0; j < N; ++j) { A[i + (size_t)j * N] -= f * A[c + (size_t)j * N]; B[i + (size_t)j * N] -= f * B[c + (size_t)j * N]; }
        }
    }
    A.swap(B);
    return true;
}

// b <- A^-1 b by Gaussian elimination with partial pivoting (A is overwritten); false if a pivot is exactly zero
inline bool ge_solve(std::vector<double>& A, std::vector<double>& b, int P)
{
    for (int k = 0; k < P; ++k) {
        int piv = k;
        for (int i = k + 1; i < P; ++i) if (fabs(A[i + (size_t)k * P]) > fabs(A[piv + (size_t)k * P])) piv = i;
        if (A[piv + (size_t)k * P] == 0.0) return false;
        if (piv != k) { for (int j = 0; j < P; ++j) std::swap(A[k + (size_t)j * P], A[piv + (size_t)j * P]); std::swap(b[k], b[piv]); }
        for (int i = k + 1; i < P; ++i) {
            const double f = A[i + (size_t)k * P] / A[k + (size_t)k * P];
            for (int j = k; j < P; ++j) A[i + (size_t)j * P] -= f * A[k + (size_t)j * P];
            b[i] -= f * b[k];
        }
    }
    for (int k = P - 1; k >= 0; --k) {
        double s = b[k];
        for (int j = k + 1; j < P; ++j) s -= A[k + (size_t)j * P] * b[j];
        b[k] = s / A[k + (size_t)k * P];
    }
    return true;
}

// out = H^-1 through the Cholesky factor of H (lower triangle read), column by column; false if H is not positive definite
inline bool spd_inverse(const std::vector<double>& H, int nv, std::vector<double>* out)
{
    std::vector<double> L(H);
    for (int j = 0; j < nv; ++j) {
        double d = L[j + (size_t)j * nv];
        for (int k = 0; k < j; ++k) d -= L[j + (size_t)k * nv] * L[j + (size_t)k * nv];
        if (!(d > 0.0)) return false;
        d = sqrt(d);
        L[j + (size_t)j * nv] = d;
        for (int i = j + 1; i < nv; ++i) {
            double s = L[i + (size_t)j * nv];
            for (int k = 0; k < j; ++k) s -= L[i + (size_t)k * nv] * L[j + (size_t)k * nv];
            L[i + (size_t)j * nv] = s / d;
        }
    }
    out->assign((size_t)nv * nv, 0.0);
    for (int col = 0; col < nv; ++col) {
        std::vector<double> x(nv, 0.0);
        x[col] = 1.0;
        for (int i = 0; i < nv; ++i) {
            double s = x[i];
            for (int k = 0; k < i; ++k) s -= L[i + (size_t)k * nv] * x[k];
            x[i] = s / L[i + (size_t)i * nv];
        }
        for (int i = nv - 1; i >= 0; --i) {
            double s = x[i];
            for (int k = i + 1; k < nv; ++k) s -= L[k + (size_t)i * nv] * x[k];
            x[i] = s / L[i + (size_t)i * nv];
        }
        for (int i = 0; i < nv; ++i) (*out)[i + (size_t)col * nv] = x[i];
    }
    return true;
}

}  // namespace mcml
