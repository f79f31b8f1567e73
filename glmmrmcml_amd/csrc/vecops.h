// vecops.h -- the vector-sized streaming kernels several modules share (vecops.hip), each behind a host launcher on
// c.stream that returns the launch's error.  Reductions are two-stage with a fixed order: bit-reproducible.
#pragma once
#include "ctx.h"

namespace mcml {

// out[0] = (accumulate ? out[0] : 0) + sum(x[0 .. n)), one workgroup
int dev_sum(Ctx& c, const double* x, int n, double* out, bool accumulate = false);
// partials[by * gx + bx] = sum of squares of rows [256 bx, 256 bx + 256) over columns by, by + gy, ... of A (rows x cols);
// gx >= ceil(rows / 256) or the rows beyond are left out
int dev_sumsq_partials(Ctx& c, const double* A, int lda, int rows, int cols, int gx, int gy, double* partials);
// out[0] = sum_i 2 log A_ii: the log-determinant of L L' from its factor (mcmldmatrix.h:67-70)
int dev_logdet_chol(Ctx& c, const double* A, int lda, int n, double* out);
// y = A x (A rows x cols, column-major): one thread per row
int dev_gemv_n(Ctx& c, const double* A, int lda, int rows, int cols, const double* x, double* y);
// y[j] = beta y[j] + alpha sum_i A[i + j lda] x[i]  (A' x): one wave per column; beta == 0 does not read y
int dev_gemv_t(Ctx& c, const double* A, int lda, int rows, int cols, const double* x, double* y, double alpha, double beta);
int dev_axpy(Ctx& c, double* y, const double* x, double a, int n);     // y += a x
int dev_copy(Ctx& c, double* dst, const double* src, int n);
// AT (cols x rows) = A' through a 32 x 33 LDS tile; nbatch > 1: the same A into AT + z * bsT, z < nbatch
int dev_transpose(Ctx& c, const double* A, int lda, int rows, int cols, double* AT, int ldt, int nbatch = 1, size_t bsT = 0);

}  // namespace mcml
