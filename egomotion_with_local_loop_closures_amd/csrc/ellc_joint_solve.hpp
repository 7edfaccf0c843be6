// The host solves of the ring's Gauss-Newton calls: one L D L^T routine of size n behind ellc_sim3_solve (n = 7) and ellc_joint_solve
// (n = 6 B <= 48), and the reduced system of an ellc_joint_normal. Plain C++ without HIP: ellc_sim3_impl.hpp and ellc_joint_impl.hpp
// include it, and so does tools/check_joint_solve.cpp, which runs it under the host sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>
#include "../../include/ellc_abi.h"

namespace ellc {

// A x = -b for a symmetric A (row-major n x n, both triangles given) by L D L^T in double, no pivoting. Non-zero, and x unwritten, when a
// pivot is not above 1e-10 times the largest diagonal entry (NaN fails). x may be b.
inline int ldlt_solve_neg(int n, const double* A, const double* b, double* x) {
  std::vector<double> L((size_t)n * n, 0.0), d((size_t)n), y((size_t)n);
  double big = A[0];
  for (int j = 1; j < n; j++) big = std::max(big, A[(size_t)j * n + j]);   // (a NaN on the diagonal fails its own pivot test below)
  const double thr = 1e-10 * big;
  for (int j = 0; j < n; j++) {
    double dj = A[(size_t)j * n + j];
    for (int k = 0; k < j; k++) dj -= L[(size_t)j * n + k] * L[(size_t)j * n + k] * d[k];
    if (!(dj > thr)) return 1;
    d[j] = dj;
    for (int i = j + 1; i < n; i++) {
      double s = A[(size_t)i * n + j];
      for (int k = 0; k < j; k++) s -= L[(size_t)i * n + k] * L[(size_t)j * n + k] * d[k];
      L[(size_t)i * n + j] = s / dj;
    }
  }
  for (int i = 0; i < n; i++) {   // L y = -b
    double s = -b[i];
    for (int k = 0; k < i; k++) s -= L[(size_t)i * n + k] * y[k];
    y[i] = s;
  }
  for (int i = 0; i < n; i++) y[i] /= d[i];
  for (int i = n - 1; i >= 0; i--) {   // L^T x = y
    double s = y[i];
    for (int k = i + 1; k < n; k++) s -= L[(size_t)k * n + i] * y[k];
    y[i] = s;
  }
  for (int i = 0; i < n; i++) x[i] = y[i];
  return 0;
}

// index of (i, j), i <= j, in the row-major upper triangle of an n x n
inline size_t tri_index(int n, int i, int j) { return (size_t)i * n - ((size_t)i * (i - 1)) / 2 + (size_t)(j - i); }

// ellc_joint_solve's body: H = blockdiag(A) - S with its diagonal times (1 + lambda), b = a - s, H xi = -b
inline int joint_solve_record(const ellc_joint_normal* r, double lambda, double* xi) {
  const int B = r->B;
  if (B < 1 || B > ELLC_JOINT_MAX_VIEWS || !(lambda >= 0.0) || !std::isfinite(lambda)) return 1;
  const int n = 6 * B;
  std::vector<double> H((size_t)n * n), g((size_t)n);
  for (int i = 0; i < n; i++) {
    for (int j = i; j < n; j++) {
      double h = -r->S[tri_index(n, i, j)];
      if (i / 6 == j / 6) h = r->A[i / 6][tri_index(6, i % 6, j % 6)] - r->S[tri_index(n, i, j)];
      if (i == j) h *= 1.0 + lambda;
      H[(size_t)i * n + j] = H[(size_t)j * n + i] = h;
    }
    g[i] = r->a[i / 6][i % 6] - r->s[i];
  }
  // a sum that is not finite is refused here, so that every pivot below is finite or fails its test; so is a step that overflowed
  for (size_t k = 0; k < H.size(); k++)
    if (!std::isfinite(H[k])) return 1;
  for (int i = 0; i < n; i++)
    if (!std::isfinite(g[i])) return 1;
  if (ldlt_solve_neg(n, H.data(), g.data(), g.data())) return 1;
  for (int i = 0; i < n; i++)
    if (!std::isfinite(g[i])) return 1;
  for (int i = 0; i < n; i++) xi[i] = g[i];
  return 0;
}

}  // namespace ellc
