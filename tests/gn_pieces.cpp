// gn_pieces.cpp — the pieces of csrc/pf_gn.hpp behind a C interface, for tests/test_gn_pieces_host.py: the header as
// plain host C++ (g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC), loaded with ctypes.  No GPU, no library.
#include "../pf_monocular_pose_estimator_amd/csrc/pf_gn.hpp"

extern "C" {

// sin and cos of n angles
void gnp_sincos(const double* th, int n, double* s, double* c) {
  for (int i = 0; i < n; ++i) pfmpe::gn_sincos(th[i], s[i], c[i]);
}

// A (6 x 6 symmetric, row-major; the lower triangle is read) factored, then A x = b solved and A^-1 formed by
// columns as gn_optimise does.  fac: the 21 words of the factored lower triangle, pv: the 6 exchanges, x: 6,
// inv: 36 row-major.  Returns gn_factor's result; x and inv are computed only when it is true.
int gnp_factor_solve(const double* A, const double* b, double* fac, int* pv, double* x, double* inv) {
  double a[21];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j <= i; ++j) a[PFGN_L(i, j)] = A[i * 6 + j];
  const bool ok = pfmpe::gn_factor(a, pv);
  for (int q = 0; q < 21; ++q) fac[q] = a[q];
  if (!ok) return 0;
  for (int q = 0; q < 6; ++q) x[q] = b[q];
  pfmpe::gn_solve(a, pv, x);
  for (int c = 0; c < 6; ++c) {
    double e[6];
    for (int r = 0; r < 6; ++r) e[r] = (r == c) ? 1.0 : 0.0;
    pfmpe::gn_solve(a, pv, e);
    for (int r = 0; r < 6; ++r) inv[r * 6 + c] = e[r];
  }
  return 1;
}

// P (12 doubles, 3 x 4 row-major) <- exponentialMap(xi) * P, xi = [upsilon; omega]
void gnp_exp_apply(const double* xi, double* P) { pfmpe::gn_exp_apply(xi, P); }

}  // extern "C"
