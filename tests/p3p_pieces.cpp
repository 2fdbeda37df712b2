// p3p_pieces.cpp — the pieces of csrc/pf_p3p.hpp and csrc/pf_init_index.hpp behind a C interface, for
// tests/test_p3p_pieces_host.py: the headers as plain host C++ (g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC, the
// oracle's flags), loaded with ctypes.  No GPU, no library.
//
// p3_cx_op computes each complex operation twice: with the header's Cx, and with std::complex<double> written as
// P3P::solveQuartic writes it.  The std::complex side is the reference's arithmetic, not the header's.  std::pow goes
// through ref_pow: g++ -O2 keeps libstdc++'s pow(complex, double) out of line in the oracle's solve_quartic, with the
// exponent in a register, so its real case is libm's pow for every exponent, 2.0 included; inlined into a loop here
// the compiler would see the 2.0 and multiply instead.
#include <complex>

#include "../pf_monocular_pose_estimator_amd/csrc/pf_init_index.hpp"
#include "../pf_monocular_pose_estimator_amd/csrc/pf_p3p.hpp"

using pfmpe::p3p::Cx;
typedef std::complex<double> cplx;

static __attribute__((noinline, noclone)) cplx ref_pow(const cplx& z, const double& y) { return std::pow(z, y); }

#define P3_LOOP(HDR, REF)                          \
  for (int i = 0; i < n; ++i) {                    \
    const Cx z{zr[i], zi[i]}, w{wr[i], wi[i]};     \
    const cplx Z(zr[i], zi[i]), W(wr[i], wi[i]);   \
    const double x = wr[i];                        \
    (void)w;                                       \
    (void)W;                                       \
    (void)x;                                       \
    const Cx h = HDR;                              \
    const cplx r = REF;                            \
    hdr[2 * i] = h.re;                             \
    hdr[2 * i + 1] = h.im;                         \
    ref[2 * i] = r.real();                         \
    ref[2 * i + 1] = r.imag();                     \
  }                                                \
  return 0

extern "C" {

// hdr, ref (n x 2) <- operation `op` of z = zr + i zi and w = wr + i wi (x = wr where a scalar is the other operand).
// Returns -1 for an unknown op.
int p3_cx_op(int op, int n, const double* zr, const double* zi, const double* wr, const double* wi, double* hdr,
             double* ref) {
  using namespace pfmpe::p3p;
  switch (op) {
    case 0: P3_LOOP(z / w, Z / W);
    case 1: P3_LOOP(z / x, Z / x);
    case 2: P3_LOOP(x / z, x / Z);
    case 3: P3_LOOP(x * z, x * Z);
    case 4: P3_LOOP(x + z, x + Z);
    case 5: P3_LOOP(x - z, x - Z);
    case 6: P3_LOOP(z + w, Z + W);
    case 7: P3_LOOP(z - w, Z - W);
    case 8: P3_LOOP(-z, -Z);
    case 9: P3_LOOP(csqrt(z), std::sqrt(Z));
    case 10: P3_LOOP(clog(z), std::log(Z));
    case 11: P3_LOOP(cpow2(z), ref_pow(Z, 2.0));
    case 12: P3_LOOP(cpow(z, 3.0), ref_pow(Z, 3.0));
    case 13: P3_LOOP(cpow(z, 1.0 / 3.0), ref_pow(Z, 1.0 / 3.0));
  }
  return -1;
}

// setup + the four solutions: fv / wp 3 x 3 with rows = the three unit feature vectors / world points (as orc_p3p).
// Returns -1 when setup returns false (collinear world points), else 0 with sol48 (4 x 12) and roots (4).
int p3_p3p(const double* fv, const double* wp, double* sol48, double* roots) {
  double f[3][3], w[3][3];
  for (int k = 0; k < 3; ++k)
    for (int q = 0; q < 3; ++q) {
      f[k][q] = fv[3 * k + q];
      w[k][q] = wp[3 * k + q];
    }
  pfmpe::p3p::Setup s;
  if (!pfmpe::p3p::setup(f, w, s, roots)) return -1;
  for (int k = 0; k < 4; ++k) pfmpe::p3p::solution(s, roots[k], sol48 + 12 * k);
  return 0;
}

// n problems at once: fv, wp n x 9, sol n x 48, rc n
void p3_p3p_n(int n, const double* fv, const double* wp, double* sol, int* rc) {
  double roots[4];
  for (int i = 0; i < n; ++i) rc[i] = p3_p3p(fv + 9 * i, wp + 9 * i, sol + 48 * i, roots);
}

int p3_finite12(const double* a) { return pfmpe::p3p::finite12(a) ? 1 : 0; }
void p3_inverse34(const double* m12, double* inv12) { pfmpe::p3p::inverse34(m12, inv12); }
void p3_project(const double* K, const double* T12, const double* X, double* uv) {
  pfmpe::p3p::project(K, T12, X, uv[0], uv[1]);
}

void p3_unrank3(int n, const int64_t* r, int* abc) {
  for (int i = 0; i < n; ++i) pfmpe::unrank3(r[i], abc[3 * i], abc[3 * i + 1], abc[3 * i + 2]);
}
int64_t p3_c3(int64_t n) { return pfmpe::c3(n); }
int64_t p3_c2(int64_t n) { return pfmpe::c2(n); }
// all M (M - 1) (M - 2) ordered triples, in the order of p
void p3_perm3_all(int M, int* out) {
  for (int p = 0; p < M * (M - 1) * (M - 2); ++p) pfmpe::perm3(p, M, out[3 * p], out[3 * p + 1], out[3 * p + 2]);
}
// the kernel instance's unused_markers<maxu> (maxu 2, 9 or 13): un receives maxu entries.  Returns -1 for another maxu.
int p3_unused(int maxu, int x, int y, int z, int* un) {
  if (maxu == 2)
    pfmpe::unused_markers<2>(x, y, z, un);
  else if (maxu == 9)
    pfmpe::unused_markers<9>(x, y, z, un);
  else if (maxu == 13)
    pfmpe::unused_markers<13>(x, y, z, un);
  else
    return -1;
  return 0;
}

}  // extern "C"
