#pragma once
// pf_gn.hpp — Gauss-Newton pose refinement of one hypothesis over its LED-blob pairs: optimisePose
// (pf_mpe_lib/src/pose_estimator.cpp:1805-2009) with computeJacobian (PE:2163-2192) and exponentialMap
// (PE:2194-2226), in fp64.  One function for the kernel (k_refine, one lane per hypothesis) and the host
// (pfmpe_host_optimise_pose); both sides are built with -ffp-contract=off and share gn_sincos, so they do the same
// arithmetic (+, -, *, /, sqrt and fmod are correctly rounded on both).  What IEEE 754 leaves open is which NaN an
// operation gives (the sign of a generated one, the payload that is passed on): every double of a result goes through
// gn_canon, so a non-finite row is the same bytes on both sides too.
//
// Everything a lane keeps across iterations lives in registers: the pose (12), the lower triangle of A (21), b (6),
// K34 * pose (12) and the pivots (6).  Every array below is indexed by loop counters of fully unrolled loops only;
// the pivot search exchanges rows with compare-and-swap chains (selects on `p == i` for every static i), never with
// an index that is a runtime value, so nothing is demoted to scratch memory.
#include <math.h>
#include <stdint.h>

#include "../../include/pfmpe.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PFGN_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PFGN_HD inline __attribute__((always_inline))
#endif

namespace pfmpe {

// lower-triangle index, i >= j
#define PFGN_L(i, j) ((i) * ((i) + 1) / 2 + (j))

// compare-and-swap as two selects (a branch around a swap invites the compiler to index the array by the runtime row)
PFGN_HD void gn_cswap(const bool sw, double& x, double& y) {
  const double a = x, b = y;
  x = sw ? b : a;
  y = sw ? a : b;
}

// P A P for the transposition (k p), k < p, on the lower triangle: the diagonal pair, the rows' parts left of column
// k (the multipliers already stored there), the column / row parts between and below.  a[p][k] stays.
PFGN_HD void gn_sym_swap(const bool sw, double* a, const int k, const int p) {
  gn_cswap(sw, a[PFGN_L(k, k)], a[PFGN_L(p, p)]);
#pragma unroll
  for (int j = 0; j < 6; ++j)
    if (j < k) gn_cswap(sw, a[PFGN_L(k, j)], a[PFGN_L(p, j)]);
#pragma unroll
  for (int i = 0; i < 6; ++i)
    if (i > k && i < p) gn_cswap(sw, a[PFGN_L(i, k)], a[PFGN_L(p, i)]);
#pragma unroll
  for (int i = 0; i < 6; ++i)
    if (i > p) gn_cswap(sw, a[PFGN_L(i, k)], a[PFGN_L(i, p)]);
}

// A.ldlt() in place: L D L^T with Eigen's symmetric diagonal pivoting (the largest remaining |diagonal|, the first
// one among equals).  pv[k] is the row exchanged with row k.  false when a pivot is exactly 0.
PFGN_HD bool gn_factor(double* a, int* pv) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    int p = k;
    double dm = fabs(a[PFGN_L(k, k)]);
#pragma unroll
    for (int i = k + 1; i < 6; ++i) {
      const double di = fabs(a[PFGN_L(i, i)]);
      if (di > dm) {
        dm = di;
        p = i;
      }
    }
    pv[k] = p;
#pragma unroll
    for (int i = k + 1; i < 6; ++i)
      gn_sym_swap(p == i, a, k, i);
    const double d = a[PFGN_L(k, k)];
    if (d == 0.0) ok = false;
    double l[6];
#pragma unroll
    for (int i = k + 1; i < 6; ++i) l[i] = a[PFGN_L(i, k)] / d;
    // the Schur update reads the original column k; the multipliers are stored afterwards
#pragma unroll
    for (int i = k + 1; i < 6; ++i)
#pragma unroll
      for (int j = k + 1; j <= i; ++j) a[PFGN_L(i, j)] -= l[i] * a[PFGN_L(j, k)];
#pragma unroll
    for (int i = k + 1; i < 6; ++i) a[PFGN_L(i, k)] = l[i];
  }
  return ok;
}

// x = A^-1 x through the factors: the row exchanges, L, D, L^T, the exchanges undone in reverse order
PFGN_HD void gn_solve(const double* a, const int* pv, double* x) {
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int i = k + 1; i < 6; ++i)
      gn_cswap(pv[k] == i, x[k], x[i]);
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < i; ++j) x[i] -= a[PFGN_L(i, j)] * x[j];
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] /= a[PFGN_L(i, i)];
#pragma unroll
  for (int i = 5; i >= 0; --i)
#pragma unroll
    for (int j = i + 1; j < 6; ++j) x[i] -= a[PFGN_L(j, i)] * x[j];
#pragma unroll
  for (int k = 5; k >= 0; --k)
#pragma unroll
    for (int i = k + 1; i < 6; ++i)
      gn_cswap(pv[k] == i, x[k], x[i]);
}

// sin and cos of th >= 0, the same arithmetic on the host and on the device (the math libraries of the two sides
// round differently, and the iteration count follows the last bit: with this the host function is the kernel's lane
// to the bit).  Reduction to |y| <= pi/4 by quarter turns with pi/2 in two parts (Cody-Waite), then the kernels of
// fdlibm's k_sin.c / k_cos.c (Copyright (C) 1993 by Sun Microsystems, Inc.  Developed at SunPro.  Permission to use,
// copy, modify, and distribute this software is freely granted, provided that this notice is preserved): within 1 ulp
// for the angles a Gauss-Newton step takes.  Above 1e5 rad the angle is first taken modulo the double nearest 2 pi
// (exact fmod): the result stays in [-1, 1], its error grows with th * 2^-53.  Not finite: NaN.
PFGN_HD void gn_sincos(const double th, double& s, double& c) {
  if (!(th - th == 0.0)) {
    s = c = th - th;
    return;
  }
  const double x = th > 1e5 ? fmod(th, 6.283185307179586) : th;
  const double n = floor(x * 6.36619772367581382433e-01 + 0.5);  // quarter turns
  const double r = x - n * 1.57079632673412561417e+00;            // pi/2, first 33 bits
  const double w = n * 6.07710050650619224932e-11;                // pi/2 - the above
  const double y = r - w, t = (r - y) - w;                        // y + t = x - n pi/2
  const double z = y * y, z2 = z * z, v = z * y;
  const double rs = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * 2.75573137070700676789e-06) +
                    z * z2 * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10);
  const double ks = y - ((z * (0.5 * t - v * rs) - t) - v * -1.66666666666666324348e-01);
  const double rc = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * 2.48015872894767294178e-05)) +
                    (z2 * z2) * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11));
  const double hz = 0.5 * z, wc = 1.0 - hz;
  const double kc = wc + (((1.0 - wc) - hz) + (z * rc - y * t));
  const int q = (int)n & 3;
  s = q == 0 ? ks : (q == 1 ? kc : (q == 2 ? -ks : -kc));
  c = q == 0 ? kc : (q == 1 ? -ks : (q == 2 ? -kc : ks));
}

// pose = exponentialMap(xi) * pose (PE:1880, PE:2194-2226), xi = [upsilon; omega]; the product as the 4x4 one
PFGN_HD void gn_exp_apply(const double* xi, double* P) {
  const double th = sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]), th2 = th * th;
  const double O[9] = {0, -xi[5], xi[4], xi[5], 0, -xi[3], -xi[4], xi[3], 0};
  double O2[9], R[9], V[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) O2[i * 3 + j] = O[i * 3] * O[j] + O[i * 3 + 1] * O[3 + j] + O[i * 3 + 2] * O[6 + j];
  double s = 0.0, c = 1.0;
  if (th != 0.0) gn_sincos(th, s, c);
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const double I = (i % 4 == 0) ? 1.0 : 0.0;
    R[i] = I;
    V[i] = I;
    if (th != 0.0) {
      R[i] = I + O[i] / th * s + O2[i] / th2 * (1 - c);
      V[i] = I + (1 - c) / th2 * O[i] + (th - s) / (th2 * th) * O2[i];
    }
  }
  double t[3], N[12];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = V[i * 3] * xi[0] + V[i * 3 + 1] * xi[1] + V[i * 3 + 2] * xi[2];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double v = R[i * 3] * P[j];
      v = v + R[i * 3 + 1] * P[4 + j];
      v = v + R[i * 3 + 2] * P[8 + j];
      v = v + t[i] * (j == 3 ? 1.0 : 0.0);
      N[i * 4 + j] = v;
    }
#pragma unroll
  for (int q = 0; q < 12; ++q) P[q] = N[q];
}

// Q = K34 * pose (project2d, PE:1017-1034): computed once per pose, used for every pair
PFGN_HD void gn_kt(const double* K, const double* P, double* Q) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double s = K[i * 3] * P[j];
      s = s + K[i * 3 + 1] * P[4 + j];
      s = s + K[i * 3 + 2] * P[8 + j];
      s = s + 0.0 * (j == 3 ? 1.0 : 0.0);
      Q[i * 4 + j] = s;
    }
}
// e = z - project2d(X)
PFGN_HD void gn_residual(const double* Q, const double* X, const double* z, double* e) {
  double p[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double s = Q[i * 4] * X[0];
    s = s + Q[i * 4 + 1] * X[1];
    s = s + Q[i * 4 + 2] * X[2];
    s = s + Q[i * 4 + 3] * 1.0;
    p[i] = s;
  }
  e[0] = z[0] - p[0] / p[2];
  e[1] = z[1] - p[1] / p[2];
}

// a NaN as one bit pattern (the positive quiet NaN without payload); every other value as it is
PFGN_HD double gn_canon(const double v) { return v == v ? v : __builtin_nan(""); }

// One hypothesis.  markers: M x 3, K: 3 x 3 row-major, blobs: B x 2, corr: n_rows 1-based (LED, blob) rows of which
// those with blob 0 are skipped, pose0: the 12 doubles of the start pose (read again for the divergence rule, not
// kept).  The indices are the caller's to check.  cov36: 36 doubles.
PFGN_HD void gn_optimise(const double* markers, const double* K, const double* blobs, const uint32_t* corr,
                         const int n_rows, const int max_iter, const int revert, const double converged,
                         const double* pose0, pfmpe_refine_row& out, double* cov36) {
  int np = 0, nr = 0;
  for (int j = 0; j < n_rows; ++j)
    if (corr[2 * j + 1] != 0u) {
      ++np;
      nr = j + 1;
    }
  double P[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) P[q] = pose0[q];
  out.n_pairs = np;
  out.pad = 0;
  if (np == 0) {
#pragma unroll
    for (int q = 0; q < 12; ++q) out.pose[q] = P[q];
    out.rms_before = out.rms_after = 0.0;
    out.iters = 0;
    out.status = PFMPE_REFINE_NO_PAIRS;
#pragma unroll
    for (int q = 0; q < 36; ++q) cov36[q] = 0.0;
    return;
  }
  const double fx = K[0], fy = K[4];
  double a[21], Q[12];
  int pv[6];
  bool ok = false, conv = false, reverted = false;
  double e_init = 0.0, e_end = 0.0, ss0 = 0.0;
  int iters = max_iter;
  for (int it = 0; it < max_iter; ++it) {
    double b[6];
#pragma unroll
    for (int q = 0; q < 21; ++q) a[q] = 0.0;
#pragma unroll
    for (int q = 0; q < 6; ++q) b[q] = 0.0;
    gn_kt(K, P, Q);
    for (int j = 0; j < nr; ++j) {
      const uint32_t led = corr[2 * j], blob = corr[2 * j + 1];
      if (blob == 0u) continue;
      const double* Xp = markers + 3 * (size_t)(led - 1u);
      const double* zp = blobs + 2 * (size_t)(blob - 1u);
      const double X[3] = {Xp[0], Xp[1], Xp[2]}, z[2] = {zp[0], zp[1]};
      double e[2];
      gn_residual(Q, X, z, e);
      const double e2 = e[0] * e[0] + e[1] * e[1];
      // the reference's `=+`: the last used pair's error norm, at iteration 0 and at the last allowed iteration
      if (it == 0) {
        e_init = sqrt(e2);
        ss0 = ss0 + e2;
      } else if (it + 1 == max_iter) {
        e_end = sqrt(e2);
      }
      double pc[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) pc[r] = P[r * 4] * X[0] + P[r * 4 + 1] * X[1] + P[r * 4 + 2] * X[2] + P[r * 4 + 3];
      const double x = pc[0], y = pc[1], zz = pc[2], z2 = zz * zz;
      double J[12];
      J[0] = 1 / zz * fx; J[1] = 0; J[2] = -x / z2 * fx; J[3] = -x * y / z2 * fx;
      J[4] = (1 + (x * x / z2)) * fx; J[5] = -y / zz * fx;
      J[6] = 0; J[7] = 1 / zz * fy; J[8] = -y / z2 * fy; J[9] = -(1 + y * y / z2) * fy;
      J[10] = x * y / z2 * fy; J[11] = x / zz * fy;
#pragma unroll
      for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = 0; c <= r; ++c) a[PFGN_L(r, c)] += J[r] * J[c] + J[6 + r] * J[6 + c];
        b[r] += J[r] * e[0] + J[6 + r] * e[1];
      }
    }
    ok = gn_factor(a, pv);
    if (ok) {
      gn_solve(a, pv, b);
    } else {
#pragma unroll
      for (int q = 0; q < 6; ++q) b[q] = 0.0;
    }
    gn_exp_apply(b, P);
    double nm = -1.0;  // std::max(nm, |dT|): a NaN entry is passed over
#pragma unroll
    for (int q = 0; q < 6; ++q) nm = nm < fabs(b[q]) ? fabs(b[q]) : nm;
    if (nm <= converged) {
      iters = it;
      conv = true;
      break;
    }
    if (it + 1 == max_iter && e_init < e_end && revert) {
#pragma unroll
      for (int q = 0; q < 12; ++q) P[q] = pose0[q];
      reverted = true;
    }
  }
  // pose_covariance_ = A.inverse() of the last A formed (PE:2004), a column per solve
  if (ok) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double x[6];
#pragma unroll
      for (int r = 0; r < 6; ++r) x[r] = (r == c) ? 1.0 : 0.0;
      gn_solve(a, pv, x);
#pragma unroll
      for (int r = 0; r < 6; ++r) cov36[r * 6 + c] = gn_canon(x[r]);
    }
  } else {
#pragma unroll
    for (int q = 0; q < 36; ++q) cov36[q] = 0.0;
  }
  gn_kt(K, P, Q);
  double ss1 = 0.0;
  for (int j = 0; j < nr; ++j) {
    const uint32_t led = corr[2 * j], blob = corr[2 * j + 1];
    if (blob == 0u) continue;
    const double* Xp = markers + 3 * (size_t)(led - 1u);
    const double* zp = blobs + 2 * (size_t)(blob - 1u);
    const double X[3] = {Xp[0], Xp[1], Xp[2]}, z[2] = {zp[0], zp[1]};
    double e[2];
    gn_residual(Q, X, z, e);
    ss1 = ss1 + (e[0] * e[0] + e[1] * e[1]);
  }
#pragma unroll
  for (int q = 0; q < 12; ++q) out.pose[q] = gn_canon(P[q]);
  out.rms_before = gn_canon(sqrt(ss0 / (double)np));
  out.rms_after = gn_canon(sqrt(ss1 / (double)np));
  out.iters = iters;
  out.status = conv ? PFMPE_REFINE_CONVERGED : (reverted ? PFMPE_REFINE_CAP_REVERTED : PFMPE_REFINE_CAP_KEPT);
}

// the order of the best hypothesis: most pairs, then the smallest rms_after, then the lowest index; a hypothesis
// without pairs or with a non-finite rms_after does not take part (idx < 0: none)
PFGN_HD bool gn_better(int np1, double r1, int64_t i1, int np2, double r2, int64_t i2) {
  if (i1 < 0) return false;
  if (i2 < 0) return true;
  if (np1 != np2) return np1 > np2;
  if (r1 != r2) return r1 < r2;
  return i1 < i2;
}
PFGN_HD bool gn_eligible(const pfmpe_refine_row& r) {
  return r.n_pairs > 0 && r.rms_after - r.rms_after == 0.0;
}
// the parameters every refinement entry point accepts
inline bool refine_params_ok(const pfmpe_refine_params& p) {
  return p.max_iter >= 1 && p.max_iter <= 10000 && p.converged >= 0.0;  // (a NaN fails the comparison)
}

}  // namespace pfmpe
