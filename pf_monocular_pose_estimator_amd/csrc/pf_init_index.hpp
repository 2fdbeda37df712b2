#pragma once
// pf_init_index.hpp — the index maps of the brute-force (re)initialisation (pfmpe_init.hip): a work item's number to
// its blob combination, its ordered marker triple and the markers the triple leaves unused.  Host and device code
// (PFP3P_HD, pf_p3p.hpp): tests/p3p_pieces.cpp builds it with g++ and tests/test_p3p_pieces_host.py walks every index.
#include <stdint.h>

#include "pf_p3p.hpp"

namespace pfmpe {

PFP3P_HD int64_t c3(int64_t n) { return n * (n - 1) * (n - 2) / 6; }
PFP3P_HD int64_t c2(int64_t n) { return n * (n - 1) / 2; }

// colex rank r -> a < b < c with r = C(c,3) + C(b,2) + a
PFP3P_HD void unrank3(int64_t r, int& a, int& b, int& c) {
  int cc = (int)cbrt(6.0 * (double)r);
  cc = cc < 2 ? 2 : cc;
  while (c3(cc) > r) --cc;
  while (c3(cc + 1) <= r) ++cc;
  const int64_t r2 = r - c3(cc);
  int bb = (int)sqrt(2.0 * (double)r2);
  bb = bb < 1 ? 1 : bb;
  while (c2(bb) > r2) --bb;
  while (c2(bb + 1) <= r2) ++bb;
  a = (int)(r2 - c2(bb));
  b = bb;
  c = cc;
}

// p-th ordered triple of distinct markers (any fixed order: the histogram is a commutative sum)
PFP3P_HD void perm3(int p, int M, int& i0, int& i1, int& i2) {
  const int m12 = (M - 1) * (M - 2);
  i0 = p / m12;
  const int rem = p - i0 * m12;
  const int j1 = rem / (M - 2);
  const int j2 = rem - j1 * (M - 2);
  i1 = j1 + (j1 >= i0 ? 1 : 0);
  const int lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
  i2 = j2;
  if (i2 >= lo) ++i2;
  if (i2 >= hi) ++i2;
}

// un[m] = the m-th index of {0, 1, ...} without x, y, z (ascending), in registers (no scratch)
template <int MAXU>
PFP3P_HD void unused_markers(int x, int y, int z, int* un) {
  const int yz_lo = y < z ? y : z, yz_hi = y < z ? z : y;
  const int lo = x < yz_lo ? x : yz_lo, hi = x > yz_hi ? x : yz_hi, mid = x + y + z - lo - hi;
#pragma unroll
  for (int m = 0; m < MAXU; ++m) {
    int v = m;
    v += v >= lo ? 1 : 0;
    v += v >= mid ? 1 : 0;
    v += v >= hi ? 1 : 0;
    un[m] = v;
  }
}

}  // namespace pfmpe
