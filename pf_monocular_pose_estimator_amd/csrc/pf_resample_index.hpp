#pragma once
// pf_resample_index.hpp — the index rule of pfmpe_resample_prior (include/pfmpe.h): which member of the source set a
// slot of the new prior copies, and which slots a member owns.  Integers only; host and device code (PFRS_HD), so the
// kernels of pfmpe_resample_prior.hip and pfmpe_host_resample_source evaluate the same functions.
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PFRS_HD __host__ __device__ __forceinline__
#else
#define PFRS_HD inline __attribute__((always_inline))
#endif

namespace pfmpe {

constexpr int64_t kResampleMaxCount = 2147483647;  // N and n_new: 2k + 1 < 2^32 and m < 2^31, so no product overflows

// Slot k of n_new copies the member of rank r = ((2k + 1) m) / (2 n_new) among the m members in ascending particle
// index: systematic resampling of unit weights with offset 1/2.  0 <= k < n_new, m >= 1: 0 <= r < m, non-decreasing in k.
PFRS_HD uint64_t resample_rank(uint64_t k, uint64_t m, uint64_t n_new) { return ((2u * k + 1u) * m) / (2u * n_new); }

// The first slot whose rank is >= r, 0 <= r <= m: rank(k) >= r <=> (2k + 1) m >= 2 n_new r <=> 2k + 1 >= x with
// x = ceil(2 n_new r / m) <=> k >= floor(x / 2).  Rank r owns the slots first_slot(r) .. first_slot(r + 1) - 1, a
// possibly empty run; first_slot(0) = 0 and first_slot(m) = n_new.  (2 n_new r + m - 1 < 2^63.)
PFRS_HD uint64_t resample_first_slot(uint64_t r, uint64_t m, uint64_t n_new) {
  return ((2u * n_new * r + m - 1u) / m) >> 1;
}

// source[k] = the particle slot k copies, for the members n with mode_of[n] == mode (mode_of null: every particle) of
// N particles; *n_members = m.  With m == 0 no source entry is written.  The arguments are the caller's to check.
inline void resample_source(const uint8_t* mode_of, int64_t N, int mode, int64_t n_new, int32_t* source,
                            int64_t* n_members) {
  int64_t m = N;
  if (mode_of) {
    m = 0;
    for (int64_t n = 0; n < N; ++n) m += (int)mode_of[n] == mode ? 1 : 0;
  }
  *n_members = m;
  if (m == 0) return;
  int64_t n = -1, seen = -1;  // particle n is the member of rank `seen`
  for (int64_t k = 0; k < n_new; ++k) {
    const int64_t r = (int64_t)resample_rank((uint64_t)k, (uint64_t)m, (uint64_t)n_new);
    while (seen < r) {
      ++n;
      if (!mode_of || (int)mode_of[n] == mode) ++seen;
    }
    source[k] = (int32_t)n;
  }
}

}  // namespace pfmpe
