#pragma once
// pf_top.hpp — pfmpe_top_particles: the K best distinct hypotheses of the last step's kept propagated set (the
// definition is in include/pfmpe.h).  Here: the separation predicate and the suppression walk, shared by the device
// and pfmpe_host_top_suppress; the keys as ordered bit patterns; the scratch layout.  The kernels, their launches and the
// entry point are in pfmpe_top.hip.
#include <math.h>
#include <stdint.h>

#include "../../include/pfmpe.h"
#include "pf_types.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PFTOP_HD __host__ __device__ inline
#else
#define PFTOP_HD inline
#endif

struct pfmpe_ctx;

namespace pfmpe {

constexpr int kTopPool = PFMPE_TOP_POOL;     // ranked candidates the suppression walks
constexpr int kTopWords = kTopPool / 32;     // words of one row of the near-matrix (and of the kept mask)
constexpr int kTopDigitBits = 11;            // radix-select digit
constexpr int kTopBins = 1 << kTopDigitBits;
constexpr int kTopMaxPasses = 6;             // 64-bit keys: 11 + 11 + 11 + 11 + 11 + 9 bits
// the grid rule of cloud_blocks / kAssocMaxBlocks: a block per 256 particles up to 1024 blocks, strips beyond
constexpr int kTopMaxBlocks = 1024;
static_assert(PFMPE_TOP_MAX <= PFMPE_TOP_POOL && kTopPool % 32 == 0, "the rows come out of the pool");

// The thresholds as the predicate uses them, formed once on the host: t2 = min_trans * min_trans,
// rc = 1 + 2 * cos(min_rot).
struct TopThresholds {
  double min_trans, t2, min_rot, rc;
};
inline TopThresholds top_thresholds(double min_trans, double min_rot) {
  TopThresholds t;
  t.min_trans = min_trans;
  t.t2 = min_trans * min_trans;
  t.min_rot = min_rot;
  t.rc = 1.0 + 2.0 * cos(min_rot);
  return t;
}

// Candidate j is near the kept candidate i: closer than min_trans AND rotated by less than min_rot (a threshold of 0
// does not separate).  fp64 on the 12-double poses (r00 r01 r02 t0 r10 ...), every product and sum rounded on its own,
// in the order written; the same function on both sides, so the device walk equals the host walk bit for bit.
PFTOP_HD bool top_near(const double* pj, const double* pi, const TopThresholds& th) {
#pragma clang fp contract(off)
  const double dx = pj[3] - pi[3], dy = pj[7] - pi[7], dz = pj[11] - pi[11];
  double d2 = dx * dx;
  d2 = d2 + dy * dy;
  d2 = d2 + dz * dz;
  const bool near_t = th.min_trans == 0.0 || d2 < th.t2;
  double tr = pj[0] * pi[0];
  tr = tr + pj[1] * pi[1];
  tr = tr + pj[2] * pi[2];
  tr = tr + pj[4] * pi[4];
  tr = tr + pj[5] * pi[5];
  tr = tr + pj[6] * pi[6];
  tr = tr + pj[8] * pi[8];
  tr = tr + pj[9] * pi[9];
  tr = tr + pj[10] * pi[10];
  const bool near_r = th.min_rot == 0.0 || tr > th.rc;
  return near_t && near_r;
}

// The suppression walk over P poses in rank order: candidate j is kept unless a kept one is near it; stops at K kept
// or at the end of the list.  keep: positions within the list.  Both thresholds 0: no suppression, the first
// min(K, P).
inline void top_walk(const double* poses, int P, int K, const TopThresholds& th, int32_t* keep, int32_t* n_out,
                     int32_t* n_examined) {
  const bool suppress = th.min_trans != 0.0 || th.min_rot != 0.0;
  int kept = 0, j = 0;
  for (; j < P && kept < K; ++j) {
    bool near = false;
    for (int i = 0; suppress && i < kept && !near; ++i) near = top_near(poses + 12 * (size_t)j, poses + 12 * (size_t)keep[i], th);
    if (!near) keep[kept++] = j;
  }
  *n_out = kept;
  *n_examined = j;
}

// ---- the keys as unsigned integers that order like the values: an eligible key is > 0, so its bit pattern (fp32 or
// fp64 weight, uint32 count) orders like its value; every other key (0, -0, negative, NaN) maps to 0 = not eligible.
template <typename KT>
struct TopKey;
template <>
struct TopKey<float> {
  using U = uint32_t;
  static constexpr int kBits = 32;
  PFTOP_HD static U bits(float x) {
    union {
      float f;
      uint32_t u;
    } c;
    c.f = x;
    return x > 0.0f ? c.u : 0u;
  }
  PFTOP_HD static double value(uint64_t b) {
    union {
      float f;
      uint32_t u;
    } c;
    c.u = (uint32_t)b;
    return (double)c.f;
  }
};
template <>
struct TopKey<double> {
  using U = uint64_t;
  static constexpr int kBits = 64;
  PFTOP_HD static U bits(double x) {
    union {
      double f;
      uint64_t u;
    } c;
    c.f = x;
    return x > 0.0 ? c.u : 0ull;
  }
  PFTOP_HD static double value(uint64_t b) {
    union {
      double f;
      uint64_t u;
    } c;
    c.u = b;
    return c.f;
  }
};
template <>
struct TopKey<uint32_t> {
  using U = uint32_t;
  static constexpr int kBits = 32;
  PFTOP_HD static U bits(uint32_t x) { return x; }
  PFTOP_HD static double value(uint64_t b) { return (double)(uint32_t)b; }
};
// digit passes of a key type, and pass p's shift and width (most significant digit first)
constexpr int top_passes(int bits) { return (bits + kTopDigitBits - 1) / kTopDigitBits; }
PFTOP_HD int top_shift(int bits, int pass) {
  const int s = bits - kTopDigitBits * (pass + 1);
  return s > 0 ? s : 0;
}
PFTOP_HD int top_width(int bits, int pass) {
  const int w = bits - kTopDigitBits * pass;
  return w < kTopDigitBits ? w : kTopDigitBits;
}
static_assert(top_passes(64) == kTopMaxPasses, "digit passes");

// blocks of the selection's kernels and the contiguous strip of each (a multiple of 4 keys: the vector loads stay
// aligned); block b ranks particles b * strip .. min(N, (b + 1) * strip) - 1, so block order is index order
inline int top_blocks(int N) {
  const int b = (N + kBlock - 1) / kBlock;
  return b < kTopMaxBlocks ? (b > 0 ? b : 1) : kTopMaxBlocks;
}
PFTOP_HD int top_strip(int N, int nblk) {
  const int per = (int)(((int64_t)N + nblk - 1) / nblk);
  return (per + 3) & ~3;
}

// The state of the radix select: entering pass p (state[p]) and, in state[kTopMaxPasses], the result.
struct TopState {
  uint64_t prefix;     // the digits decided so far, in place (the result: the threshold key)
  uint32_t need;       // candidates still to take among the keys that carry the prefix (the result: the keys equal to
                       // the threshold that are taken, lowest index first)
  uint32_t done;       // every key that carries the prefix is taken: no later pass narrows further
  int64_t n_positive;  // eligible keys
  uint32_t pool;       // min(kTopPool, n_positive)
  uint32_t pad;
};
static_assert(sizeof(TopState) == 32, "select state");
struct TopBlockCount {
  uint32_t gt, eq;  // keys of the block's strip above / equal to the threshold
};

// what the last kernel writes and the host reads back in one copy: this header, then the rows of K particles
struct TopRecord {
  int64_t n_positive;
  int32_t n_out, n_examined;
};
struct TopRows {  // byte offsets of the row arrays behind the header, for `rows` rows
  static constexpr size_t kKey = sizeof(TopRecord);
  static size_t poses(int rows) { return kKey + (size_t)rows * sizeof(double); }
  static size_t index(int rows) { return poses(rows) + (size_t)rows * 12 * sizeof(double); }
  static size_t n_corr(int rows) { return index(rows) + (size_t)rows * sizeof(int32_t); }
  static size_t corr(int rows) { return n_corr(rows) + (size_t)rows * sizeof(int32_t); }  // 16-byte aligned
  static size_t bytes(int rows) { return corr(rows) + (size_t)rows * 2 * kMaxMarkers * sizeof(uint32_t); }
};
static_assert(sizeof(TopRecord) == 16, "the pair rows stay 16-byte aligned");

// The scratch of the call (pfmpe_ctx::d_top), one allocation of fixed size: nothing in it grows with N.
struct TopBuf {
  static constexpr size_t kHist = 0;  // kTopMaxPasses histograms of kTopBins words, then the states: cleared per call
  static constexpr size_t kState = kHist + (size_t)kTopMaxPasses * kTopBins * sizeof(uint32_t);
  static constexpr size_t kClear = kState + (kTopMaxPasses + 1) * sizeof(TopState);
  static constexpr size_t kBlockCount = kClear;
  static constexpr size_t kCandKey = kBlockCount + (size_t)kTopMaxBlocks * sizeof(TopBlockCount);  // uint64, unsorted
  static constexpr size_t kCandIdx = kCandKey + (size_t)kTopPool * sizeof(uint64_t);
  static constexpr size_t kPoolKey = kCandIdx + (size_t)kTopPool * sizeof(uint32_t);  // double, ranked
  static constexpr size_t kPoolIdx = kPoolKey + (size_t)kTopPool * sizeof(double);
  static constexpr size_t kPoolPoses = kPoolIdx + (size_t)kTopPool * sizeof(int32_t);
  static constexpr size_t kNear = kPoolPoses + (size_t)kTopPool * 12 * sizeof(double);
  static constexpr size_t kRecord = kNear + (size_t)kTopPool * kTopWords * sizeof(uint32_t);
  static size_t bytes() { return kRecord + TopRows::bytes(PFMPE_TOP_MAX); }
};
static_assert(TopBuf::kRecord % 16 == 0 && TopBuf::kCandKey % 8 == 0 && TopBuf::kPoolPoses % 8 == 0, "scratch alignment");

}  // namespace pfmpe
