#pragma once
// pf_modes.hpp — a particle of a cloud entry as the statistics read it, and the assignment of every particle to its
// nearest seed pose: the one definition of mode_dist / mode_assign and of k_cloud_assign, shared by pfmpe_cloud_modes,
// pfmpe_host_cloud_assign (pfmpe_cloud.hip) and pfmpe_resample_prior (pfmpe_resample_prior.hip).
#include <float.h>

#include <cmath>
#include <cstring>

#include "../../include/pfmpe.h"
#include "pf_state.hpp"
#include "pf_wave.hpp"

namespace pfmpe {

// The grid is a function of N alone (one N, one reduction tree): a block per 256 particles up to 1024 blocks (two
// rounds of the resident grid: 256 CUs x 2 blocks at the kernel's ~210 VGPRs), grid-stride beyond.
constexpr int kCloudMaxBlocks = 1024;
inline int cloud_blocks(int N) {
  const int b = (N + kBlock - 1) / kBlock;
  return b < kCloudMaxBlocks ? b : kCloudMaxBlocks;
}
struct CloudArgs {
  double ref[12], anchor[12];
  int32_t N, pad;
  int64_t ld;
  const uint32_t* owner;  // a deferred prior's owner indices (FrameArgsT::owner), or null
  const double* dense;    // dense: N x 12 poses (the regenerated kept set)
  const void* w;          // dense: its raw weights (compute type T)
};
struct CloudDesc {
  CloudArgs a;
  const void* st;          // resident: the prior's storage (SP planes); dense: unused
  const uint8_t* mode_of;  // a filtered entry (pfmpe_cloud_modes): every particle's mode, k_cloud_assign's output
  int32_t dense;
  int32_t mode;            // a filtered entry reduces the particles with mode_of[n] == mode, in the entry's order
};
// Particle n of an entry as the statistics read it, for every kernel that reads an entry: a dense entry's row and its
// weight widened as k_weights_export widens it; a resident entry's prior row through the owner indices and the fp16
// anchor, exactly what k_export writes, with unit weight.  dense is wave-uniform.
template <typename T, typename SP>
__device__ __forceinline__ void cloud_load(const CloudArgs& ca, const SP* __restrict__ st, bool dense, int64_t n,
                                           double* P, double& w) {
  if (dense) {
#pragma unroll
    for (int q = 0; q < 12; ++q) P[q] = ca.dense[12 * n + q];
    w = (double)((const T*)ca.w)[n];
  } else {
    const int64_t r = ca.owner ? (int64_t)ca.owner[n] : n;
#pragma unroll
    for (int q = 0; q < 12; ++q)
      P[q] = (double)StateIO<T, SP>::load(st[plane_index<SP>(q, r, ca.ld)], (T)ca.anchor[q]);
  }
}

// ---- the assignment (pfmpe_cloud_modes; the definition is in include/pfmpe.h): every particle goes to its nearest seed
constexpr int kModesMax = 16;
constexpr int kModeNone = 255;
static_assert(PFMPE_MODES_MAX == kModesMax && PFMPE_MODE_NONE == kModeNone, "mode constants");
// The seeds and the scales as the distance uses them, formed once on the host: it2 = 1 / trans_scale^2 and
// ir2 = 1 / rot_scale^2 (0 for a scale of 0).  A kernel argument: wave-uniform, read with scalar loads.
struct ModeSeeds {
  double seed[kModesMax][12];
  double it2, ir2, max_dist;
  int32_t K, pad;
};
inline double mode_inv2(double scale) { return scale > 0.0 ? 1.0 / (scale * scale) : 0.0; }
// Distance of pose p to seed s: d2 and tr as top_near (pf_top.hpp) forms them, fp64 on the 12-double rows, every
// product and sum rounded on its own, in the order written; the same function on both sides, so the device's
// assignment equals pfmpe_host_cloud_assign's bit for bit.
__host__ __device__ inline double mode_dist(const double* p, const double* s, double it2, double ir2) {
#pragma clang fp contract(off)
  const double dx = p[3] - s[3], dy = p[7] - s[7], dz = p[11] - s[11];
  double d2 = dx * dx;
  d2 = d2 + dy * dy;
  d2 = d2 + dz * dz;
  double tr = p[0] * s[0];
  tr = tr + p[1] * s[1];
  tr = tr + p[2] * s[2];
  tr = tr + p[4] * s[4];
  tr = tr + p[5] * s[5];
  tr = tr + p[6] * s[6];
  tr = tr + p[8] * s[8];
  tr = tr + p[9] * s[9];
  tr = tr + p[10] * s[10];
  const double a = d2 * it2;
  const double b = (3.0 - tr) * ir2;
  return a + b;
}
// The nearest seed: the lowest k among equal distances; a NaN or infinite distance (of either sign: an infinite
// rotation entry can give -inf) never wins; with a gate, a particle farther than max_dist from every seed has none.
__host__ __device__ inline int mode_assign(const double* p, const ModeSeeds& ms) {
  double best = (double)INFINITY;
  int mode = kModeNone;
  for (int k = 0; k < ms.K; ++k) {
    const double dist = mode_dist(p, ms.seed[k], ms.it2, ms.ir2);
    if (dist < best && dist >= -DBL_MAX) {
      best = dist;
      mode = k;
    }
  }
  if (ms.max_dist > 0.0 && !(best <= ms.max_dist)) mode = kModeNone;
  return mode;
}
// One lane per particle over cloud_blocks(N) blocks, grid-stride beyond: mode_of[n] = the mode of particle n of the
// entry `d` (read as k_cloud_multi reads it), counts[k] += the members of mode k, counts[K] those without a mode.
// Every output is order-free: a byte per particle, and integer adds (a wave counts a mode with one ballot, lane k
// keeps mode k's count; the block's waves meet in LDS and each non-empty bin goes out with one device atomic, the
// k_top_hist idiom).  The host clears counts before the launch.
template <typename T, typename SP>
__global__ __launch_bounds__(kBlock) void k_cloud_assign(const CloudDesc d, const ModeSeeds ms,
                                                        uint8_t* __restrict__ mode_of, uint32_t* __restrict__ counts) {
  __shared__ uint32_t bins[kModesMax + 1];
  if (threadIdx.x <= kModesMax) bins[threadIdx.x] = 0u;
  __syncthreads();
  const CloudArgs& ca = d.a;
  const bool dense = d.dense != 0;  // wave-uniform
  const SP* __restrict__ st = (const SP*)d.st;
  const int lane = lane_id();
  uint32_t mine = 0u;  // lane k <= K: this wave's particles in bin k
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t n0 = (int64_t)blockIdx.x * kBlock; n0 < ca.N; n0 += stride) {  // block-uniform trips: ballots
    const int64_t n = n0 + threadIdx.x;
    int bin = -1;
    if (n < ca.N) {
      double P[12], w = 1.0;  // (the weight plays no part in the assignment)
      cloud_load<T, SP>(ca, st, dense, n, P, w);
      const int mode = mode_assign(P, ms);
      mode_of[n] = (uint8_t)mode;
      bin = mode == kModeNone ? ms.K : mode;
    }
    for (int k = 0; k <= ms.K; ++k) {
      const uint32_t c = (uint32_t)__popcll(__ballot(bin == k));
      mine += lane == k ? c : 0u;
    }
  }
  if (mine) (void)__hip_atomic_fetch_add(bins + lane, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();
  if ((int)threadIdx.x <= ms.K) {
    const uint32_t x = bins[threadIdx.x];
    if (x) (void)__hip_atomic_fetch_add(counts + threadIdx.x, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// the K + 1 member counts in front of pfmpe_ctx::d_modes' bytes
constexpr size_t kModesCountBytes = 256;
static_assert((kModesMax + 1) * sizeof(uint32_t) <= kModesCountBytes, "the counts of a call");

// the checks pfmpe_cloud_modes, pfmpe_host_cloud_assign and pfmpe_resample_prior share: K, the seeds, the parameters
inline const char* modes_args_bad(const double* seeds, int K, const pfmpe_modes_params& p) {
  if (K < 1 || K > PFMPE_MODES_MAX) return "K outside 1..PFMPE_MODES_MAX";
  for (int q = 0; q < 12 * K; ++q)
    if (!std::isfinite(seeds[q])) return "non-finite seed";
  for (const double v : {p.trans_scale, p.rot_scale, p.max_dist})
    if (!(v >= 0.0) || !std::isfinite(v)) return "a scale or max_dist is negative or not finite";
  if (p.trans_scale == 0.0 && p.rot_scale == 0.0) return "both scales are 0";
  return nullptr;
}
inline ModeSeeds mode_seeds(const double* seeds, int K, const pfmpe_modes_params& p) {
  ModeSeeds ms{};
  std::memcpy(ms.seed, seeds, (size_t)K * 12 * sizeof(double));
  ms.it2 = mode_inv2(p.trans_scale);
  ms.ir2 = mode_inv2(p.rot_scale);
  ms.max_dist = p.max_dist;
  ms.K = K;
  return ms;
}

}  // namespace pfmpe
