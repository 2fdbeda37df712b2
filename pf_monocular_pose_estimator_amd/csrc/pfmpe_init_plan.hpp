#pragma once
// pfmpe_init_plan.hpp — the work mapping of pfmpe_initialise_multi's histogram stage, host C++ without device
// code: shared by the host-only entry point (pfmpe_init_plan.cpp: pfmpe_host_init_plan) and the device call
// (pfmpe_init.hip), which launches exactly this plan.
#include <algorithm>
#include <cstdint>

#include "../../include/pfmpe.h"

namespace pfmpe_plan {

constexpr int kInitBlockThreads = 256;       // threads of a histogram block (one item each per round)
constexpr int kInitBlocksPerCu = 8;          // a launch's block cap per CU
constexpr int64_t kInitLdsHistBytes = 32 * 1024;  // largest histogram kept in LDS

// the unused-marker bucket of M markers: the kernels' MAXU is 2, 9, PFMPE_MAX_MARKERS - 3
inline int init_bucket(int M) { return M - 3 <= 2 ? 0 : M - 3 <= 9 ? 1 : 2; }

// (3-blob combination, ordered 3-marker triple) items of a stream; 0 when the call stops at "too few blobs".
// hist_only: the stream of pfmpe_p3p_histogram, which computes the histogram for 3 <= B < M too.
inline int64_t init_items(int M, int B, bool hist_only = false) {
  if ((B < M && !hist_only) || B < 3) return 0;
  return (int64_t)B * (B - 1) * (B - 2) / 6 * ((int64_t)M * (M - 1) * (M - 2));
}

// The plan of S streams (M[s] markers, B[s] blobs, validated by the caller) on a device of num_cu CUs.  Per bucket:
// a stream wants ceil(items / 256) blocks; when the wants exceed the cap of 8 * max(num_cu, 1) blocks, a stream gets
// floor(want * cap / wants) blocks, and one block where that is zero (so the launch exceeds the cap by at most one
// block per stream with work); first_block is the running sum in ascending stream index.  hist_only: init_items'.
inline void init_plan(const int32_t* M, const int32_t* B, int S, int num_cu, pfmpe_init_plan* plan,
                      int32_t* blocks_per_bucket, bool hist_only = false) {
  const int64_t cap = (int64_t)kInitBlocksPerCu * std::max(num_cu, 1);
  int64_t wants[3] = {0, 0, 0};
  for (int s = 0; s < S; ++s) {
    pfmpe_init_plan& p = plan[s];
    p.items = init_items(M[s], B[s], hist_only);
    p.bucket = init_bucket(M[s]);
    p.lds_hist = (int64_t)B[s] * M[s] * 4 <= kInitLdsHistBytes ? 1 : 0;
    wants[p.bucket] += (p.items + kInitBlockThreads - 1) / kInitBlockThreads;
  }
  int32_t next[3] = {0, 0, 0};
  for (int s = 0; s < S; ++s) {
    pfmpe_init_plan& p = plan[s];
    const int64_t want = (p.items + kInitBlockThreads - 1) / kInitBlockThreads;
    int64_t get = want;
    if (wants[p.bucket] > cap)  // the product can pass 2^63 at 1024 blobs
      get = std::max<int64_t>((int64_t)((unsigned __int128)want * cap / wants[p.bucket]), want > 0 ? 1 : 0);
    p.first_block = next[p.bucket];
    p.blocks = (int32_t)get;
    next[p.bucket] += p.blocks;
  }
  for (int b = 0; b < 3; ++b) blocks_per_bucket[b] = next[b];
}

}  // namespace pfmpe_plan
