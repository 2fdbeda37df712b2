#pragma once
// pfmpe_refine_plan.hpp — the packed upload buffer of pfmpe_refine_multi, host C++ without device code: shared by the
// host-only entry point (pfmpe_refine_plan.cpp: pfmpe_host_refine_plan) and the device call (pfmpe_refine.hip), which
// stages exactly this plan and whose kernels read the descriptor defined here.
#include <cstdint>

#include "../../include/pfmpe.h"

namespace pfmpe_plan {

// A stream of the batch as the kernels read it: where its model and blobs are in the upload buffer, its range of
// hypotheses and its parameters.
struct RefineDesc {
  int64_t model_offset;  // markers (PFMPE_MAX_MARKERS x 3 doubles), then K (9)
  int64_t blobs_offset;  // 2 * B doubles
  int64_t first;         // index in the batch of the stream's first hypothesis
  int32_t count;         // its hypotheses
  int32_t max_iter;
  int32_t revert;
  int32_t pad;
  double converged;
};
static_assert(sizeof(RefineDesc) == PFMPE_REFINE_DESC_BYTES, "descriptor size of include/pfmpe.h");

constexpr int64_t kRefineModelDoubles = 3 * PFMPE_MAX_MARKERS + 9;
constexpr int64_t kRefineRowWords = 2 * PFMPE_MAX_MARKERS;

inline int64_t refine_align(int64_t x) { return (x + 15) / 16 * 16; }

// The layout for S streams of K[s] hypotheses and B[s] blobs (validated by the caller): descriptors, the stream of
// every hypothesis, start poses, pair rows, then every stream's model and blobs in ascending stream index; each
// region begins at a multiple of 16 bytes.  The device's results follow the upload: S summaries, H rows, H covariances.
inline void refine_plan(const int32_t* K, const int32_t* B, int S, pfmpe_refine_plan* plan,
                        pfmpe_refine_plan_total* total) {
  int64_t H = 0;
  for (int s = 0; s < S; ++s) {
    plan[s].first = H;
    H += K[s];
  }
  int64_t off = 0;
  auto take = [&off](int64_t bytes) {
    const int64_t at = off;
    off = refine_align(off + bytes);
    return at;
  };
  total->hypotheses = H;
  total->desc_offset = take((int64_t)S * (int64_t)sizeof(RefineDesc));
  total->stream_of_offset = take(H * 4);
  total->poses_offset = take(H * 12 * 8);
  total->corr_offset = take(H * kRefineRowWords * 4);
  for (int s = 0; s < S; ++s) {
    plan[s].model_offset = take(kRefineModelDoubles * 8);
    plan[s].blobs_offset = take((int64_t)(B[s] > 0 ? B[s] : 1) * 16);  // (B = 0: an offset inside the buffer)
  }
  total->upload_bytes = off;
  total->download_bytes = (int64_t)S * (int64_t)sizeof(pfmpe_refine_out) +
                          H * ((int64_t)sizeof(pfmpe_refine_row) + 36 * 8);
}

}  // namespace pfmpe_plan
