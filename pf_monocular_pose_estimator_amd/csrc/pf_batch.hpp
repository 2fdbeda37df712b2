// pf_batch.hpp — the device side of the flat-batch idiom of the batch calls (ROI, cloud statistics, association,
// detector): the host writes the batch's head and descriptors into a pinned image, one staging launch copies them
// into device memory; the work kernels run one flat grid in which stream s owns the blocks first[s] .. first[s + 1].
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pfmpe {

constexpr int kBatchMaxStreams = 64;
// The stream that owns block b: how many of first[0 .. S) are <= b, less one (first[0] = 0).  One wave-wide comparison,
// lane s holding first[s], so S <= 64 (asserted by every user); wave-uniform: what it selects is read by scalar loads.
__device__ __forceinline__ int batch_stream_of_block(const int32_t* __restrict__ first, const int S, const int b) {
  const int lane = threadIdx.x & 63;
  const bool le = lane < S && first[lane] <= b;
  return __builtin_amdgcn_readfirstlane(__popcll(__ballot(le)) - 1);
}

// The batch's first launch, one block of kThreads: nwords 8-byte words of the pinned image into device memory (the
// work blocks then read them from L2, not over the host link) and nzero <= kThreads counters cleared (nullptr, 0:
// none).  In place of an async copy and a memset, which cost the detector's batch 20 us of wall time at R = 1.
template <int kThreads>
__global__ __launch_bounds__(kThreads) void k_batch_stage(const uint64_t* __restrict__ src, uint64_t* __restrict__ dst,
                                                          const int nwords, int* __restrict__ zero, const int nzero) {
  for (int i = threadIdx.x; i < nwords; i += kThreads) dst[i] = src[i];
  if ((int)threadIdx.x < nzero) zero[threadIdx.x] = 0;
}

}  // namespace pfmpe
