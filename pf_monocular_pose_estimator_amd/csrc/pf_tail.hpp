#pragma once
// pf_tail.hpp — the step's tail (pfmpe_step_refine / pfmpe_step_refine_multi): optimisePose of a finished frame's
// winner (PE:687-690) from the frame record itself.  What decides and what computes is __host__ __device__ code shared
// by the kernel (k_step_tail, pfmpe_refine.hip: one wave per stream behind the frame's finisher) and the host
// (pfmpe_host_step_tail); the record the wave publishes and the staging block it reads are laid out here.
#include "pf_gn.hpp"
#include "pf_types.hpp"

namespace pfmpe {

// What a tail leaves for its frame: the refinement, the empty summary (a rejected frame, a non-finite winner pose),
// or "not ready" (the frame record was not whole, an index out of range: the host takes the recovery path).
enum : uint32_t { kTailRefined = 1u, kTailEmpty = 2u, kTailNotReady = 3u };

// The tail record in mapped pinned memory, published like RecOut: data-tagged 8-byte granules {word k (low 32 bits),
// tag (high 32)}, tag = frame sequence << 2 | state (never 0).  Word 0 is the state again, words 1 .. 32 the
// pfmpe_refine_row, words 33 .. 104 the covariance; kTailEmpty / kTailNotReady publish granule 0 alone.
constexpr int kTailRowWords = (int)(sizeof(pfmpe_refine_row) / 4);
constexpr int kTailWords = 1 + kTailRowWords + 72;
constexpr int kTailGran = 128;
static_assert(kTailWords > 64 && kTailWords <= kTailGran, "two granules per lane at most");
struct TailRec {
  uint64_t g[kTailGran];
};
PFGN_HD uint32_t tail_tag(int32_t seq, uint32_t state) { return ((uint32_t)seq << 2) | state; }

// One stream of a call in the staging block (mapped pinned memory the host writes once per call, before the first
// launch): where its frame record and its tail record are, and the byte offsets within the block of its fp64 model
// (kMaxMarkers x 3 marker doubles, then the 9 of K) and of its 2 * B blob doubles.
struct TailDesc {
  const uint64_t* rec;  // the stream's RecOut granules (device address)
  uint64_t* out;        // its TailRec granules (device address)
  uint32_t model_off, blobs_off;
  int32_t seq0;         // the stream's frame sequence number when the call began
  int32_t M, B, max_iter, revert, pad;
  double converged;
};
static_assert(sizeof(TailDesc) == 56, "TailDesc layout");
constexpr size_t kTailModelBytes = (kMaxMarkers * 3 + 16) * sizeof(double);

// the frame is refined at all: accepted, and every word of the winner pose finite
PFGN_HD bool tail_wanted(const int32_t flag_fail, const double* pose) {
  bool fin = flag_fail == PFMPE_FLAG_ACCEPTED;
  for (int q = 0; q < 12; ++q) fin = fin && (pose[q] - pose[q] == 0.0);
  return fin;
}
// Row j of the frame's pair row for the compact blob list (slot j holds the blob row j names): the indices checked by
// pfmpe_refine_poses' rules (LED 1 .. M beside a blob, never above M; blob 0 .. B), lrow = (LED, j + 1) or (LED, 0).
PFGN_HD bool tail_pair(const uint32_t* corr, const int j, const int M, const int B, uint32_t* lrow) {
  const uint32_t led = corr[2 * j], blob = corr[2 * j + 1];
  lrow[0] = led;
  lrow[1] = blob != 0u ? (uint32_t)(j + 1) : 0u;
  return led <= (uint32_t)M && blob <= (uint32_t)B && (blob == 0u || led != 0u);
}
// Gauss-Newton of the winner over the compact list: the arithmetic of k_refine's lane (gn_optimise reads a blob's two
// doubles and never its index, so the compact list gives pfmpe_refine_poses' bits)
PFGN_HD void tail_refine(const double* markers, const double* K, const double* zb, const uint32_t* lcorr,
                         const int max_iter, const int revert, const double converged, const double* pose,
                         pfmpe_refine_row& row, double* cov36) {
  gn_optimise(markers, K, zb, lcorr, kMaxMarkers, max_iter, revert, converged, pose, row, cov36);
}

}  // namespace pfmpe
