// pf_roi.hpp — ROI prediction (pfmpe_predict_roi, pfmpe_predict_roi_multi) and its host twin.
#pragma once
#include "pf_state.hpp"
#include "pf_wave.hpp"

namespace pfmpe {

// ---- ROI prediction (§8f next row 1): predictMarkerPositionsInImage (PE:1036-1053) projects every marker
// through camMoveInv * prior_j * predictionMatrix (Eigen left-to-right products) for all N particles of
// the current prior; LEDDetector::determineROI (led_detector.cpp:217-243) keeps x_min / y_min from +inf and
// x_max / y_max from 0 with strict comparisons (NaN positions never win).  fp64 throughout: the same
// arithmetic as the oracle, so the box is exact for every state type.  One partial per block, then one
// block reduces them.
struct RoiArgs {
  double cam[12], predm[12], K[9], markers[kMaxMarkers * 3], anchor[12];
  int32_t N, M;
  int64_t ld;
  const uint32_t* owner;  // a deferred prior's owner indices (FrameArgsT::owner), or null
};
// One particle's share of the box: prior particle n (stored row owner[n] of a deferred prior) through
// camMoveInv * prior_n * predictionMatrix, K * that, and the M projections folded into box = {x_min, x_max, y_min,
// y_max} with the reference's strict comparisons.  The one body of k_roi_multi and the host twin
// (pfmpe_host_predict_roi, which passes each caller-given pose as a one-particle set with ld = 1); host and device
// are built with -ffp-contract=off, so they round alike.
template <typename T, typename SP>
__host__ __device__ __forceinline__ void roi_particle_box(const RoiArgs& ra, const SP* __restrict__ prior, const int n,
                                                          double& xmin, double& xmax, double& ymin, double& ymax) {
  double A[12], X[12], P[12];
  const int r = ra.owner ? (int)ra.owner[n] : n;
#pragma unroll
  for (int q = 0; q < 12; ++q)
    A[q] = (double)StateIO<T, SP>::load(prior[plane_index<SP>(q, r, ra.ld)], (T)ra.anchor[q]);
  compose(ra.cam, A, X);   // camMoveInv * newPoseEstimation[j]
  compose(X, ra.predm, P); // ... * predictionMatrix
  double Q[12];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double s = ra.K[i * 3 + 0] * P[0 * 4 + j];
      s = s + ra.K[i * 3 + 1] * P[1 * 4 + j];
      s = s + ra.K[i * 3 + 2] * P[2 * 4 + j];
      Q[i * 4 + j] = s;
    }
  for (int m = 0; m < ra.M; ++m) {
    const double x = ra.markers[3 * m], y = ra.markers[3 * m + 1], z = ra.markers[3 * m + 2];
    double p[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double s = Q[i * 4 + 0] * x;
      s = s + Q[i * 4 + 1] * y;
      s = s + Q[i * 4 + 2] * z;
      p[i] = s + Q[i * 4 + 3];
    }
    const double u = p[0] / p[2], v = p[1] / p[2];
    if (u < xmin) xmin = u;
    if (u > xmax) xmax = u;
    if (v < ymin) ymin = v;
    if (v > ymax) ymax = v;
  }
}
// the lanes' boxes of one block -> o[0..3], written by thread 0
__device__ __forceinline__ void roi_block_box(double (&sh)[4][kWaves], double xmin, double xmax, double ymin,
                                              double ymax, double* __restrict__ o) {
  xmin = wave_min(xmin);
  xmax = wave_max(xmax);
  ymin = wave_min(ymin);
  ymax = wave_max(ymax);
  const int lane = lane_id(), wv = wave_id();
  if (lane == 0) {
    sh[0][wv] = xmin;
    sh[1][wv] = xmax;
    sh[2][wv] = ymin;
    sh[3][wv] = ymax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; ++w) {
      xmin = sh[0][w] < xmin ? sh[0][w] : xmin;
      xmax = sh[1][w] > xmax ? sh[1][w] : xmax;
      ymin = sh[2][w] < ymin ? sh[2][w] : ymin;
      ymax = sh[3][w] > ymax ? sh[3][w] : ymax;
    }
    o[0] = xmin;
    o[1] = xmax;
    o[2] = ymin;
    o[3] = ymax;
  }
}
// nblk block partials -> out[0..3], by one block (several passes of the strided loop when nblk > kBlock)
__device__ __forceinline__ void roi_partials_box(double (&sh)[4][kWaves], const double* __restrict__ part,
                                                 const int nblk, double* __restrict__ out) {
  double xmin = INFINITY, xmax = 0.0, ymin = INFINITY, ymax = 0.0;
  for (int b = threadIdx.x; b < nblk; b += kBlock) {
    const double* o = part + 4 * (size_t)b;
    xmin = o[0] < xmin ? o[0] : xmin;
    xmax = o[1] > xmax ? o[1] : xmax;
    ymin = o[2] < ymin ? o[2] : ymin;
    ymax = o[3] > ymax ? o[3] : ymax;
  }
  roi_block_box(sh, xmin, xmax, ymin, ymax, out);
}

// ---- the ROIs of S contexts in one batch (pfmpe_predict_roi_multi; pfmpe_predict_roi is a batch of one).  One flat
// grid: stream s owns the blocks first[s] .. first[s + 1] (kBlock particles each), so a small cloud next to a large
// one launches its own block count only.  A block finds its stream by one wave-wide comparison against the prefix
// (S <= 64 = the wave size: lane s holds first[s]); the index is wave-uniform, so the descriptor is read with scalar
// loads.  Block and wave boundaries, the partials and their reduction are a stream's own, so its bits do not depend
// on its neighbours.
constexpr int kRoiMaxStreams = 64;
static_assert(kRoiMaxStreams <= 64, "roi_stream_of_block compares one prefix entry per lane of a wave");
struct RoiBatch {  // head of the batch's device image, the descriptors follow
  int32_t S, pad;
  int32_t first[kRoiMaxStreams + 1];  // first block of stream s; first[S] = all blocks
  int32_t pad2;
};
struct RoiDesc {
  RoiArgs a;
  const void* prior;
};
static_assert(sizeof(RoiBatch) % sizeof(uint64_t) == 0 && sizeof(RoiDesc) % sizeof(uint64_t) == 0,
              "k_roi_stage copies 8-byte words");
__device__ __forceinline__ int roi_stream_of_block(const int32_t* __restrict__ first, const int S, const int b) {
  const int lane = threadIdx.x & 63;
  const bool le = lane < S && first[lane] <= b;  // first[0] = 0: at least one
  return __builtin_amdgcn_readfirstlane(__popcll(__ballot(le)) - 1);
}
// The batch's first launch: head and descriptors from the host's pinned image into device memory, so that the
// particle blocks read them from L2 and not over the host link.
template <typename W>
__global__ __launch_bounds__(kBlock) void k_roi_stage(const W* __restrict__ src, W* __restrict__ dst, const int nwords) {
  for (int i = threadIdx.x; i < nwords; i += kBlock) dst[i] = src[i];
}
template <typename T, typename SP>
__global__ __launch_bounds__(kBlock) void k_roi_multi(const RoiBatch* __restrict__ hd, const RoiDesc* __restrict__ descs,
                                                     double* __restrict__ part) {
  __shared__ double sh[4][kWaves];
  const int s = roi_stream_of_block(hd->first, hd->S, blockIdx.x);
  const RoiDesc& d = descs[s];
  const int n = ((int)blockIdx.x - hd->first[s]) * kBlock + threadIdx.x;
  double xmin = INFINITY, xmax = 0.0, ymin = INFINITY, ymax = 0.0;
  if (n < d.a.N) roi_particle_box<T, SP>(d.a, (const SP*)d.prior, n, xmin, xmax, ymin, ymax);
  roi_block_box(sh, xmin, xmax, ymin, ymax, part + 4 * (size_t)blockIdx.x);
}
// one block per stream: its partials -> box s of `out` (pinned, host-mapped: no copy back)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_roi_multi_final(const RoiBatch* __restrict__ hd, const T* __restrict__ part,
                                                           T* __restrict__ out) {
  __shared__ double sh[4][kWaves];
  const int s = blockIdx.x, b0 = hd->first[s];
  roi_partials_box(sh, part + 4 * (size_t)b0, hd->first[s + 1] - b0, out + 4 * (size_t)s);
}

}  // namespace pfmpe
