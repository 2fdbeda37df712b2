// pfmpe_roi.hip — ROI prediction: k_roi_multi and k_roi_multi_final, their launches and host epilogue, the entry
// points pfmpe_predict_roi_multi and pfmpe_predict_roi (a batch of one), and the host twin pfmpe_host_predict_roi.
#include "pf_batch.hpp"
#include "pf_state.hpp"
#include "pf_wave.hpp"
#include "pfmpe_ctx.hpp"

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
// grid (pf_batch.hpp), kBlock particles per block: a small cloud next to a large one launches its own block count only.
// Block and wave boundaries, partials and reduction are a stream's own: its bits do not depend on its neighbours.
constexpr int kRoiMaxStreams = 64;
static_assert(kRoiMaxStreams <= kBatchMaxStreams, "RoiBatch::first is read by batch_stream_of_block");
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
              "k_batch_stage copies 8-byte words");
template <typename T, typename SP>
__global__ __launch_bounds__(kBlock) void k_roi_multi(const RoiBatch* __restrict__ hd, const RoiDesc* __restrict__ descs,
                                                     double* __restrict__ part) {
  __shared__ double sh[4][kWaves];
  const int s = batch_stream_of_block(hd->first, hd->S, blockIdx.x);
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

using namespace pfmpe_impl;

namespace {
// project2d (PE:1017-1034) in double on the host: (K34 * T) * [X;1], then / z
void host_project(const double* K, const double* T12, const double* X, double* uv) {
  double Q[12];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = K[i * 3 + 0] * T12[0 * 4 + j];
      s = s + K[i * 3 + 1] * T12[1 * 4 + j];
      s = s + K[i * 3 + 2] * T12[2 * 4 + j];
      Q[i * 4 + j] = s;
    }
  double p[3];
  for (int i = 0; i < 3; ++i) {
    double s = Q[i * 4 + 0] * X[0];
    s = s + Q[i * 4 + 1] * X[1];
    s = s + Q[i * 4 + 2] * X[2];
    p[i] = s + Q[i * 4 + 3];
  }
  uv[0] = p[0] / p[2];
  uv[1] = p[1] / p[2];
}
// LEDDetector::distortPoints (led_detector.cpp:371-414) on cv::Point2f inputs, result back to float
void host_distort(const double* K, const double* D, float xin, float yin, float* xo, float* yo) {
  const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  const double k1 = D[0], k2 = D[1], p1 = D[2], p2 = D[3], k3 = D[4];
  const double x = ((double)xin - cx) / fx;
  const double y = ((double)yin - cy) / fy;
  const double r2 = x * x + y * y;
  double xc = x * (1. + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2);
  double yc = y * (1. + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2);
  xc = xc + (2. * p1 * x * y + p2 * (r2 + 2. * x * x));
  yc = yc + (p1 * (r2 + 2. * y * y) + 2. * p2 * x * y);
  *xo = (float)(xc * fx + cx);
  *yo = (float)(yc * fy + cy);
}
// The host end of every ROI entry point: bb = the particles' box {x_min, x_max, y_min, y_max} -> out.
void roi_epilogue(const double* K, const double* markers, int M, const pfmpe_roi_in* in, double* bb,
                  pfmpe_roi_out* out) {
  // + the markers at predicted_pose_ (PE:1049-1052)
  for (int m = 0; m < M; ++m) {
    double uv[2];
    host_project(K, in->predicted_pose, markers + 3 * m, uv);
    if (uv[0] < bb[0]) bb[0] = uv[0];
    if (uv[0] > bb[1]) bb[1] = uv[0];
    if (uv[1] < bb[2]) bb[2] = uv[1];
    if (uv[1] > bb[3]) bb[3] = uv[1];
  }
  std::memcpy(out->bbox, bb, 4 * sizeof(double));
  // determineROI (led_detector.cpp:317-368): corners as cv::Point2f, distorted, border, clamp, cv::Rect
  float x0f, y0f, x1f, y1f;
  host_distort(K, in->D, (float)bb[0], (float)bb[2], &x0f, &y0f);
  host_distort(K, in->D, (float)bb[1], (float)bb[3], &x1f, &y1f);
  const double W = in->image_w, H = in->image_h, b = in->border;
  const double x0 = std::max(0.0, std::min(W, (double)x0f - b));
  const double x1 = std::max(0.0, std::min(W, (double)x1f + b));
  const double y0 = std::max(0.0, std::min(H, (double)y0f - b));
  const double y1 = std::max(0.0, std::min(H, (double)y1f + b));
  if (x1 - x0 < 1 || y1 - y0 < 1) {
    out->x = 0;
    out->y = 0;
    out->width = in->image_w;
    out->height = in->image_h;
  } else {
    out->x = (int32_t)x0;
    out->y = (int32_t)y0;
    out->width = (int32_t)(x1 - x0);
    out->height = (int32_t)(y1 - y0);
  }
}
// the kernel arguments of one ROI request for a model of M markers; the particle set's fields are the caller's
RoiArgs roi_args(const pfmpe_roi_in* in, const double* K, const double* markers, int M) {
  RoiArgs ra{};
  std::memcpy(ra.cam, in->cam_move_inv, sizeof(ra.cam));
  std::memcpy(ra.predm, in->prediction, sizeof(ra.predm));
  std::memcpy(ra.K, K, sizeof(ra.K));
  std::memcpy(ra.markers, markers, (size_t)M * 3 * sizeof(double));
  ra.M = M;
  return ra;
}
// what one stream of an ROI call must satisfy: its context c and its request; the text begins with `at`, on `err`
int roi_check_stream(pfmpe_ctx* err, const pfmpe_ctx* c, const pfmpe_roi_in* in, const std::string& at) {
  if (!c->has_model || !c->has_prior) return fail(err, PFMPE_E_STATE, at + "set_model and set_prior first");
  if (in->image_w < 1 || in->image_h < 1) return fail(err, PFMPE_E_ARG, at + "bad image size");
  return PFMPE_OK;
}
// The ROIs of S checked streams, 1 <= S <= kRoiMaxStreams, on ctxs[0]'s stream: pfmpe_predict_roi_multi and, as a
// batch of one, pfmpe_predict_roi.  The errors it can raise itself begin with `who`.
int roi_run(pfmpe_ctx* const* ctxs, int S, const pfmpe_roi_in* in, pfmpe_roi_out* out, const std::string& who) {
  pfmpe_ctx* c0 = ctxs[0];
  int64_t total = 0;
  for (int s = 0; s < S; ++s) total += (ctxs[s]->N + kBlock - 1) / kBlock;
  if (total > INT32_MAX) return fail(c0, PFMPE_E_CAP, who + ": too many blocks in one batch");
  RET(set_device(c0));
  // the scratch before any member's ordering state changes: pinned image (head, descriptors, result boxes) once,
  // device image + partials grown on demand (nothing of an earlier batch is pending: the call is blocking)
  constexpr size_t kDescOff = (sizeof(RoiBatch) + 255) / 256 * 256;
  constexpr size_t kBoxOff = kDescOff + kRoiMaxStreams * sizeof(RoiDesc);
  RET(c0->h_roim.ensure(c0, kBoxOff + kRoiMaxStreams * 4 * sizeof(double)));
  const size_t need = kBoxOff + (size_t)total * 4 * sizeof(double);
  RET(c0->d_roim.grow(c0, need, kBoxOff + (need - kBoxOff) * 2));
  unsigned char* hd_img = c0->h_roim.dev();
  BatchMembers members(who.c_str(), S);  // (the callers' checks: no context twice)
  for (int s = 0; s < S; ++s) members.add(ctxs[s]);
  RET(members.order());
  RoiBatch* hd = (RoiBatch*)c0->h_roim.get();
  RoiDesc* descs = (RoiDesc*)(c0->h_roim.get() + kDescOff);
  std::memset(hd, 0, sizeof(*hd));
  hd->S = S;
  int32_t nb = 0;
  for (int s = 0; s < S; ++s) {
    const pfmpe_ctx* c = ctxs[s];
    RoiDesc& d = descs[s];
    d.a = roi_args(&in[s], c->K, c->markers, c->M);  // (c->markers is zero beyond M, as ra.markers is)
    std::memcpy(d.a.anchor, c->anchor[c->prior_idx], sizeof(d.a.anchor));
    d.a.N = c->N;
    d.a.ld = c->ld;
    d.a.owner = prior_owner_ptr(c);
    d.prior = c->d_state[c->prior_idx].get();
    hd->first[s] = nb;
    nb += (c->N + kBlock - 1) / kBlock;
  }
  hd->first[S] = nb;
  const int stage_words = (int)((kDescOff + (size_t)S * sizeof(RoiDesc)) / sizeof(uint64_t));
  const RoiBatch* dhd = (const RoiBatch*)c0->d_roim.get();
  const RoiDesc* ddescs = (const RoiDesc*)(c0->d_roim.get() + kDescOff);
  double* part = (double*)(c0->d_roim.get() + kBoxOff);
  const double* hbox = (const double*)(c0->h_roim.get() + kBoxOff);
  double* dbox = (double*)(hd_img + kBoxOff);
  RET(timed(c0, [&] {
    return launch(c0, PFMPE_K_ROI, [&] {
      hipLaunchKernelGGL((k_batch_stage<kBlock>), dim3(1), dim3(kBlock), 0, c0->stream, (const uint64_t*)hd_img,
                         (uint64_t*)c0->d_roim.get(), stage_words, (int*)nullptr, 0);
      visit_state(c0, [&](auto s) {
        hipLaunchKernelGGL((k_roi_multi<typename decltype(s)::T, typename decltype(s)::SP>), dim3(nb), dim3(kBlock), 0,
                           c0->stream, dhd, ddescs, part);
      });
      hipLaunchKernelGGL((k_roi_multi_final<double>), dim3(S), dim3(kBlock), 0, c0->stream, dhd, (const double*)part,
                         dbox);
    });
  }));
  RET(members.finish());
  for (int s = 0; s < S; ++s) {
    double bb[4];
    std::memcpy(bb, hbox + 4 * (size_t)s, sizeof(bb));
    roi_epilogue(ctxs[s]->K, ctxs[s]->markers, ctxs[s]->M, &in[s], bb, &out[s]);
  }
  return PFMPE_OK;
}
}  // namespace

extern "C" {

int pfmpe_predict_roi(pfmpe_ctx* c, const pfmpe_roi_in* in, pfmpe_roi_out* out) {
  if (!c) return PFMPE_E_ARG;
  if (!in || !out) return fail(c, PFMPE_E_ARG, "predict_roi: null in/out");
  RET(roi_check_stream(c, c, in, "predict_roi: "));
  return roi_run(&c, 1, in, out, "predict_roi");
}

int pfmpe_predict_roi_multi(pfmpe_ctx* const* ctxs, int S, const pfmpe_roi_in* in, pfmpe_roi_out* out) {
  if (!ctxs || S < 1 || !ctxs[0]) return PFMPE_E_ARG;
  pfmpe_ctx* c0 = ctxs[0];
  if (!in || !out) return fail(c0, PFMPE_E_ARG, "predict_roi_multi: null in/out");
  if (S > PFMPE_ROI_MAX_STREAMS)
    return fail(c0, PFMPE_E_CAP, "predict_roi_multi: S exceeds PFMPE_ROI_MAX_STREAMS");
  RET(check_members(
      ctxs, S, "predict_roi_multi", "device and state type", [](const pfmpe_ctx*) { return true; },
      [&](int s, const std::string& at) { return roi_check_stream(c0, ctxs[s], &in[s], at); }));
  return roi_run(ctxs, S, in, out, "predict_roi_multi");
}

int pfmpe_host_predict_roi(const double* markers_xyz, int M, const double* K, const double* poses, int64_t N,
                           const pfmpe_roi_in* in, pfmpe_roi_out* out) {
  if (!markers_xyz || !K || !in || !out || M < 1 || M > PFMPE_MAX_MARKERS || N < 0 || (N > 0 && !poses) ||
      in->image_w < 1 || in->image_h < 1)
    return PFMPE_E_ARG;
  RoiArgs ra = roi_args(in, K, markers_xyz, M);
  ra.N = 1;  // each pose row is a one-particle set: 12 planes of one element
  ra.ld = 1;
  double bb[4] = {INFINITY, 0.0, INFINITY, 0.0};
  for (int64_t n = 0; n < N; ++n) roi_particle_box<double, double>(ra, poses + 12 * n, 0, bb[0], bb[1], bb[2], bb[3]);
  roi_epilogue(ra.K, ra.markers, M, in, bb, out);
  return PFMPE_OK;
}

}  // extern "C"
