// pfmpe_cloud.hip — the cloud statistics: k_cloud_multi, k_cloud_multi_final and k_cloud_assign (pf_modes.hpp) with their runner, and
// the entry points pfmpe_cloud_stats_multi, pfmpe_cloud_stats (a batch of one), pfmpe_cloud_modes (the statistics per
// hypothesis) and the host twins pfmpe_host_cloud_plan, pfmpe_host_cloud_assign and pfmpe_host_pose_twist.
#include "pf_batch.hpp"
#include "pf_modes.hpp"
#include "pf_state.hpp"
#include "pf_wave.hpp"
#include "pfmpe_ctx.hpp"

namespace pfmpe {

// ---- cloud statistics (pfmpe_cloud_stats; the definition is in include/pfmpe.h): weighted sums of the particles'
// twists about a reference pose.  fp64 throughout, for every state type.
// Twist xi = [upsilon; omega] of D = T * ref^-1 (left perturbation T = exp(xi) * ref), logarithmMap's order
// (PE:2228-2296).  The stored matrices are used as they are (no re-orthonormalisation).  1 - cos(phi) is formed as
// 2 sin^2(phi / 2): the same number without the cancellation at small phi.  A pose bit-equal to the reference has
// twist exactly 0 (R R^T of a stored R is the identity only up to rounding).  Shared by the kernel and the host
// helper (pfmpe_host_pose_twist), built with -ffp-contract=off on both sides.
__host__ __device__ inline void pose_twist(const double* T, const double* ref, double* xi) {
  bool same = true;
#pragma unroll
  for (int q = 0; q < 12; ++q) same = same && (T[q] == ref[q]);
  double DR[9], d[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {  // D_R = R_i R_r^T
      double s = T[i * 4 + 0] * ref[j * 4 + 0];
      s = s + T[i * 4 + 1] * ref[j * 4 + 1];
      s = s + T[i * 4 + 2] * ref[j * 4 + 2];
      DR[i * 3 + j] = s;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {  // d = t_i - D_R t_r
    double s = DR[i * 3 + 0] * ref[3];
    s = s + DR[i * 3 + 1] * ref[7];
    s = s + DR[i * 3 + 2] * ref[11];
    d[i] = T[i * 4 + 3] - s;
  }
  const double a0 = 0.5 * (DR[7] - DR[5]), a1 = 0.5 * (DR[2] - DR[6]), a2 = 0.5 * (DR[3] - DR[1]);
  const double s = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
  const double c = 0.5 * (((DR[0] + DR[4]) + DR[8]) - 1.0);
  const double phi = atan2(s, c);
  const double f = s > 1e-8 ? phi / s : 1.0 + (s * s) / 6.0;
  const double w0 = f * a0, w1 = f * a1, w2 = f * a2;
  const double sh = sin(0.5 * phi), p2 = phi * phi;
  const double k = phi >= 1e-4 ? (1.0 - (phi * sin(phi)) / (2.0 * ((2.0 * sh) * sh))) / p2 : 1.0 / 12.0 + p2 / 720.0;
  // upsilon = (I - 1/2 w^ + k w^ w^) d
  const double c10 = w1 * d[2] - w2 * d[1], c11 = w2 * d[0] - w0 * d[2], c12 = w0 * d[1] - w1 * d[0];
  const double c20 = w1 * c12 - w2 * c11, c21 = w2 * c10 - w0 * c12, c22 = w0 * c11 - w1 * c10;
  xi[0] = same ? 0.0 : (d[0] - 0.5 * c10) + k * c20;
  xi[1] = same ? 0.0 : (d[1] - 0.5 * c11) + k * c21;
  xi[2] = same ? 0.0 : (d[2] - 0.5 * c12) + k * c22;
  xi[3] = same ? 0.0 : w0;
  xi[4] = same ? 0.0 : w1;
  xi[5] = same ? 0.0 : w2;
}

// One partial row per block, kCloudWords doubles: sum w, sum w^2, sum w xi (6), the upper triangle of sum w xi xi^T
// (21, row by row), max |upsilon|^2 and max |omega|^2 over particles with w > 0, one unused word.
constexpr int kCloudWords = 32;
constexpr int kCloudSums = 29;
// (the grid, cloud_blocks, and the arguments of an entry, CloudArgs / CloudDesc / cloud_load: pf_modes.hpp)
// ---- the cloud statistics of S entries in one batch (pfmpe_cloud_stats_multi; pfmpe_cloud_stats is a batch of
// one).  One flat grid (pf_batch.hpp): entry s owns cloud_blocks(N_s) blocks, and inside its entry a block is block
// lb of nb: it starts at particle lb * kBlock and strides by nb * kBlock.
// Grid, stride, reductions and the tree over the partial rows are a function of the entry's N alone, so an entry's
// bits do not depend on its neighbours.
// Resident entry: the prior through StateIO / the owner indices, exactly the rows k_export writes, unit weights.
// Dense entry: N x 12 doubles with weights widened as k_weights_export widens them.  Each lane sums its particles
// in index order; one DPP reduction per wave after the stride loop; the block's waves are added in wave order
// through LDS.  No atomics, no waits on other blocks: k_cloud_multi_final is a second launch.
constexpr int kCloudMaxStreams = 64;
static_assert(kCloudMaxStreams <= kBatchMaxStreams, "CloudBatch::first is read by batch_stream_of_block");
struct CloudBatch {  // head of the batch's device image, the descriptors follow
  int32_t S, pad;
  int32_t first[kCloudMaxStreams + 1];  // first block of entry s; first[S] = all blocks
  int32_t pad2;
};
static_assert(sizeof(CloudBatch) % sizeof(uint64_t) == 0 && sizeof(CloudDesc) % sizeof(uint64_t) == 0,
              "k_batch_stage copies 8-byte words");
// kFiltered (pfmpe_cloud_modes): the entry's sums run over its mode's members alone, in the same order; a non-member
// costs its byte of mode_of and nothing else (no state load, no twist).  The unfiltered instances are the ones
// pfmpe_cloud_stats and pfmpe_cloud_stats_multi launch: no part of the test is compiled into them.
template <typename T, typename SP, bool kFiltered>
__global__ __launch_bounds__(kBlock) void k_cloud_multi(const CloudBatch* __restrict__ hd,
                                                       const CloudDesc* __restrict__ descs,
                                                       double* __restrict__ part) {
  __shared__ double sh[kWaves][kCloudWords];
  const int s = batch_stream_of_block(hd->first, hd->S, blockIdx.x);
  const CloudDesc& d = descs[s];
  const CloudArgs& ca = d.a;
  const int b0 = hd->first[s];
  const int lb = (int)blockIdx.x - b0, nb = hd->first[s + 1] - b0;
  const bool dense = d.dense != 0;  // wave-uniform
  const SP* __restrict__ st = (const SP*)d.st;
  double acc[kCloudSums];
#pragma unroll
  for (int q = 0; q < kCloudSums; ++q) acc[q] = 0.0;
  double mt = 0.0, mr = 0.0;
  const int64_t stride = (int64_t)nb * kBlock;  // the entry's own grid, not gridDim.x
  for (int64_t n = (int64_t)lb * kBlock + threadIdx.x; n < ca.N; n += stride) {
    if constexpr (kFiltered) {
      if ((int32_t)d.mode_of[n] != d.mode) continue;
    }
    double P[12], w = 1.0;
    cloud_load<T, SP>(ca, st, dense, n, P, w);
    double xi[6], wx[6];
    pose_twist(P, ca.ref, xi);
    acc[0] = acc[0] + w;
    acc[1] = acc[1] + w * w;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      wx[q] = w * xi[q];
      acc[2 + q] = acc[2 + q] + wx[q];
    }
    int k = 8;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j, ++k) acc[k] = acc[k] + wx[i] * xi[j];
    const double t2 = (xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2];
    const double r2 = (xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5];
    mt = (w > 0.0 && t2 > mt) ? t2 : mt;
    mr = (w > 0.0 && r2 > mr) ? r2 : mr;
  }
#pragma unroll
  for (int q = 0; q < kCloudSums; ++q) acc[q] = lane_value(wave_incl_sum(acc[q]), 63);
  mt = wave_max(mt);
  mr = wave_max(mr);
  const int wv = wave_id();
  if (lane_id() == 0) {
#pragma unroll
    for (int q = 0; q < kCloudSums; ++q) sh[wv][q] = acc[q];
    sh[wv][kCloudSums] = mt;
    sh[wv][kCloudSums + 1] = mr;
    sh[wv][kCloudSums + 2] = 0.0;
  }
  __syncthreads();
  if (threadIdx.x < kCloudWords) {
    const int q = threadIdx.x;
    double v = sh[0][q];
    for (int x = 1; x < kWaves; ++x) v = q < kCloudSums ? v + sh[x][q] : (sh[x][q] > v ? sh[x][q] : v);
    part[(size_t)blockIdx.x * kCloudWords + q] = v;  // row first[s] + lb
  }
}
// One block per entry: word q of its result = its partial rows' word q combined in block order -> the kCloudWords
// words of entry e of `out` (pinned, host-mapped: no copy back).  The rows are cut into kCloudSegs runs of
// consecutive rows; 32 lanes per run add its rows in index order (16 loads in flight: one lane walking all 1024 rows,
// a load's latency per row, took 50 us), then the runs are added in run order.  The tree depends on the entry's own
// block count alone.  (0 is the identity of the sums and of the maxima, which are of squares.)
constexpr int kCloudSegs = 8;
__global__ __launch_bounds__(kCloudSegs* kCloudWords) void k_cloud_multi_final(const CloudBatch* __restrict__ hd,
                                                                              const double* __restrict__ part,
                                                                              double* __restrict__ out) {
  __shared__ double sh[kCloudSegs][kCloudWords];
  const int e = blockIdx.x, r0 = hd->first[e], nblk = hd->first[e + 1] - r0;
  part += (size_t)r0 * kCloudWords;
  const int q = threadIdx.x % kCloudWords, sg = threadIdx.x / kCloudWords;
  const int per = (nblk + kCloudSegs - 1) / kCloudSegs;
  const int b0 = sg * per, b1 = b0 + per < nblk ? b0 + per : nblk;
  const bool sum = q < kCloudSums;
  double v = 0;
  int b = b0;
  for (; b + 16 <= b1; b += 16) {
    double x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = part[(size_t)(b + i) * kCloudWords + q];
#pragma unroll
    for (int i = 0; i < 16; ++i) v = sum ? v + x[i] : (x[i] > v ? x[i] : v);
  }
  for (; b < b1; ++b) {
    const double x = part[(size_t)b * kCloudWords + q];
    v = sum ? v + x : (x > v ? x : v);
  }
  sh[sg][q] = v;
  __syncthreads();
  if (sg == 0) {
    for (int s = 1; s < kCloudSegs; ++s) v = sum ? v + sh[s][q] : (sh[s][q] > v ? sh[s][q] : v);
    out[(size_t)e * kCloudWords + q] = v;
  }
}

// ---- the cloud's mass and statistics per hypothesis (pfmpe_cloud_modes; the definition is in include/pfmpe.h): every
// particle goes to its nearest seed, then the reduction above runs once per mode as a filtered entry.
// The assignment itself (ModeSeeds, mode_dist, mode_assign, k_cloud_assign) is in pf_modes.hpp: one definition, shared
// with pfmpe_resample_prior.

}  // namespace pfmpe

using namespace pfmpe_impl;

namespace {
// exponentialMap (PE:2194-2226): twist [upsilon; omega] -> pose
void host_exp_map(const double* xi, double* pose) {
  const double* u = xi;
  const double* w = xi + 3;
  const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), th2 = th * th;
  const double O[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  double O2[9], R[9], V[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) O2[i * 3 + j] = O[i * 3] * O[j] + O[i * 3 + 1] * O[3 + j] + O[i * 3 + 2] * O[6 + j];
  for (int i = 0; i < 9; ++i) {
    const double I = (i % 4 == 0) ? 1.0 : 0.0;
    R[i] = I;
    V[i] = I;
    if (th != 0) {
      const double s = std::sin(th), c = std::cos(th);
      R[i] = I + O[i] / th * s + O2[i] / th2 * (1 - c);
      V[i] = I + (1 - c) / th2 * O[i] + (th - s) / (th2 * th) * O2[i];
    }
  }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) pose[i * 4 + j] = R[i * 3 + j];
    pose[i * 4 + 3] = V[i * 3] * u[0] + V[i * 3 + 1] * u[1] + V[i * 3 + 2] * u[2];
  }
}
// the kernel arguments of one statistics request on context c: its kept propagated set regenerated into d_xfer with
// the kept iteration's raw weights (WEIGHTED), or its current prior (POSTERIOR)
CloudArgs cloud_args(const pfmpe_ctx* c, int which, const double* ref) {
  CloudArgs ca{};
  std::memcpy(ca.ref, ref, sizeof(ca.ref));
  ca.N = c->N;
  if (which == PFMPE_CLOUD_WEIGHTED) {
    ca.dense = c->d_xfer.get();
    ca.w = c->d_w[c->last_kept_slot].get();
  } else {
    std::memcpy(ca.anchor, c->anchor[c->prior_idx], sizeof(ca.anchor));
    ca.ld = c->ld;
    ca.owner = prior_owner_ptr(c);
  }
  return ca;
}
// the kCloudWords reduced words r of a set of N particles about ref -> pfmpe_cloud_out (pfmpe_cloud_stats and every
// entry of pfmpe_cloud_stats_multi)
void cloud_epilogue(const double* r, int N, const double* ref, pfmpe_cloud_out* out) {
  std::memset(out, 0, sizeof(*out));
  out->n = N;
  out->wsum = r[0];
  if (!(r[0] > 0.0)) {  // all weights zero (the re-initialisation branch): no mean to speak of
    out->degenerate = 1;
    std::memcpy(out->mean_pose, ref, sizeof(out->mean_pose));
    return;
  }
  const double W = r[0];
  out->ess = W * W / r[1];
  for (int q = 0; q < 6; ++q) out->mean_twist[q] = r[2 + q] / W;
  int k = 8;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j, ++k) {
      const double v = r[k] / W - out->mean_twist[i] * out->mean_twist[j];
      out->cov[i * 6 + j] = v;
      out->cov[j * 6 + i] = v;
    }
  out->max_trans = std::sqrt(r[kCloudSums]);
  out->max_rot = std::sqrt(r[kCloudSums + 1]);
  // mean_pose = exp(mu) * ref: one step toward the intrinsic mean
  double E[12];
  host_exp_map(out->mean_twist, E);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      out->mean_pose[i * 4 + j] = E[i * 4] * ref[j] + E[i * 4 + 1] * ref[4 + j] + E[i * 4 + 2] * ref[8 + j];
    out->mean_pose[i * 4 + 3] = E[i * 4] * ref[3] + E[i * 4 + 1] * ref[7] + E[i * 4 + 2] * ref[11] + E[i * 4 + 3];
  }
}
// pfmpe_cloud_modes' batch: its S = K + 1 entries are one set of one context, entry s < K about seed s and restricted
// to mode s, entry K about seed 0 and restricted to the particles without a mode.
struct CloudModesRun {
  ModeSeeds seeds;
  uint8_t* mode_of;  // the caller's N bytes, or null
};
static_assert(kModesMax + 1 <= kCloudMaxStreams, "the modes of a call are one batch");
// The statistics of S checked entries, 1 <= S <= kCloudMaxStreams, on ctxs[0]'s stream: pfmpe_cloud_stats_multi, as a
// batch of one pfmpe_cloud_stats and, with `modes`, pfmpe_cloud_modes (the assignment runs between the regeneration
// and the reduction, and every entry reduces its mode's members: the same launches otherwise).  The errors it can
// raise itself begin with `who`.
int cloud_run(pfmpe_ctx* const* ctxs, int S, const pfmpe_cloud_in* in, pfmpe_cloud_out* out, const std::string& who,
              const CloudModesRun* modes = nullptr) {
  pfmpe_ctx* c0 = ctxs[0];
  BatchMembers members(who.c_str(), S);  // flagged: a context with a WEIGHTED entry (all its entries read one regenerated set)
  int32_t Ns[PFMPE_CLOUD_MAX_STREAMS];
  for (int s = 0; s < S; ++s) {
    members.add(ctxs[s], in[s].which == PFMPE_CLOUD_WEIGHTED);
    Ns[s] = ctxs[s]->N;
  }
  pfmpe_cloud_plan plan[PFMPE_CLOUD_MAX_STREAMS];
  int32_t total = 0;
  if (pfmpe_host_cloud_plan(Ns, S, plan, &total) != PFMPE_OK)
    return fail(c0, PFMPE_E_STATE, who + ": a context without particles");
  RET(set_device(c0));
  // the scratch before any member's ordering state changes: pinned image (head, descriptors, result rows) once,
  // device image + partial rows grown on demand (nothing of an earlier batch is pending: the call is blocking)
  constexpr size_t kDescOff = (sizeof(CloudBatch) + 255) / 256 * 256;
  constexpr size_t kRowOff = (kDescOff + kCloudMaxStreams * sizeof(CloudDesc) + 255) / 256 * 256;
  constexpr size_t kRowBytes = kCloudWords * sizeof(double);
  RET(c0->h_cloudm.ensure(c0, kRowOff + kCloudMaxStreams * kRowBytes));
  const size_t need = kRowOff + (size_t)total * kRowBytes;
  RET(c0->d_cloudm.grow(c0, need, kRowOff + (need - kRowOff) * 2));
  if (modes) {
    RET(c0->h_modes.ensure(c0, kModesCountBytes));
    const size_t bytes = kModesCountBytes + (((size_t)c0->N + 3) & ~(size_t)3);
    RET(c0->d_modes.grow(c0, bytes, bytes));
  }
  RET(members.regen());
  RET(members.order());
  unsigned char* hd_img = c0->h_cloudm.dev();
  CloudBatch* hd = (CloudBatch*)c0->h_cloudm.get();
  CloudDesc* descs = (CloudDesc*)(c0->h_cloudm.get() + kDescOff);
  std::memset(hd, 0, sizeof(*hd));
  hd->S = S;
  for (int s = 0; s < S; ++s) {
    const pfmpe_ctx* c = ctxs[s];
    CloudDesc& d = descs[s];
    d.a = cloud_args(c, in[s].which, in[s].ref_pose);
    d.dense = in[s].which == PFMPE_CLOUD_WEIGHTED;
    d.st = d.dense ? nullptr : c->d_state[c->prior_idx].get();
    d.mode_of = modes ? c0->d_modes.get() + kModesCountBytes : nullptr;
    d.mode = s < S - 1 ? s : kModeNone;  // (read by a filtered entry only)
    hd->first[s] = plan[s].first_block;
  }
  hd->first[S] = total;
  const int stage_words = (int)((kDescOff + (size_t)S * sizeof(CloudDesc)) / sizeof(uint64_t));
  const CloudBatch* dhd = (const CloudBatch*)c0->d_cloudm.get();
  const CloudDesc* ddescs = (const CloudDesc*)(c0->d_cloudm.get() + kDescOff);
  double* part = (double*)(c0->d_cloudm.get() + kRowOff);
  const double* hrow = (const double*)(c0->h_cloudm.get() + kRowOff);
  hipLaunchKernelGGL((k_batch_stage<kBlock>), dim3(1), dim3(kBlock), 0, c0->stream, (const uint64_t*)hd_img,
                     (uint64_t*)c0->d_cloudm.get(), stage_words, (int*)nullptr, 0);
  uint32_t* d_count = (uint32_t*)c0->d_modes.get();
  if (modes) {  // every entry reads the same set: entry 0's descriptor names it
    HIPCHK(c0, hipMemsetAsync(d_count, 0, kModesCountBytes, c0->stream));
    visit_state(c0, [&](auto s) {
      hipLaunchKernelGGL((k_cloud_assign<typename decltype(s)::T, typename decltype(s)::SP>), dim3(cloud_blocks(c0->N)),
                         dim3(kBlock), 0, c0->stream, descs[0], modes->seeds, c0->d_modes.get() + kModesCountBytes,
                         d_count);
    });
  }
  visit_state(c0, [&](auto s) {
    using T = typename decltype(s)::T;
    using SP = typename decltype(s)::SP;
    const auto kernel = modes ? k_cloud_multi<T, SP, true> : k_cloud_multi<T, SP, false>;
    hipLaunchKernelGGL(kernel, dim3(total), dim3(kBlock), 0, c0->stream, dhd, ddescs, part);
  });
  hipLaunchKernelGGL(k_cloud_multi_final, dim3(S), dim3(kCloudSegs * kCloudWords), 0, c0->stream, dhd,
                     (const double*)part, (double*)(hd_img + kRowOff));
  HIPCHK(c0, hipGetLastError());
  if (modes) {
    HIPCHK(c0, hipMemcpyAsync(c0->h_modes.get(), d_count, (size_t)S * sizeof(uint32_t), hipMemcpyDeviceToHost, c0->stream));
    if (modes->mode_of)
      HIPCHK(c0, hipMemcpyAsync(modes->mode_of, c0->d_modes.get() + kModesCountBytes, (size_t)c0->N,
                                hipMemcpyDeviceToHost, c0->stream));
  }
  RET(members.finish());
  for (int s = 0; s < S; ++s) {
    double r[kCloudWords];
    std::memcpy(r, hrow + (size_t)kCloudWords * s, sizeof(r));
    const int64_t n = modes ? (int64_t)((const uint32_t*)c0->h_modes.get())[s] : (int64_t)ctxs[s]->N;
    cloud_epilogue(r, n, in[s].ref_pose, &out[s]);
  }
  return PFMPE_OK;
}
}  // namespace

extern "C" {

int pfmpe_host_cloud_plan(const int32_t* N, int S, pfmpe_cloud_plan* plan, int32_t* total_blocks) {
  if (!N || !plan || !total_blocks || S < 1) return PFMPE_E_ARG;
  if (S > PFMPE_CLOUD_MAX_STREAMS) return PFMPE_E_CAP;
  for (int s = 0; s < S; ++s)
    if (N[s] < 1) return PFMPE_E_ARG;
  int32_t nb = 0;  // at most 64 x 1024
  for (int s = 0; s < S; ++s) {
    plan[s].first_block = nb;
    // (cloud_blocks rounds N up in int: any N, not a context's only, comes through here)
    plan[s].blocks = N[s] >= kCloudMaxBlocks * kBlock ? kCloudMaxBlocks : cloud_blocks(N[s]);
    nb += plan[s].blocks;
  }
  *total_blocks = nb;
  return PFMPE_OK;
}

void pfmpe_default_modes_params(pfmpe_modes_params* p) {
  if (!p) return;
  p->trans_scale = 0.01;
  p->rot_scale = 0.05;
  p->max_dist = 0.0;
}

int pfmpe_cloud_modes(pfmpe_ctx* c, int which, const double* seeds, int K, const pfmpe_modes_params* params,
                      pfmpe_mode_out* out, uint8_t* mode_of) {
  static_assert(sizeof(pfmpe_modes_params) == 24 && sizeof(pfmpe_mode_out) == 488, "ABI");
  if (!c) return PFMPE_E_ARG;
  if (!seeds || !out || (which != PFMPE_CLOUD_WEIGHTED && which != PFMPE_CLOUD_POSTERIOR))
    return fail(c, PFMPE_E_ARG, "cloud_modes: bad arguments");
  pfmpe_modes_params prm;
  pfmpe_default_modes_params(&prm);
  if (params) prm = *params;
  if (const char* bad = modes_args_bad(seeds, K, prm)) return fail(c, PFMPE_E_ARG, std::string("cloud_modes: ") + bad);
  if (!c->has_prior) return fail(c, PFMPE_E_STATE, "cloud_modes: no particle set");
  if (which == PFMPE_CLOUD_WEIGHTED && !c->has_last) return fail(c, PFMPE_E_STATE, "cloud_modes(weighted): no step yet");
  CloudModesRun run{mode_seeds(seeds, K, prm), mode_of};
  pfmpe_ctx* ctxs[kModesMax + 1];
  pfmpe_cloud_in in[kModesMax + 1];
  pfmpe_cloud_out stats[kModesMax + 1];
  for (int s = 0; s <= K; ++s) {
    ctxs[s] = c;
    in[s] = pfmpe_cloud_in{};
    std::memcpy(in[s].ref_pose, seeds + 12 * (s < K ? s : 0), sizeof(in[s].ref_pose));
    in[s].which = which;
  }
  RET(cloud_run(ctxs, K + 1, in, stats, "cloud_modes", &run));
  double total = 0.0;
  for (int s = 0; s <= K; ++s) total = total + stats[s].wsum;
  for (int s = 0; s <= K; ++s) {
    out[s].stats = stats[s];
    out[s].share = total > 0.0 ? stats[s].wsum / total : 0.0;
  }
  return PFMPE_OK;
}

int pfmpe_host_cloud_assign(const double* poses, int64_t N, const double* seeds, int K, const pfmpe_modes_params* params,
                            uint8_t* mode_of, int64_t* counts) {
  if (!seeds || N < 0 || (N > 0 && (!poses || !mode_of))) return PFMPE_E_ARG;
  pfmpe_modes_params prm;
  pfmpe_default_modes_params(&prm);
  if (params) prm = *params;
  if (modes_args_bad(seeds, K, prm)) return PFMPE_E_ARG;
  const ModeSeeds ms = mode_seeds(seeds, K, prm);
  int64_t cnt[kModesMax + 1] = {0};
  for (int64_t n = 0; n < N; ++n) {
    const int mode = mode_assign(poses + 12 * n, ms);
    mode_of[n] = (uint8_t)mode;
    cnt[mode == kModeNone ? K : mode] += 1;
  }
  if (counts) std::memcpy(counts, cnt, (size_t)(K + 1) * sizeof(int64_t));
  return PFMPE_OK;
}

int pfmpe_cloud_stats(pfmpe_ctx* c, int which, const double* ref, pfmpe_cloud_out* out) {
  if (!c) return PFMPE_E_ARG;
  if (!ref || !out || (which != PFMPE_CLOUD_WEIGHTED && which != PFMPE_CLOUD_POSTERIOR))
    return fail(c, PFMPE_E_ARG, "cloud_stats: bad arguments");
  for (int q = 0; q < 12; ++q)
    if (!std::isfinite(ref[q])) return fail(c, PFMPE_E_ARG, "cloud_stats: non-finite reference pose");
  if (!c->has_prior) return fail(c, PFMPE_E_STATE, "cloud_stats: no particle set");
  if (which == PFMPE_CLOUD_WEIGHTED && !c->has_last) return fail(c, PFMPE_E_STATE, "cloud_stats(weighted): no step yet");
  pfmpe_cloud_in e{};
  std::memcpy(e.ref_pose, ref, sizeof(e.ref_pose));
  e.which = which;
  return cloud_run(&c, 1, &e, out, "cloud_stats");
}

int pfmpe_cloud_stats_multi(pfmpe_ctx* const* ctxs, int S, const pfmpe_cloud_in* in, pfmpe_cloud_out* out) {
  static_assert(PFMPE_CLOUD_MAX_STREAMS == kCloudMaxStreams, "stream capacity mismatch");
  if (!ctxs || S < 1 || !ctxs[0]) return PFMPE_E_ARG;
  pfmpe_ctx* c0 = ctxs[0];
  if (!in || !out) return fail(c0, PFMPE_E_ARG, "cloud_stats_multi: null in/out");
  if (S > PFMPE_CLOUD_MAX_STREAMS)
    return fail(c0, PFMPE_E_CAP, "cloud_stats_multi: S exceeds PFMPE_CLOUD_MAX_STREAMS");
  for (int s = 0; s < S; ++s) {
    const pfmpe_ctx* c = ctxs[s];
    const std::string at = "cloud_stats_multi: stream " + std::to_string(s) + ": ";
    if (!c) return fail(c0, PFMPE_E_ARG, at + "null context");
    if (c->device != c0->device || c->state_dtype != c0->state_dtype)
      return fail(c0, PFMPE_E_ARG, at + "device and state type must match ctxs[0]");
    const int which = in[s].which;
    if (which != PFMPE_CLOUD_WEIGHTED && which != PFMPE_CLOUD_POSTERIOR) return fail(c0, PFMPE_E_ARG, at + "bad which");
    for (int q = 0; q < 12; ++q)
      if (!std::isfinite(in[s].ref_pose[q])) return fail(c0, PFMPE_E_ARG, at + "non-finite reference pose");
    if (!c->has_prior) return fail(c0, PFMPE_E_STATE, at + "no particle set");
    if (which == PFMPE_CLOUD_WEIGHTED && !c->has_last) return fail(c0, PFMPE_E_STATE, at + "weighted: no step yet");
  }
  return cloud_run(ctxs, S, in, out, "cloud_stats_multi");
}

// the twist the cloud-statistics kernel forms for one particle
void pfmpe_host_pose_twist(const double* pose12, const double* ref_pose12, double* twist6) {
  pose_twist(pose12, ref_pose12, twist6);
}

}  // extern "C"
