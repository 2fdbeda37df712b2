// pfmpe_refine.hip — Gauss-Newton refinement (optimisePose, PE:1805-2009; pf_gn.hpp) of one hypothesis per lane, fp64
// for every state type, and the call's summary: k_refine / k_refine_fold with pfmpe_refine_poses / pfmpe_refine_cloud,
// k_refine_multi / k_refine_fold_multi with pfmpe_refine_multi, pfmpe_host_optimise_pose, and k_step_tail with its
// launch (pfmpe_step_refine / pfmpe_step_refine_multi are with the step in pfmpe_engine.hip).  A TU of its own so it
// builds beside the others.
#include "pf_gn.hpp"
#include "pf_tail.hpp"
#include "pf_wave.hpp"
#include "pfmpe_ctx.hpp"
#include "pfmpe_refine_plan.hpp"

namespace pfmpe_impl {

// The scratch of pfmpe_refine_poses / pfmpe_refine_cloud (d_refine), one allocation: the call's summary, the model in
// fp64 (markers, K, the call's blobs), one partial per block, then the rows and covariances of one chunk of hypotheses.
// Hypotheses are refined a chunk at a time (the pair rows of a chunk are in d_pairs, kPairsChunk rows at most), so the
// scratch does not grow with the particle count.
constexpr int kRefineMaxBlocks = kPairsChunk / kBlock;
struct RefinePart {
  int64_t n_with, n_conv, n_kept, n_rev, it_total;
  int32_t it_max, best_np;
  double best_rms;
  int64_t best;  // index within the call, -1: none
};
struct RefineBuf {
  static constexpr size_t kOut = 0;
  static constexpr size_t kMarkers = 512;
  static constexpr size_t kK = kMarkers + kMaxMarkers * 3 * sizeof(double);
  static constexpr size_t kBlobs = kK + 16 * sizeof(double);
  static size_t part(int max_blobs) { return (kBlobs + (size_t)max_blobs * 2 * sizeof(double) + 255) / 256 * 256; }
  static size_t rows(int max_blobs) { return part(max_blobs) + kRefineMaxBlocks * sizeof(RefinePart); }
  static size_t cov(int max_blobs, int cap) { return rows(max_blobs) + (size_t)cap * sizeof(pfmpe_refine_row); }
  static size_t bytes(int max_blobs, int cap) { return cov(max_blobs, cap) + (size_t)cap * 36 * sizeof(double); }
};
static_assert(sizeof(pfmpe_refine_row) == 128 && sizeof(pfmpe_refine_out) <= RefineBuf::kMarkers, "refine layout");

// The batch (pfmpe_refine_multi): the leader's d_refm holds the packed upload of pfmpe_refine_plan.hpp (`up`), and
// behind it what the device writes: S summaries, H rows, H covariances, read back as one block.  All pointers are
// into d_refm.
using pfmpe_plan::RefineDesc;
struct RefineMultiArgs {
  const unsigned char* up;   // the upload: the descriptors' model_offset / blobs_offset count from here
  const RefineDesc* desc;    // S
  const int32_t* stream_of;  // H: the stream of hypothesis h
  const double* poses;       // H x 12
  const uint32_t* corr;      // H x 2 * kMaxMarkers
  pfmpe_refine_out* out;     // S
  pfmpe_refine_row* rows;    // H
  double* cov;               // H x 36
  int32_t H, pad;
};

namespace {
constexpr int kWave = 64;
struct RefineArgs {
  const double* poses;     // start poses of the chunk, 12 doubles each
  const uint32_t* corr;    // pair rows of the chunk, 2 * kMaxMarkers words each
  const double* markers;   // M x 3
  const double* K;         // 3 x 3
  const double* blobs;     // B x 2
  pfmpe_refine_row* rows;  // the chunk's rows
  double* cov;             // the chunk's covariances, 36 doubles each
  RefinePart* part;        // one partial per block
  int64_t base;            // index within the call of the chunk's first hypothesis
  int32_t count, max_iter, revert, pad;
  double converged;
};

__device__ inline void part_merge(RefinePart& a, const RefinePart& b) {
  a.n_with += b.n_with;
  a.n_conv += b.n_conv;
  a.n_kept += b.n_kept;
  a.n_rev += b.n_rev;
  a.it_total += b.it_total;
  a.it_max = b.it_max > a.it_max ? b.it_max : a.it_max;
  if (gn_better(b.best_np, b.best_rms, b.best, a.best_np, a.best_rms, a.best)) {
    a.best_np = b.best_np;
    a.best_rms = b.best_rms;
    a.best = b.best;
  }
}
// every lane gets the wave's merged partial (sums of integers and a total order: the tree's shape does not matter)
__device__ inline void part_wave_merge(RefinePart& p) {
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) {
    RefinePart o;
    o.n_with = __shfl_xor((long long)p.n_with, m);
    o.n_conv = __shfl_xor((long long)p.n_conv, m);
    o.n_kept = __shfl_xor((long long)p.n_kept, m);
    o.n_rev = __shfl_xor((long long)p.n_rev, m);
    o.it_total = __shfl_xor((long long)p.it_total, m);
    o.it_max = __shfl_xor(p.it_max, m);
    o.best_np = __shfl_xor(p.best_np, m);
    o.best_rms = __shfl_xor(p.best_rms, m);
    o.best = __shfl_xor((long long)p.best, m);
    part_merge(p, o);
  }
}
__device__ inline RefinePart part_zero() {
  RefinePart p;
  p.n_with = p.n_conv = p.n_kept = p.n_rev = p.it_total = 0;
  p.it_max = 0;
  p.best_np = 0;
  p.best_rms = 0.0;
  p.best = -1;
  return p;
}
// a lane's partial of one refined hypothesis, `index` within the call (or the stream)
__device__ inline RefinePart part_of_row(const pfmpe_refine_row& r, int64_t index) {
  RefinePart h = part_zero();
  h.n_with = r.n_pairs > 0 ? 1 : 0;
  h.n_conv = r.status == PFMPE_REFINE_CONVERGED ? 1 : 0;
  h.n_kept = r.status == PFMPE_REFINE_CAP_KEPT ? 1 : 0;
  h.n_rev = r.status == PFMPE_REFINE_CAP_REVERTED ? 1 : 0;
  h.it_total = r.iters;
  h.it_max = r.iters;
  if (gn_eligible(r)) {
    h.best_np = r.n_pairs;
    h.best_rms = r.rms_after;
    h.best = index;
  }
  return h;
}
// the nine summary fields of a call over n hypotheses (one lane)
__device__ inline void summary_store(pfmpe_refine_out* out, int64_t n, const RefinePart& p) {
  out->n = n;
  out->n_with_pairs = p.n_with;
  out->n_converged = p.n_conv;
  out->n_cap_kept = p.n_kept;
  out->n_cap_reverted = p.n_rev;
  out->iters_total = p.it_total;
  out->iters_max = p.it_max;
  out->pad = 0;
  out->best = p.best;
}
// the summary's best row and covariance, a word per lane of one wave: those of hypothesis i of rows / cov, or zeros
// (i < 0: none)
__device__ inline void best_copy(pfmpe_refine_out* out, const pfmpe_refine_row* rows, const double* cov, int64_t i) {
  constexpr int kRowWords = (int)(sizeof(pfmpe_refine_row) / sizeof(double));
  double* brow = (double*)&out->best_row;
  const int q = threadIdx.x;
  if (i >= 0) {
    if (q < kRowWords) brow[q] = ((const double*)(rows + i))[q];
    else if (q < kRowWords + 36) out->best_cov[q - kRowWords] = cov[36 * i + (q - kRowWords)];
  } else {
    if (q < kRowWords) brow[q] = 0.0;
    else if (q < kRowWords + 36) out->best_cov[q - kRowWords] = 0.0;
  }
}
static_assert(sizeof(pfmpe_refine_row) / sizeof(double) + 36 <= kWave, "best_copy copies a word per lane");

// One lane per hypothesis, grid-stride.  Lanes of a wave stop at different iterations: the wave runs as long as its
// slowest lane (no compaction).  The row and the covariance go to the chunk's buffers; the lane's counts and best key
// are merged per wave, then per block in wave order through LDS, into one partial per block.  No atomics, no waits
// on other blocks: k_refine_fold is a second launch.
__global__ __launch_bounds__(kBlock) void k_refine(const RefineArgs ra) {
  __shared__ RefinePart sh[kWaves];
  RefinePart acc = part_zero();
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < ra.count; i += stride) {
    pfmpe_refine_row r;
    gn_optimise(ra.markers, ra.K, ra.blobs, ra.corr + (size_t)i * (2 * kMaxMarkers), kMaxMarkers, ra.max_iter,
                ra.revert, ra.converged, ra.poses + 12 * (size_t)i, r, ra.cov + 36 * (size_t)i);
    ra.rows[i] = r;
    part_merge(acc, part_of_row(r, ra.base + i));
  }
  part_wave_merge(acc);
  if (lane_id() == 0) sh[wave_id()] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; ++w) part_merge(acc, sh[w]);
    ra.part[blockIdx.x] = acc;
  }
}

// One wave: the chunk's partials merged (lane l takes partials l, l + 64, ...), added to the call's summary, and the
// chunk's best row and covariance copied into it when they beat the summary's.
__global__ __launch_bounds__(kWave) void k_refine_fold(const RefinePart* __restrict__ part, int nblk,
                                                      const pfmpe_refine_row* __restrict__ rows,
                                                      const double* __restrict__ cov, int64_t base, int begin,
                                                      pfmpe_refine_out* __restrict__ out) {
  RefinePart p = part_zero();
  for (int b = threadIdx.x; b < nblk; b += kWave) part_merge(p, part[b]);
  part_wave_merge(p);
  // the summary so far, read by every lane before lane 0 rewrites it
  RefinePart s = part_zero();
  if (!begin) {
    s.n_with = out->n_with_pairs;
    s.n_conv = out->n_converged;
    s.n_kept = out->n_cap_kept;
    s.n_rev = out->n_cap_reverted;
    s.it_total = out->iters_total;
    s.it_max = out->iters_max;
    s.best = out->best;
    s.best_np = out->best_row.n_pairs;
    s.best_rms = out->best_row.rms_after;
  }
  const bool take = gn_better(p.best_np, p.best_rms, p.best, s.best_np, s.best_rms, s.best);
  part_merge(s, p);
  if (threadIdx.x == 0) summary_store(out, 0, s);  // (n: the host's)
  // a later chunk whose best does not beat the summary's leaves the row and the covariance as they are
  if (take) best_copy(out, rows, cov, p.best - base);
  else if (begin) best_copy(out, rows, cov, -1);
}

// One lane per hypothesis of all streams together, no grid stride (H <= kPairsChunk).
// Lane h looks up its stream and that stream's descriptor, so the model pointers and the parameters are per-lane values
// (a wave of the usual batch, one hypothesis per stream, holds 64 streams); the arithmetic is k_refine's, the same
// gn_optimise on the same numbers.  The summaries are k_refine_fold_multi's: nothing is reduced here.
__global__ __launch_bounds__(kBlock) void k_refine_multi(const RefineMultiArgs ma) {
  const int h = blockIdx.x * kBlock + threadIdx.x;
  if (h >= ma.H) return;
  const RefineDesc d = ma.desc[ma.stream_of[h]];
  const double* markers = (const double*)(ma.up + d.model_offset);
  pfmpe_refine_row r;
  gn_optimise(markers, markers + 3 * kMaxMarkers, (const double*)(ma.up + d.blobs_offset),
              ma.corr + (size_t)h * (2 * kMaxMarkers), kMaxMarkers, d.max_iter, d.revert, d.converged,
              ma.poses + 12 * (size_t)h, r, ma.cov + 36 * (size_t)h);
  ma.rows[h] = r;
}

// One wave per stream: lane l takes rows first + l, + 64, ... of its stream, forms k_refine's per-lane partial of each
// (best: the index within the stream), and the wave's merge is the stream's summary; then the best row and covariance
// are copied, or zeros, as k_refine_fold does for `begin`.  Sums of integers and a total order: the summary is the
// single call's whatever the shape of the reduction.
__global__ __launch_bounds__(kWave) void k_refine_fold_multi(const RefineMultiArgs ma) {
  const RefineDesc d = ma.desc[blockIdx.x];
  const pfmpe_refine_row* rows = ma.rows + d.first;
  const double* cov = ma.cov + 36 * d.first;
  pfmpe_refine_out* out = ma.out + blockIdx.x;
  RefinePart p = part_zero();
  for (int i = threadIdx.x; i < d.count; i += kWave) part_merge(p, part_of_row(rows[i], i));
  part_wave_merge(p);
  if (threadIdx.x == 0) summary_store(out, d.count, p);
  best_copy(out, rows, cov, p.best);
}

// ---- the step's tail (pfmpe_step_refine / pfmpe_step_refine_multi, pf_tail.hpp)
typedef __attribute__((address_space(1))) uint64_t tail_gu64_t;
__device__ __forceinline__ void tail_st_sys64(uint64_t* p, uint64_t v) {
  __hip_atomic_store((tail_gu64_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ uint64_t tail_ld_sys64(const uint64_t* p) {
  return __hip_atomic_load((tail_gu64_t*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// One wave per stream, launched behind every launch that can finish a frame.  The wave takes its stream's frame
// record where the finishing wave left it (the mapped pinned RecOut), and only if every granule carries this frame's
// finished tag (sequence seq0 + delta) goes on: an unfinished iteration round, another frame's record (an orphaned
// tail, a stream of a batch that finished in an earlier round) leave nothing.  The winner pose and the pair row come
// out of the record, the fp64 model and the blobs the row names out of the staging block, all into LDS, once; then lane
// 0 runs k_refine's gn_optimise on LDS alone and the wave publishes the row and the covariance as tagged granules.
// No wait, no atomic read-modify-write, no loop but Gauss-Newton's own (max_iter <= 10000): stream order is the only
// synchronisation.  miss: kDiagTailMiss, every finished frame is reported "not ready".
__global__ __launch_bounds__(kWave) void k_step_tail(const TailDesc* __restrict__ desc,
                                                     const unsigned char* __restrict__ block, const int32_t delta,
                                                     const int32_t miss) {
  __shared__ __attribute__((aligned(16))) uint32_t s_rec[2 * kWave];  // the OutDev words
  __shared__ double s_model[kMaxMarkers * 3 + 16];
  __shared__ double s_zb[2 * kMaxMarkers];
  __shared__ uint32_t s_corr[2 * kMaxMarkers];
  __shared__ pfmpe_refine_row s_row;
  __shared__ double s_cov[36];
  static_assert(kRecWords <= 2 * kWave && kTailWords <= 2 * kWave, "two words per lane");
  const int lane = threadIdx.x;
  const TailDesc d = desc[blockIdx.x];
  const int32_t seq = (d.seq0 + delta) & 0x3fffffff;
  const uint32_t fin = ((uint32_t)seq << 1) | 1u;
  const uint64_t g0 = tail_ld_sys64(d.rec + lane);
  const uint64_t g1 = lane + kWave < kRecWords ? tail_ld_sys64(d.rec + lane + kWave) : ((uint64_t)fin << 32);
  const uint32_t t0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(g0 >> 32));
  if (t0 != fin) return;  // not this frame's, or unfinished
  const bool stale = (uint32_t)(g0 >> 32) != fin || (uint32_t)(g1 >> 32) != fin;
  const bool torn = __builtin_amdgcn_ballot_w64(stale) != 0ull;
  s_rec[lane] = (uint32_t)g0;
  s_rec[lane + kWave] = (uint32_t)g1;
  wave_lds_sync();
  const OutDev& rec = *(const OutDev*)s_rec;
  uint32_t state = kTailRefined;
  if (torn || miss) {
    state = kTailNotReady;
  } else if (!tail_wanted(rec.flag_fail, rec.winner_pose)) {
    state = kTailEmpty;
  } else {
    // the model (a double per lane) and the blobs the pair row names (a row per lane), straight into LDS
    const double* model = (const double*)(block + d.model_off);
    const double* blobs = (const double*)(block + d.blobs_off);
    if (lane < kMaxMarkers * 3 + 9) s_model[lane] = model[lane];
    bool bad = false;
    if (lane < kMaxMarkers) {
      uint32_t lrow[2];
      bad = !tail_pair(rec.corr, lane, d.M, d.B, lrow);
      const bool used = !bad && lrow[1] != 0u;
      const size_t b = used ? (size_t)(rec.corr[2 * lane + 1] - 1u) : 0;
      s_zb[2 * lane] = used ? blobs[2 * b] : 0.0;
      s_zb[2 * lane + 1] = used ? blobs[2 * b + 1] : 0.0;
      s_corr[2 * lane] = lrow[0];
      s_corr[2 * lane + 1] = lrow[1];
    }
    if (__builtin_amdgcn_ballot_w64(bad) != 0ull) state = kTailNotReady;  // (the host path reports the index)
  }
  wave_lds_sync();
  const uint64_t th = (uint64_t)tail_tag(seq, state) << 32;
  if (state != kTailRefined) {
    if (lane == 0) tail_st_sys64(d.out, th | state);
    return;
  }
  if (lane == 0) {
    pfmpe_refine_row r;
    tail_refine(s_model, s_model + kMaxMarkers * 3, s_zb, s_corr, d.max_iter, d.revert, d.converged, rec.winner_pose, r,
                s_cov);
    s_row = r;
  }
  wave_lds_sync();
  // word k of the record: the state, the row's words, the covariance's
  const uint32_t* rw = (const uint32_t*)&s_row;
  const uint32_t* cw = (const uint32_t*)s_cov;
  const int k1 = lane + kWave;
  tail_st_sys64(d.out + lane, th | (lane == 0 ? state : (lane <= kTailRowWords ? rw[lane - 1] : cw[lane - 1 - kTailRowWords])));
  if (k1 < kTailWords) tail_st_sys64(d.out + k1, th | cw[k1 - 1 - kTailRowWords]);
}
}  // namespace

int tail_launch(pfmpe_ctx* c, int32_t delta) {
  return launch_ext(c, PFMPE_K_AUX, [&] {
    klaunch(c, k_step_tail, dim3((unsigned)c->tail_S), dim3(kWave), 0, (const TailDesc*)c->h_tail.dev(),
            (const unsigned char*)c->h_tail.dev(), delta, (c->diag & kDiagTailMiss) ? 1 : 0);
  });
}

namespace {
// k_refine_multi over the H hypotheses (skipped when H = 0), then k_refine_fold_multi, one wave per stream, on the
// leader's stream.
int refine_multi_launch(pfmpe_ctx* c0, const RefineMultiArgs& ma, int S) {
  const int nblk = (ma.H + kBlock - 1) / kBlock;
  if (nblk > 0) hipLaunchKernelGGL(k_refine_multi, dim3(nblk), dim3(kBlock), 0, c0->stream, ma);
  hipLaunchKernelGGL(k_refine_fold_multi, dim3(S), dim3(kWave), 0, c0->stream, ma);
  HIPCHK(c0, hipGetLastError());
  return PFMPE_OK;
}

// One chunk: k_refine over `count` hypotheses (start poses at poses + 12 * i, rows at corr + 2 * kMaxMarkers * i,
// i = 0 .. count - 1; index within the call base + i), then k_refine_fold of its partials into the summary at
// d_refine (begun anew when `begin`).  d_refine holds the model and the blobs already.
int refine_launch(pfmpe_ctx* c, const pfmpe_refine_params& prm, const double* poses, const uint32_t* corr, int64_t base,
                  int count, int cap, bool begin) {
  unsigned char* d = c->d_refine.get();
  RefineArgs ra{};
  ra.poses = poses;
  ra.corr = corr;
  ra.markers = (const double*)(d + RefineBuf::kMarkers);
  ra.K = (const double*)(d + RefineBuf::kK);
  ra.blobs = (const double*)(d + RefineBuf::kBlobs);
  ra.rows = (pfmpe_refine_row*)(d + RefineBuf::rows(c->max_blobs));
  ra.cov = (double*)(d + RefineBuf::cov(c->max_blobs, cap));
  ra.part = (RefinePart*)(d + RefineBuf::part(c->max_blobs));
  ra.base = base;
  ra.count = count;
  ra.max_iter = prm.max_iter;
  ra.revert = prm.revert_on_divergence ? 1 : 0;
  ra.converged = prm.converged;
  int nblk = (count + kBlock - 1) / kBlock;
  nblk = nblk < kRefineMaxBlocks ? nblk : kRefineMaxBlocks;
  if (nblk > 0) hipLaunchKernelGGL(k_refine, dim3(nblk), dim3(kBlock), 0, c->stream, ra);
  hipLaunchKernelGGL(k_refine_fold, dim3(1), dim3(kWave), 0, c->stream, (const RefinePart*)ra.part, nblk,
                     (const pfmpe_refine_row*)ra.rows, (const double*)ra.cov, base, begin ? 1 : 0,
                     (pfmpe_refine_out*)(d + RefineBuf::kOut));
  HIPCHK(c, hipGetLastError());
  return PFMPE_OK;
}

// the rows' indices: LED 1 .. M beside a blob, never above M; blob 0 .. B
bool refine_corr_ok(const uint32_t* corr, size_t n_rows, int M, int B) {
  for (size_t j = 0; j < n_rows; ++j) {
    const uint32_t led = corr[2 * j], blob = corr[2 * j + 1];
    if (led > (uint32_t)M || blob > (uint32_t)B || (blob != 0u && led == 0u)) return false;
  }
  return true;
}
bool refine_poses_finite(const double* poses, size_t n) {
  for (size_t q = 0; q < 12 * n; ++q)
    if (!std::isfinite(poses[q])) return false;
  return true;
}

// the scratch, the model and the call's blobs in fp64 (enqueued on the stream; `stage` must outlive the copy)
int refine_stage(pfmpe_ctx* c, const double* blobs, int B, int cap, std::vector<double>& stage) {
  RET(c->d_refine.ensure(c, RefineBuf::bytes(c->max_blobs, cap)));
  const size_t words = (RefineBuf::kBlobs - RefineBuf::kMarkers) / sizeof(double) + 2 * (size_t)B;
  stage.assign(words, 0.0);
  std::memcpy(stage.data(), c->markers, sizeof(c->markers));
  std::memcpy(stage.data() + (RefineBuf::kK - RefineBuf::kMarkers) / sizeof(double), c->K, sizeof(c->K));
  if (B > 0) std::memcpy(stage.data() + (RefineBuf::kBlobs - RefineBuf::kMarkers) / sizeof(double), blobs, 2 * (size_t)B * sizeof(double));
  HIPCHK(c, hipMemcpyAsync(c->d_refine.get() + RefineBuf::kMarkers, stage.data(), words * sizeof(double), hipMemcpyHostToDevice,
                           c->stream));
  return PFMPE_OK;
}
// a chunk's rows and covariances, hypotheses lo .. hi - 1 of the chunk, to the caller's arrays at index `at`
int refine_fetch(pfmpe_ctx* c, int cap, int lo, int hi, pfmpe_refine_row* rows, double* cov, int64_t at) {
  if (hi <= lo) return PFMPE_OK;
  const unsigned char* d = c->d_refine.get();
  if (rows)
    HIPCHK(c, hipMemcpyAsync(rows + at, d + RefineBuf::rows(c->max_blobs) + (size_t)lo * sizeof(pfmpe_refine_row),
                             (size_t)(hi - lo) * sizeof(pfmpe_refine_row), hipMemcpyDeviceToHost, c->stream));
  if (cov)
    HIPCHK(c, hipMemcpyAsync(cov + 36 * at, d + RefineBuf::cov(c->max_blobs, cap) + (size_t)lo * 36 * sizeof(double),
                             (size_t)(hi - lo) * 36 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  return PFMPE_OK;
}
int refine_finish(pfmpe_ctx* c, int64_t n, pfmpe_refine_out* out) {
  HIPCHK(c, hipMemcpyAsync(out, c->d_refine.get() + RefineBuf::kOut, sizeof(*out), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  RET(harvest_timing(c));  // (a propagated call's regeneration is bracketed like the particle read-back's)
  out->n = n;
  return PFMPE_OK;
}
}  // namespace

}  // namespace pfmpe_impl

// ======================================================================================= C-ABI
using namespace pfmpe_impl;

void pfmpe_default_refine_params(pfmpe_refine_params* p) {
  if (!p) return;
  p->max_iter = 500;
  p->revert_on_divergence = 1;
  p->converged = 1e-13;
}

int pfmpe_refine_poses(pfmpe_ctx* c, const pfmpe_assoc_in* in, const pfmpe_refine_params* params, const double* poses,
                       const uint32_t* corr, int32_t K, pfmpe_refine_out* out, pfmpe_refine_row* rows, double* cov) {
  if (!c) return PFMPE_E_ARG;
  pfmpe_refine_params prm;
  pfmpe_default_refine_params(&prm);
  if (params) prm = *params;
  if (!out || !in || K < 0 || (K > 0 && (!poses || !corr))) return fail(c, PFMPE_E_ARG, "refine_poses: bad arguments");
  if (!refine_params_ok(prm)) return fail(c, PFMPE_E_ARG, "refine_poses: bad parameters");
  const double* blobs = nullptr;
  int B = 0;
  RET(resolve_blobs(c, "refine_poses", in, &blobs, &B));
  if (K > c->max_particles) return fail(c, PFMPE_E_CAP, "refine_poses: K exceeds max_particles");
  if (!c->has_model) return fail(c, PFMPE_E_STATE, "refine_poses: set_model first");
  if (K > 0 && !refine_corr_ok(corr, (size_t)K * kMaxMarkers, c->M, B))
    return fail(c, PFMPE_E_ARG, "refine_poses: LED or blob index out of range");
  if (K > 0 && !refine_poses_finite(poses, (size_t)K)) return fail(c, PFMPE_E_ARG, "refine_poses: non-finite start pose");
  RET(set_device(c));
  RET(ensure_xfer(c));
  constexpr size_t kRow = kPairRow;
  const int cap = pairs_cap(c);
  RET(ensure_pairs(c));
  std::vector<double> stage;
  RET(refine_stage(c, blobs, B, cap, stage));
  // d_xfer is written and read inside one blocking call by every user
  if (K > 0) HIPCHK(c, hipMemcpyAsync(c->d_xfer.get(), poses, (size_t)K * 12 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  int64_t done = 0;
  do {  // (K = 0: one empty chunk writes the empty summary)
    const int n = (int)std::min<int64_t>(cap, (int64_t)K - done);
    if (n > 0)
      HIPCHK(c, hipMemcpyAsync(c->d_pairs.get(), corr + (size_t)done * kRow, (size_t)n * kRow * sizeof(uint32_t),
                               hipMemcpyHostToDevice, c->stream));
    RET(refine_launch(c, prm, c->d_xfer.get() + 12 * done, c->d_pairs.get(), done, n, cap, done == 0));
    RET(refine_fetch(c, cap, 0, n, rows, cov, done));
    done += n;
  } while (done < K);
  return refine_finish(c, K, out);
}

int pfmpe_refine_cloud(pfmpe_ctx* c, int which, const pfmpe_assoc_in* in, const pfmpe_refine_params* params,
                       int64_t first, int32_t count, pfmpe_refine_out* out, pfmpe_refine_row* rows, double* cov) {
  if (!c) return PFMPE_E_ARG;
  pfmpe_refine_params prm;
  pfmpe_default_refine_params(&prm);
  if (params) prm = *params;
  if (!out || first < 0 || count < 0) return fail(c, PFMPE_E_ARG, "refine_cloud: null out or bad range");
  if (c->has_prior && first + (int64_t)count > (int64_t)c->N)
    return fail(c, PFMPE_E_ARG, "refine_cloud: first + count exceeds the particle count");
  if (!refine_params_ok(prm)) return fail(c, PFMPE_E_ARG, "refine_cloud: bad parameters");
  const double* blobs = nullptr;
  int B = 0;
  size_t tbytes = 0;
  GridHdr gh{};
  AssocArgs aa{};
  RET(assoc_prepare(c, "refine_cloud", which, in, &blobs, &B, &tbytes, &gh, &aa));
  const int N = c->N;
  // the start poses as get_particles delivers them: the propagated set is in d_xfer already (assoc_prepare)
  if (which == PFMPE_ASSOC_POSTERIOR) {
    RET(ensure_xfer(c));
    RET(export_prior(c, N));
  }
  constexpr size_t kRow = kPairRow;
  const int cap = pairs_cap(c);
  RET(ensure_pairs(c));
  std::vector<double> stage;
  RET(refine_stage(c, blobs, B, cap, stage));
  aa.corr = c->d_pairs.get();
  aa.n_corr = (int32_t*)(c->d_pairs.get() + (size_t)cap * kRow);
  for (int64_t done = 0; done < N; done += cap) {
    const int n = (int)std::min<int64_t>(cap, (int64_t)N - done);
    aa.first = (int32_t)done;
    aa.count = n;
    RET(assoc_rows_launch(c, B, c->d_table.get(), tbytes, gh, aa));
    RET(refine_launch(c, prm, c->d_xfer.get() + 12 * done, c->d_pairs.get(), done, n, cap, done == 0));
    const int64_t lo = std::max<int64_t>(first, done), hi = std::min<int64_t>(first + count, done + n);
    RET(refine_fetch(c, cap, (int)(lo - done), (int)(hi - done), rows, cov, lo - first));
  }
  return refine_finish(c, N, out);
}

// pfmpe_refine_poses of S streams as one batch on ctxs[0]'s stream: the per-stream checks of the single call, the
// upload of pfmpe_refine_plan.hpp built in the leader's pinned block, one copy up, two launches, one copy down, one
// synchronise, and the results scattered to the caller's arrays.
int pfmpe_refine_multi(pfmpe_ctx* const* ctxs, int S, const pfmpe_refine_in* in, const pfmpe_refine_params* params,
                       pfmpe_refine_out* out, pfmpe_refine_row* const* rows, double* const* cov) {
  if (!ctxs || S < 1 || !ctxs[0]) return PFMPE_E_ARG;
  pfmpe_ctx* c0 = ctxs[0];
  if (!in || !out) return fail(c0, PFMPE_E_ARG, "refine_multi: null in/out");
  if (S > PFMPE_REFINE_MAX_STREAMS) return fail(c0, PFMPE_E_CAP, "refine_multi: S exceeds PFMPE_REFINE_MAX_STREAMS");
  struct Stream {
    const double* blobs;
    int B;
    pfmpe_refine_params prm;
  };
  std::vector<Stream> st(S);
  int32_t Ks[PFMPE_REFINE_MAX_STREAMS], Bs[PFMPE_REFINE_MAX_STREAMS];
  int64_t H = 0;
  for (int s = 0; s < S; ++s) {
    const pfmpe_ctx* c = ctxs[s];
    const pfmpe_refine_in& q = in[s];
    const std::string at = "refine_multi: stream " + std::to_string(s) + ": ";
    if (!c) return fail(c0, PFMPE_E_ARG, at + "null context");
    if (c->device != c0->device) return fail(c0, PFMPE_E_ARG, at + "device must match ctxs[0]");
    pfmpe_default_refine_params(&st[s].prm);
    if (params) st[s].prm = params[s];
    if (q.K < 0 || (q.K > 0 && (!q.poses || !q.corr))) return fail(c0, PFMPE_E_ARG, at + "bad arguments");
    if (!refine_params_ok(st[s].prm)) return fail(c0, PFMPE_E_ARG, at + "bad parameters");
    RET(resolve_blobs(c, at + "blobs", &q.blobs, &st[s].blobs, &st[s].B, c0));
    if (q.K > c->max_particles) return fail(c0, PFMPE_E_CAP, at + "K exceeds max_particles");
    if (!c->has_model) return fail(c0, PFMPE_E_STATE, at + "set_model first");
    if (q.K > 0 && !refine_corr_ok(q.corr, (size_t)q.K * kMaxMarkers, c->M, st[s].B))
      return fail(c0, PFMPE_E_ARG, at + "LED or blob index out of range");
    if (q.K > 0 && !refine_poses_finite(q.poses, (size_t)q.K)) return fail(c0, PFMPE_E_ARG, at + "non-finite start pose");
    Ks[s] = q.K;
    Bs[s] = st[s].B;
    H += q.K;
    if (H > PFMPE_REFINE_MULTI_MAX_HYPOTHESES)
      return fail(c0, PFMPE_E_CAP, at + "the batch exceeds PFMPE_REFINE_MULTI_MAX_HYPOTHESES hypotheses");
  }
  static_assert(PFMPE_REFINE_MULTI_MAX_HYPOTHESES <= kPairsChunk, "one launch without a grid stride");
  pfmpe_refine_plan plan[PFMPE_REFINE_MAX_STREAMS];
  pfmpe_refine_plan_total tot;
  pfmpe_plan::refine_plan(Ks, Bs, S, plan, &tot);
  RET(set_device(c0));
  // the device block: the upload, then summaries, rows and covariances; the pinned block mirrors it
  const size_t up = (size_t)tot.upload_bytes, down = (size_t)tot.download_bytes, all = up + down;
  RET(c0->d_refm.grow(c0, all, all + all / 2));
  RET(c0->h_refm.grow(c0, all, all + all / 2));
  unsigned char* h = c0->h_refm.get();
  unsigned char* d = c0->d_refm.get();
  std::memset(h, 0, up);  // the gaps between regions and unused marker slots: the same bytes for the same plan
  RefineDesc* ds = (RefineDesc*)(h + tot.desc_offset);
  int32_t* stream_of = (int32_t*)(h + tot.stream_of_offset);
  for (int s = 0; s < S; ++s) {
    const pfmpe_ctx* c = ctxs[s];
    const size_t K = (size_t)Ks[s], first = (size_t)plan[s].first;
    ds[s].model_offset = plan[s].model_offset;
    ds[s].blobs_offset = plan[s].blobs_offset;
    ds[s].first = plan[s].first;
    ds[s].count = Ks[s];
    ds[s].max_iter = st[s].prm.max_iter;
    ds[s].revert = st[s].prm.revert_on_divergence ? 1 : 0;
    ds[s].converged = st[s].prm.converged;
    for (size_t i = 0; i < K; ++i) stream_of[first + i] = s;
    if (K > 0) {
      std::memcpy(h + tot.poses_offset + first * 12 * sizeof(double), in[s].poses, K * 12 * sizeof(double));
      std::memcpy(h + tot.corr_offset + first * kPairRow * sizeof(uint32_t), in[s].corr, K * kPairRow * sizeof(uint32_t));
    }
    std::memcpy(h + plan[s].model_offset, c->markers, sizeof(c->markers));
    std::memcpy(h + plan[s].model_offset + sizeof(c->markers), c->K, sizeof(c->K));
    if (st[s].B > 0) std::memcpy(h + plan[s].blobs_offset, st[s].blobs, 2 * (size_t)st[s].B * sizeof(double));
  }
  RefineMultiArgs ma{};
  ma.up = d;
  ma.desc = (const RefineDesc*)(d + tot.desc_offset);
  ma.stream_of = (const int32_t*)(d + tot.stream_of_offset);
  ma.poses = (const double*)(d + tot.poses_offset);
  ma.corr = (const uint32_t*)(d + tot.corr_offset);
  const size_t o_rows = up + (size_t)S * sizeof(pfmpe_refine_out), o_cov = o_rows + (size_t)H * sizeof(pfmpe_refine_row);
  ma.out = (pfmpe_refine_out*)(d + up);
  ma.rows = (pfmpe_refine_row*)(d + o_rows);
  ma.cov = (double*)(d + o_cov);
  ma.H = (int32_t)H;
  // what comes back: the summaries, then the rows and the covariances as far as somebody wants them
  bool want_rows = false, want_cov = false;
  for (int s = 0; s < S; ++s) {
    want_rows = want_rows || (rows && rows[s] && Ks[s] > 0);
    want_cov = want_cov || (cov && cov[s] && Ks[s] > 0);
  }
  const size_t back = want_cov ? down : want_rows ? o_cov - up : o_rows - up;
  HIPCHK(c0, hipMemcpyAsync(d, h, up, hipMemcpyHostToDevice, c0->stream));
  RET(refine_multi_launch(c0, ma, S));
  HIPCHK(c0, hipMemcpyAsync(h + up, d + up, back, hipMemcpyDeviceToHost, c0->stream));
  HIPCHK(c0, hipStreamSynchronize(c0->stream));
  std::memcpy(out, h + up, (size_t)S * sizeof(pfmpe_refine_out));
  for (int s = 0; s < S; ++s) {
    const size_t K = (size_t)Ks[s], first = (size_t)plan[s].first;
    if (K == 0) continue;
    if (rows && rows[s]) std::memcpy(rows[s], h + o_rows + first * sizeof(pfmpe_refine_row), K * sizeof(pfmpe_refine_row));
    if (cov && cov[s]) std::memcpy(cov[s], h + o_cov + first * 36 * sizeof(double), K * 36 * sizeof(double));
  }
  return PFMPE_OK;
}

int pfmpe_host_optimise_pose(const double* markers_xyz, int M, const double* K, const double* blobs, int B,
                             const uint32_t* corr, int n_rows, const pfmpe_refine_params* params, const double* pose12,
                             pfmpe_refine_row* row, double* cov36) {
  pfmpe_refine_params prm;
  pfmpe_default_refine_params(&prm);
  if (params) prm = *params;
  if (!markers_xyz || !K || !pose12 || !row || M < 1 || B < 0 || n_rows < 0 || (B > 0 && !blobs) || (n_rows > 0 && !corr))
    return PFMPE_E_ARG;
  if (!refine_params_ok(prm) || !refine_corr_ok(corr, (size_t)n_rows, M, B) || !refine_poses_finite(pose12, 1))
    return PFMPE_E_ARG;
  double cov[36];
  gn_optimise(markers_xyz, K, blobs, corr, n_rows, prm.max_iter, prm.revert_on_divergence ? 1 : 0, prm.converged, pose12,
              *row, cov);
  if (cov36) std::memcpy(cov36, cov, sizeof(cov));
  return PFMPE_OK;
}
