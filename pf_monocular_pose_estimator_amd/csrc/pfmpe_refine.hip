// pfmpe_refine.hip — k_refine / k_refine_fold (pfmpe_refine_poses / pfmpe_refine_cloud), k_refine_multi /
// k_refine_fold_multi (pfmpe_refine_multi), k_step_tail (pfmpe_step_refine / pfmpe_step_refine_multi) and their
// launches: Gauss-Newton (pf_gn.hpp) of one hypothesis per lane, fp64 for every state type, and the call's summary.
// A TU of its own so it builds beside the others.
#include "pf_gn.hpp"
#include "pf_tail.hpp"
#include "pf_wave.hpp"
#include "pfmpe_ctx.hpp"
#include "pfmpe_refine_plan.hpp"

namespace pfmpe_impl {

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
      h.best = ra.base + i;
    }
    part_merge(acc, h);
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
  if (threadIdx.x == 0) {
    out->n = 0;  // (the host's)
    out->n_with_pairs = s.n_with;
    out->n_converged = s.n_conv;
    out->n_cap_kept = s.n_kept;
    out->n_cap_reverted = s.n_rev;
    out->iters_total = s.it_total;
    out->iters_max = s.it_max;
    out->pad = 0;
    out->best = s.best;
  }
  constexpr int kRowWords = (int)(sizeof(pfmpe_refine_row) / sizeof(double));
  double* brow = (double*)&out->best_row;
  const int q = threadIdx.x;
  if (take) {
    const int64_t i = p.best - base;
    if (q < kRowWords) brow[q] = ((const double*)(rows + i))[q];
    else if (q < kRowWords + 36) out->best_cov[q - kRowWords] = cov[36 * i + (q - kRowWords)];
  } else if (begin) {
    if (q < kRowWords) brow[q] = 0.0;
    else if (q < kRowWords + 36) out->best_cov[q - kRowWords] = 0.0;
  }
}
static_assert(sizeof(pfmpe_refine_row) / sizeof(double) + 36 <= kWave, "k_refine_fold copies a word per lane");

// The batch (pfmpe_refine_multi): one lane per hypothesis of all streams together, no grid stride (H <= kPairsChunk).
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
  for (int i = threadIdx.x; i < d.count; i += kWave) {
    const pfmpe_refine_row& r = rows[i];
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
      h.best = i;
    }
    part_merge(p, h);
  }
  part_wave_merge(p);
  if (threadIdx.x == 0) {
    out->n = d.count;
    out->n_with_pairs = p.n_with;
    out->n_converged = p.n_conv;
    out->n_cap_kept = p.n_kept;
    out->n_cap_reverted = p.n_rev;
    out->iters_total = p.it_total;
    out->iters_max = p.it_max;
    out->pad = 0;
    out->best = p.best;
  }
  constexpr int kRowWords = (int)(sizeof(pfmpe_refine_row) / sizeof(double));
  double* brow = (double*)&out->best_row;
  const int q = threadIdx.x;
  if (p.best >= 0) {
    if (q < kRowWords) brow[q] = ((const double*)(rows + p.best))[q];
    else if (q < kRowWords + 36) out->best_cov[q - kRowWords] = cov[36 * p.best + (q - kRowWords)];
  } else {
    if (q < kRowWords) brow[q] = 0.0;
    else if (q < kRowWords + 36) out->best_cov[q - kRowWords] = 0.0;
  }
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

int refine_multi_launch(pfmpe_ctx* c0, const RefineMultiArgs& ma, int S) {
  const int nblk = (ma.H + kBlock - 1) / kBlock;
  if (nblk > 0) hipLaunchKernelGGL(k_refine_multi, dim3(nblk), dim3(kBlock), 0, c0->stream, ma);
  hipLaunchKernelGGL(k_refine_fold_multi, dim3(S), dim3(kWave), 0, c0->stream, ma);
  HIPCHK(c0, hipGetLastError());
  return PFMPE_OK;
}

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

}  // namespace pfmpe_impl
