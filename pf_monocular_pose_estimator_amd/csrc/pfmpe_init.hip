// pfmpe_init.hip — brute-force P3P (re)initialisation on the device, and its
// C-ABI entry points pfmpe_p3p_histogram / pfmpe_initialise / pfmpe_initialise_multi (include/pfmpe.h).
//
// Replaces PoseEstimator::initialise (pf_mpe_lib/src/pose_estimator.cpp:1503-1786, "PE") for the
// particle-filter configuration.  Work split:
//   device  k_init_prep_multi   calculateImageVectors (PE:1072-1085), one thread per blob
//           k_p3p_filter_multi  the 3-blob spread filter (PE:1554-1581), one thread per combination
//           k_p3p_hist_multi    the histogram (PE:1543-1716): one thread per (combination, ordered marker
//                               triple), P3P + 4 back projections, exact x-window pruning of the
//                               nearest-projection search, LDS histogram flushed with integer atomics
//           k_p3p_check_multi   checkCorrespondences' P3P stage (PE:1331-1475), one thread per
//                               (candidate correspondence vector, 3-subset)
//           k_init_seed_multi   the particle seeding + fill loop (PE:1429-1437, 1755-1760) into the state
//   host    candidate vectors from the histogram (PE:1134-1288), the ordered bookkeeping of
//           checkCorrespondences (flags, particle slots, mean re-projections, PE:1425-1496) and
//           computeTransformation (PE:2139-2161)
// Integer histogram increments are commutative, so the device enumerates combinations in colex order
// and marker triples in any order; the reference's lexicographic order only matters for
// checkCorrespondences (particle slot order), which keeps it.
//
// There is one set of kernels and one host path: a batch of S contexts, driven by per-stream descriptors in device
// memory, the host stages called per stream (the work mapping of the histogram stage: pfmpe_init_plan.hpp).
// pfmpe_initialise is the batch of one; pfmpe_p3p_histogram is stage 1 of a batch of one.
#include "pfmpe_init_plan.hpp"
#include "pfmpe_prior.hpp"
#include "pf_init_index.hpp"
#include "pf_p3p.hpp"

using namespace pfmpe;
using namespace pfmpe_impl;

namespace pfmpe {

constexpr int kInitBlock = 256;
#ifndef PFMPE_P3P_MINB
#define PFMPE_P3P_MINB 2  // 2 waves per SIMD: 353 us vs 519 us at 1 (scratch 160 B vs 80 B), 476 us at 3 (spills)
#endif
constexpr double kThreshDist = 10000 * 100;  // threshDist / threshDist2 (PE:1557-1558), px^2

struct InitArgs {
  double K[9];
  double markers[kMaxMarkers * 3];
  double tol;      // back_projection_pixel_tolerance_
  double win;      // x half-window of the pruned nearest-projection search (> tol, exact superset)
  int M, B, nperm;
  int ncomb_m;     // C(M, 3) (check stage)
  int64_t ncomb;   // C(B, 3)
  int64_t items;   // ncomb * nperm (hist) or ncand * ncomb_m (check)
};

// calculateImageVectors (PE:1072-1085) of blob i
__device__ __forceinline__ void prep_blob(const InitArgs& ia, const double* __restrict__ blobs, double* __restrict__ iv,
                                          int i) {
  double v[3];
  v[0] = (blobs[2 * i] - ia.K[2]) / ia.K[0];
  v[1] = (blobs[2 * i + 1] - ia.K[5]) / ia.K[4];
  v[2] = 1;
  const double n = p3p::norm3(v);
  for (int k = 0; k < 3; ++k) iv[3 * i + k] = v[k] / n;
}

__device__ __forceinline__ double sqd(double ax, double ay, double bx, double by) {
  const double dx = ax - bx, dy = ay - by;
  return dx * dx + dy * dy;
}

// PE:1554-1581: the three blobs pairwise within threshDist, and >= 5 blobs within threshDist2 of
// their centroid (the three themselves included)
__device__ __forceinline__ void filter_comb(int B, const double* __restrict__ blobs, uint8_t* __restrict__ pass,
                                            int64_t r) {
  int a, b, c;
  unrank3(r, a, b, c);
  const double x1 = blobs[2 * a], y1 = blobs[2 * a + 1];
  const double x2 = blobs[2 * b], y2 = blobs[2 * b + 1];
  const double x3 = blobs[2 * c], y3 = blobs[2 * c + 1];
  bool ok = !(sqd(x1, y1, x2, y2) > kThreshDist) && !(sqd(x1, y1, x3, y3) > kThreshDist) &&
            !(sqd(x2, y2, x3, y3) > kThreshDist);
  if (ok) {
    const double mx = (x1 + x2 + x3) / 3, my = (y1 + y2 + y3) / 3;
    int cd = 0;
    for (int k = 0; k < B; ++k) cd += sqd(mx, my, blobs[2 * k], blobs[2 * k + 1]) < kThreshDist ? 1 : 0;
    ok = cd >= 5;
  }
  pass[r] = ok ? 1 : 0;
}

// Stage 1: one thread per (colex combination, ordered marker triple), grid-stride.  HLDS: histogram in
// LDS (flushed once per block with integer atomics) or straight to global atomics for large B x M.
// The block's LDS carve: sorted blob x, y (doubles), original index (int), then the LDS histogram.
//
// hist_block: one block's share of one stream's histogram (k_p3p_hist_multi): the items first, first + stride, ...
// of ia.items; Kc = the camera matrix where the block keeps it (LDS), lds = the block's carve (laid out as above),
// s_mk = its marker table.
template <int MAXU, bool HLDS>
__device__ __forceinline__ void hist_block(const InitArgs& ia, const double* Kc, unsigned char* lds, double* s_mk,
                                           int64_t first, int64_t stride, const double* __restrict__ blobs,
                                           const double* __restrict__ iv, const double* __restrict__ sorted_xy,
                                           const int* __restrict__ sorted_idx, const uint8_t* __restrict__ pass,
                                           uint32_t* __restrict__ hist) {
  const int B = ia.B, M = ia.M;
  double* sx = (double*)lds;
  double* sy = sx + B;
  int* sidx = (int*)(sy + B);
  uint32_t* lh = (uint32_t*)(sidx + ((B + 3) & ~3));
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    sx[i] = sorted_xy[2 * i];
    sy[i] = sorted_xy[2 * i + 1];
    sidx[i] = sorted_idx[i];
  }
  for (int i = threadIdx.x; i < 3 * M; i += blockDim.x) s_mk[i] = ia.markers[i];
  if (HLDS)
    for (int i = threadIdx.x; i < B * M; i += blockDim.x) lh[i] = 0;
  __syncthreads();
  uint32_t* H = HLDS ? lh : hist;
  const double tol = ia.tol, win = ia.win;
  const int nuo = M - 3;

  const int64_t items = ia.items;
  const int nperm = ia.nperm;
  for (int64_t item = first; item < items; item += stride) {
    const int64_t r = item / nperm;
    const int p = (int)(item - r * nperm);
    if (!pass[r]) continue;
    int sa[3];
    unrank3(r, sa[0], sa[1], sa[2]);
    int pm[3];
    perm3(p, M, pm[0], pm[1], pm[2]);
    double fv[3][3], wp[3][3];
    for (int k = 0; k < 3; ++k)
      for (int q = 0; q < 3; ++q) {
        fv[k][q] = iv[3 * sa[k] + q];
        wp[k][q] = s_mk[3 * pm[k] + q];
      }
    p3p::Setup st;
    double roots[4];
    if (!p3p::setup(fv, wp, st, roots)) continue;
    int un[MAXU > 0 ? MAXU : 1];
    unused_markers<MAXU>(pm[0], pm[1], pm[2], un);
    const double dmx = (blobs[2 * sa[0]] + blobs[2 * sa[1]] + blobs[2 * sa[2]]) / 3;
    const double dmy = (blobs[2 * sa[0] + 1] + blobs[2 * sa[1] + 1] + blobs[2 * sa[2] + 1]) / 3;
    double prev[12];
    for (int k = 0; k < 4; ++k) {
      double sol[12];
      p3p::solution(st, roots[k], sol);
      bool repeated = false;  // (solutions(k) - solutions(k-1)).all() == 0: some entry unchanged
      if (k > 0)
        for (int q = 0; q < 12; ++q) repeated = repeated || (sol[q] - prev[q] == 0);
      for (int q = 0; q < 12; ++q) prev[q] = sol[q];
      if (repeated || !p3p::finite12(sol)) continue;
      double inv[12];
      p3p::inverse34(sol, inv);
      double pu[MAXU > 0 ? MAXU : 1], pv[MAXU > 0 ? MAXU : 1];
#pragma unroll
      for (int m = 0; m < MAXU; ++m)
        if (m < nuo) p3p::project(Kc, inv, &s_mk[3 * un[m]], pu[m], pv[m]);
      bool any = false;
#pragma unroll
      for (int m = 0; m < MAXU; ++m) {
        if (m >= nuo) break;
        const double u = pu[m];
        if (!(fabs(u) < 1e300) || !(fabs(pv[m]) < 1e300)) continue;  // NaN / inf never wins a strict '<'
        int lo = 0, hi = B;                                           // first sx >= u - win
        const double xl = u - win, xh = u + win;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (sx[mid] < xl) lo = mid + 1;
          else hi = mid;
        }
        for (int q = lo; q < B && sx[q] <= xh; ++q) {
          const int bi = sidx[q];
          if (bi == sa[0] || bi == sa[1] || bi == sa[2]) continue;
          const double bx = sx[q], by = sy[q];
          if (!(sqd(dmx, dmy, bx, by) < kThreshDist)) continue;
          // calculateMinDistancesAndPairs (PE:2093-2137): nearest projection, strict '<' from +inf
          double mind = INFINITY;
          int pr = -1;
#pragma unroll
          for (int m2 = 0; m2 < MAXU; ++m2)
            if (m2 < nuo) {
              const double d = sqd(bx, by, pu[m2], pv[m2]);
              if (d < mind) {
                mind = d;
                pr = m2;
              }
            }
          if (pr != m || !(sqrt(mind) < tol)) continue;
          if (!any) {
            any = true;
            for (int mm = 0; mm < 3; ++mm) atomicAdd(&H[sa[mm] * M + pm[mm]], 1u);
          }
          atomicAdd(&H[bi * M + un[m]], 1u);
        }
      }
    }
  }
  if (HLDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < B * M; i += blockDim.x)
      if (lh[i]) atomicAdd(&hist[i], lh[i]);
  }
}

// Stage 3: checkCorrespondences' P3P part (PE:1331-1475) for candidate `ci`, lexicographic 3-subset q of
// its M correspondence rows.  cand: per candidate 2*M ints (LED, detection), 1-based.
// status: 0 = P3P failed (collinear), 1 = no solution within certainty_threshold, 2 = valid (inv = the
// inverse of the smallest-error valid solution, top 3 rows).
//
// check_item: item `item` of one stream (k_p3p_check_multi).
template <int MAXU>
__device__ __forceinline__ void check_item(const InitArgs& ia, double certainty_threshold,
                                           const double* __restrict__ blobs, const double* __restrict__ iv,
                                           const int* __restrict__ cand, const int* __restrict__ triples,
                                           uint8_t* __restrict__ status, double* __restrict__ out_inv, int64_t item) {
  const int ci = (int)(item / ia.ncomb_m);
  const int q = (int)(item - (int64_t)ci * ia.ncomb_m);
  const int M = ia.M;
  const int* cp = cand + (int64_t)ci * 2 * M;
  const int t = triples[q];
  const int s[3] = {t & 0xff, (t >> 8) & 0xff, (t >> 16) & 0xff};
  double fv[3][3], wp[3][3];
  for (int k = 0; k < 3; ++k)
    for (int d = 0; d < 3; ++d) {
      wp[k][d] = ia.markers[3 * (cp[2 * s[k]] - 1) + d];
      fv[k][d] = iv[3 * (cp[2 * s[k] + 1] - 1) + d];
    }
  int un[MAXU > 0 ? MAXU : 1];
  unused_markers<MAXU>(s[0], s[1], s[2], un);
  const int nu = M - 3;
  p3p::Setup st;
  double roots[4];
  if (!p3p::setup(fv, wp, st, roots)) {
    status[item] = 0;
    return;
  }
  const double tol2 = ia.tol * ia.tol;  // pow(tol, 2) folds to tol * tol
  double min_err = INFINITY;
  double best[12];
  bool any_valid = false;
  for (int j = 0; j < 4; ++j) {
    double sol[12];
    p3p::solution(st, roots[j], sol);
    if (!p3p::finite12(sol)) continue;
    double inv[12];
    p3p::inverse34(sol, inv);
    // calculateSquaredReprojectionErrorAndCertainty (PE:1087-1132): index-paired squared distances,
    // then up to min(size) extractions of Eigen's minCoeff (first minimum, from coeff(0)) while <= tol^2
    double dist[MAXU > 0 ? MAXU : 1];
#pragma unroll
    for (int a = 0; a < MAXU; ++a)
      if (a < nu) {
        double u, v;
        p3p::project(ia.K, inv, &ia.markers[3 * (cp[2 * un[a]] - 1)], u, v);
        const int bi = cp[2 * un[a] + 1] - 1;
        dist[a] = sqd(blobs[2 * bi], blobs[2 * bi + 1], u, v);
      }
    double sq_err = 0;
    int ncorr = 0;
    for (int it = 0; it < nu; ++it) {
      double mv = dist[0];
      int r = 0;
#pragma unroll
      for (int a = 1; a < MAXU; ++a)
        if (a < nu && dist[a] < mv) {
          mv = dist[a];
          r = a;
        }
      if (!(mv <= tol2)) break;
      sq_err += mv;
      ncorr++;
#pragma unroll
      for (int a = 0; a < MAXU; ++a)
        if (a == r) dist[a] = INFINITY;
    }
    const double certainty = (double)ncorr / (double)nu;
    if (certainty >= certainty_threshold) {
      any_valid = true;
      if (sq_err < min_err) {
        min_err = sq_err;
        for (int k = 0; k < 12; ++k) best[k] = inv[k];
      }
    }
  }
  status[item] = any_valid ? 2 : 1;
  if (any_valid)
    for (int k = 0; k < 12; ++k) out_inv[item * 12 + k] = best[k];
}

// ---------------------------------------------------------------- the kernels: a batch of S streams
// S streams (one for pfmpe_initialise and pfmpe_p3p_histogram) share each stage's launches.  A stage's descriptors
// (one InitDesc per stream, in device memory: S x 0.6 KB do not belong in kernel arguments) and its head go up with
// the stage's one upload.  The flat kernels (prep, filter,
// check, seed) run over the concatenation of the streams' elements and find the stream of an element in a prefix
// table of the head; a histogram block finds its stream from the plan's first_block.
constexpr int kInitMaxStreams = PFMPE_INIT_MAX_STREAMS;
struct InitDesc {
  InitArgs a;                  // items: the stage's (histogram / check)
  double certainty_threshold;  // check
  const double* blobs;
  double* iv;
  const double* sxy;           // histogram: x-sorted blobs, their original indices, the filter's verdicts, the counts
  const int* sidx;
  uint8_t* pass;
  uint32_t* hist;
  const int* cand;             // check: candidate table, 3-subsets, results
  const int* triples;
  uint8_t* status;
  double* out_inv;
  const double* est;           // seed: stored estimates, the member's transfer block
  double* poses;
  int32_t K, N;
  int32_t identity0;           // seed, K < N: 1 = slot 0 becomes the identity (no prior), 0 = it is there already
  int32_t first_block, blocks, lds_hist;  // histogram: the plan (pfmpe_init_plan.hpp)
};
struct InitHead {
  int32_t S, pad;
  int64_t pre[2][kInitMaxStreams + 1];        // element prefixes: [0] blobs / seed slots, [1] combinations / check items
  int32_t hb_n[4];                            // histogram launch of bucket b: its streams,
  int32_t hb_first[3][kInitMaxStreams + 1];   // their first blocks (ascending; [n] = the launch's size)
  int32_t hb_stream[3][kInitMaxStreams];      // and stream indices
};

// the stream of element g: the last s with pre[s] <= g (streams without elements are skipped)
__device__ __forceinline__ int stream_of(const int64_t* __restrict__ pre, int S, int64_t g) {
  int lo = 0, hi = S;  // pre[lo] <= g < pre[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (pre[mid] <= g) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ void k_init_prep_multi(const InitHead* __restrict__ hd, const InitDesc* __restrict__ descs) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int S = hd->S;
  if (g >= hd->pre[0][S]) return;
  const int s = stream_of(hd->pre[0], S, g);
  const InitDesc& d = descs[s];
  prep_blob(d.a, d.blobs, d.iv, (int)(g - hd->pre[0][s]));
}

__global__ void k_p3p_filter_multi(const InitHead* __restrict__ hd, const InitDesc* __restrict__ descs) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int S = hd->S;
  if (g >= hd->pre[1][S]) return;
  const int s = stream_of(hd->pre[1], S, g);
  const InitDesc& d = descs[s];
  filter_comb(d.a.B, d.blobs, d.pass, g - hd->pre[1][s]);
}

// Stage 1 of the batch, one launch per unused-marker bucket present.  Block -> stream by a binary search over the
// launch's first blocks (uniform: scalar code, once per block); then the block is block (blockIdx - first_block) of
// the `blocks` that stride over that stream's items.  Dynamic LDS: K (16 doubles), then hist_block's carve for this
// stream; the launch is sized for its largest stream.
template <int MAXU>
__global__ __launch_bounds__(kInitBlock, PFMPE_P3P_MINB) void k_p3p_hist_multi(const InitHead* __restrict__ hd,
                                                                                const InitDesc* __restrict__ descs,
                                                                                int bucket) {
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ double s_mk[kMaxMarkers * 3];
  const int32_t* first = hd->hb_first[bucket];
  int lo = 0, hi = hd->hb_n[bucket];  // first[lo] <= blockIdx.x < first[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= (int)blockIdx.x) lo = mid;
    else hi = mid;
  }
  const InitDesc& d = descs[hd->hb_stream[bucket][lo]];
  double* sK = (double*)lds;
  if (threadIdx.x < 9) sK[threadIdx.x] = d.a.K[threadIdx.x];  // hist_block's barrier publishes it
  const int64_t at = (int64_t)((int)blockIdx.x - d.first_block) * kInitBlock + threadIdx.x;
  const int64_t stride = (int64_t)d.blocks * kInitBlock;
  if (d.lds_hist)
    hist_block<MAXU, true>(d.a, sK, lds + 128, s_mk, at, stride, d.blobs, d.iv, d.sxy, d.sidx, d.pass, d.hist);
  else
    hist_block<MAXU, false>(d.a, sK, lds + 128, s_mk, at, stride, d.blobs, d.iv, d.sxy, d.sidx, d.pass, d.hist);
}

// Stage 3 of the batch: flat over the streams' (candidate, 3-subset) items.  MAXU: the largest bucket in the batch (a
// wider bucket runs the same operations on a stream of fewer markers, as within a bucket).
template <int MAXU>
__global__ __launch_bounds__(kInitBlock) void k_p3p_check_multi(const InitHead* __restrict__ hd,
                                                                 const InitDesc* __restrict__ descs) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int S = hd->S;
  if (g >= hd->pre[1][S]) return;
  const int s = stream_of(hd->pre[1], S, g);
  const InitDesc& d = descs[s];
  check_item<MAXU>(d.a, d.certainty_threshold, d.blobs, d.iv, d.cand, d.triples, d.status, d.out_inv,
                   g - hd->pre[1][s]);
}

// Stage 4 of the batch: PoseParticle after initialise (PE:1429-1437 stores, PE:1755-1760 fill) over the slots of every
// found stream, each into its member's transfer block: slot s >= 1 takes estimate ((N - s - 1) mod K) + 1 (1-based,
// estimate k sits at slot N - k); slot 0 only when K >= N.
__global__ void k_init_seed_multi(const InitHead* __restrict__ hd, const InitDesc* __restrict__ descs) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int S = hd->S;
  if (g >= hd->pre[0][S]) return;
  const int si = stream_of(hd->pre[0], S, g);
  const InitDesc& d = descs[si];
  const int s = (int)(g - hd->pre[0][si]);
  if (s == 0 && d.K < d.N) {
    if (d.identity0)
      for (int q = 0; q < 12; ++q) d.poses[q] = (q == 0 || q == 5 || q == 10) ? 1.0 : 0.0;
    return;
  }
  const int e = (d.N - s - 1) % d.K;  // 0-based estimate
  for (int q = 0; q < 12; ++q) d.poses[12 * (int64_t)s + q] = d.est[12 * (int64_t)e + q];
}

}  // namespace pfmpe

// ===================================================================================== host side
namespace {

struct Arena {
  size_t off = 0;
  template <typename X>
  size_t take(size_t n) {
    const size_t o = off;
    off += (n * sizeof(X) + 255) & ~(size_t)255;
    return o;
  }
};

// the initialisation scratch, grown to exactly what a stage needs
int ensure_init(pfmpe_ctx* c, size_t bytes) { return c->d_init.grow(c, bytes, bytes); }

InitArgs make_args(const pfmpe_ctx* c, int B) {
  InitArgs ia{};
  std::memcpy(ia.K, c->K, sizeof(ia.K));
  std::memcpy(ia.markers, c->markers, sizeof(ia.markers));
  ia.tol = c->params.tol;
  ia.win = c->params.tol * (1.0 + 1e-6) + 1e-6;
  ia.M = c->M;
  ia.B = B;
  ia.nperm = c->M * (c->M - 1) * (c->M - 2);
  ia.ncomb_m = c->M * (c->M - 1) * (c->M - 2) / 6;
  ia.ncomb = (int64_t)B * (B - 1) * (B - 2) / 6;
  return ia;
}

// correspondencesFromHistogram (PE:1134-1288) with bInitialisation = true: candidate (LED, detection)
// vectors, most probable first; ambiguous ones (a detection used twice, zeros included) dropped.  An error is
// reported on c with the text `who` + ...
int candidates(pfmpe_ctx* c, const std::string& who, int B, int M, const uint32_t* hist, int max_cand,
               std::vector<std::vector<uint32_t>>& out) {
  out.clear();
  const double prob_threshold = (1.3 * 1.0) / (double)((unsigned)B * (unsigned)M);
  std::vector<double> hp((size_t)B * M);
  for (size_t i = 0; i < hp.size(); ++i) hp[i] = (double)hist[i];
  std::vector<uint32_t> rowSum(B, 0);
  for (int r = 0; r < B; ++r)
    for (int q = 0; q < M; ++q) rowSum[r] += hist[(size_t)r * M + q];
  for (int col = 0; col < M; ++col) {
    uint32_t colSum = 0;
    for (int r = 0; r < B; ++r) colSum += hist[(size_t)r * M + col];
    if (colSum == 0) continue;
    for (int r = 0; r < B; ++r) {
      const uint32_t den = colSum * rowSum[r];  // 32-bit unsigned product, as the reference's
      double& v = hp[(size_t)r * M + col];
      v = std::max(0.0, (v * v) / (double)den);
      if (v < prob_threshold) v = 0;
    }
  }
  std::vector<std::vector<double>> up(M);
  std::vector<std::vector<int>> un(M);
  for (int a = 0; a < M; ++a)
    for (int b = 0; b < B; ++b)
      if (hp[(size_t)b * M + a] != 0) {
        up[a].push_back(hp[(size_t)b * M + a]);
        un[a].push_back(b + 1);
      }
  int64_t Ntot = 1;
  for (int k = 0; k < M; ++k) {
    Ntot *= std::max<int64_t>(1, (int64_t)up[k].size());
    if (Ntot > max_cand) return fail(c, PFMPE_E_CAP, who + "correspondence vectors exceed max_candidates");
  }
  const int N = (int)Ntot;
  std::vector<double> vp(N);
  std::vector<int> comb((size_t)N * M);
  for (int i = 0; i < N; ++i) {
    double prob = 1;
    int n = 1;
    for (int led = M - 1; led > -1; --led) {
      const int nv = (int)un[led].size();
      if (nv > 0) {
        const int idx = (i / n) % nv;
        prob = prob * up[led][idx];
        comb[(size_t)i * M + led] = un[led][idx];
        n = n * nv;
      } else {
        comb[(size_t)i * M + led] = 0;
      }
    }
    vp[i] = prob;
  }
  double sum = 0;
  for (int i = 0; i < N; ++i) sum += vp[i];
  for (int i = 0; i < N; ++i) vp[i] = vp[i] / sum;
  // N rounds of std::max_element (first maximum) with the picked entry zeroed (PE:1256-1260).  Without
  // NaNs that is: the positive entries by (value desc, index asc), then index 0 (all zero by then) for
  // each entry that was not positive.  A NaN (sum 0 or inf) falls back to the literal O(N^2) rounds.
  std::vector<int> picks;
  picks.reserve(N);
  bool has_nan = false;
  for (int i = 0; i < N; ++i) has_nan = has_nan || !(vp[i] == vp[i]);
  if (!has_nan) {
    for (int i = 0; i < N; ++i)
      if (vp[i] > 0) picks.push_back(i);
    std::stable_sort(picks.begin(), picks.end(), [&](int x, int y) { return vp[x] > vp[y]; });
    while ((int)picks.size() < N) picks.push_back(0);
  } else {
    for (int bb = 0; bb < N; ++bb) {
      int row = 0;
      for (int i = 1; i < N; ++i)
        if (vp[row] < vp[i]) row = i;
      vp[row] = 0;
      picks.push_back(row);
    }
  }
  for (int bb = 0; bb < N; ++bb) {
    const int row = picks[bb];
    const int* det = &comb[(size_t)row * M];
    bool amb = false;  // checkAmbiguity (PE:2447-2458)
    for (int i = 0; i < M && !amb; ++i)
      for (int j = M - 1; j > i; --j)
        if (det[i] == det[j]) {
          amb = true;
          break;
        }
    if (amb) continue;
    std::vector<uint32_t> pr;
    for (int led = 0; led < M; ++led)
      if (det[led] != 0) {
        pr.push_back((uint32_t)(led + 1));
        pr.push_back((uint32_t)det[led]);
      }
    out.push_back(pr);
  }
  return PFMPE_OK;
}

// computeTransformation (PE:2139-2161): R = V U^T from the SVD of the 3x3 cross-covariance (one-sided
// Jacobi), t = mean(rep) - R mean(obj).
void compute_transformation(int M, const double* obj, const double* rep, double* T12) {
  double mo[3] = {0, 0, 0}, mr[3] = {0, 0, 0};
  for (int j = 0; j < M; ++j)
    for (int k = 0; k < 3; ++k) {
      mo[k] += obj[3 * j + k];
      mr[k] += rep[3 * j + k];
    }
  for (int k = 0; k < 3; ++k) {
    mo[k] /= M;
    mr[k] /= M;
  }
  double U[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int r = 0; r < 3; ++r)
    for (int col = 0; col < 3; ++col) {
      double s = 0;
      for (int j = 0; j < M; ++j) s += (obj[3 * j + r] - mo[r]) * (rep[3 * j + col] - mr[col]);
      U[3 * r + col] = s;
    }
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double al = 0, be = 0, ga = 0;
        for (int i = 0; i < 3; ++i) {
          al += U[3 * i + p] * U[3 * i + p];
          be += U[3 * i + q] * U[3 * i + q];
          ga += U[3 * i + p] * U[3 * i + q];
        }
        if (ga == 0) continue;
        off = std::max(off, std::fabs(ga) / std::sqrt(al * be));
        const double zeta = (be - al) / (2 * ga);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1 + zeta * zeta));
        const double cs = 1 / std::sqrt(1 + t * t), sn = cs * t;
        for (int i = 0; i < 3; ++i) {
          const double up = U[3 * i + p], uq = U[3 * i + q];
          U[3 * i + p] = cs * up - sn * uq;
          U[3 * i + q] = sn * up + cs * uq;
          const double vp = V[3 * i + p], vq = V[3 * i + q];
          V[3 * i + p] = cs * vp - sn * vq;
          V[3 * i + q] = sn * vp + cs * vq;
        }
      }
    if (off < 1e-15) break;
  }
  for (int k = 0; k < 3; ++k) {
    double n = 0;
    for (int i = 0; i < 3; ++i) n += U[3 * i + k] * U[3 * i + k];
    n = std::sqrt(n);
    for (int i = 0; i < 3; ++i) U[3 * i + k] = n > 0 ? U[3 * i + k] / n : 0.0;
  }
  for (int r = 0; r < 3; ++r) {
    double R[3];
    for (int col = 0; col < 3; ++col) {
      R[col] = V[3 * r + 0] * U[3 * col + 0] + V[3 * r + 1] * U[3 * col + 1] + V[3 * r + 2] * U[3 * col + 2];
      T12[4 * r + col] = R[col];
    }
    T12[4 * r + 3] = 0;  // filled below once every row of R is known
  }
  for (int r = 0; r < 3; ++r)
    T12[4 * r + 3] = mr[r] - (T12[4 * r + 0] * mo[0] + T12[4 * r + 1] * mo[1] + T12[4 * r + 2] * mo[2]);
}

// the lexicographic 3-subsets of M rows, packed a | b << 8 | d << 16 (stage 3's order, PE:1331)
std::vector<int> lex_triples(int M) {
  std::vector<int> trip;
  for (int a = 0; a < M; ++a)
    for (int b = a + 1; b < M; ++b)
      for (int d = b + 1; d < M; ++d) trip.push_back(a | (b << 8) | (d << 16));
  return trip;
}

// The ordered bookkeeping of initialise / checkCorrespondences (PE:1425-1496, 1733-1760) over the candidates of one
// context: status / invs are stage 3's results for the candidates with M rows, in candidate order; flag: the fail
// flag so far.  Fills out's found, flag_fail, n_estimates, first_match, n_corr, corr and predicted_pose, and est: the
// stored P3P poses in store order (estimate k at slot N - k).
void book_keeping(const pfmpe_ctx* c, const std::vector<std::vector<uint32_t>>& cands, const uint8_t* status,
                  const double* invs, int N, const pfmpe_init_params& p, int flag, pfmpe_init_out* out,
                  std::vector<double>& est) {
  const int M = c->M;
  const int ncm = M * (M - 1) * (M - 2) / 6;
  int n_est = 1, found = 0;
  size_t fi = 0;
  for (size_t ci = 0; ci < cands.size(); ++ci) {
    int valid = 0;
    if ((int)cands[ci].size() < 2 * M) {
      flag = 6;
    } else {
      const size_t base = fi * ncm;
      ++fi;
      double mean_rep[kMaxMarkers][3] = {{0}};
      int num_valid = 0;
      for (int q = 0; q < ncm; ++q) {
        const uint8_t st = status[base + q];
        if (st == 0) {
          flag = 9;
          continue;
        }
        if (st != 2) continue;
        num_valid++;
        const double* inv = &invs[(base + q) * 12];
        if (N >= n_est) {
          est.insert(est.end(), inv, inv + 12);
          n_est++;
        }
        for (int jj = 0; jj < M; ++jj) {
          const double* X = c->markers + 3 * jj;
          for (int r = 0; r < 3; ++r) {
            const double v = inv[4 * r + 0] * X[0] + inv[4 * r + 1] * X[1] + inv[4 * r + 2] * X[2] + inv[4 * r + 3] * 1.0;
            mean_rep[jj][r] = mean_rep[jj][r] + v;
          }
        }
      }
      if ((double)num_valid / ncm >= p.valid_corr_threshold) {
        valid = 1;
        if (n_est < N && out->first_match < 0) {
          double rep[kMaxMarkers * 3];
          for (int jj = 0; jj < M; ++jj)
            for (int r = 0; r < 3; ++r) rep[3 * jj + r] = mean_rep[jj][r] / num_valid;
          compute_transformation(M, c->markers, rep, out->predicted_pose);
          out->first_match = (int)ci;
          out->n_corr = M;
          for (int k = 0; k < 2 * M; ++k) out->corr[k] = cands[ci][k];
        }
      } else {
        flag = num_valid > 0 ? 7 : 8;
      }
    }
    if (valid && n_est < N) found = 1;
  }
  out->found = found;
  out->n_estimates = n_est - 1;
  out->flag_fail = found ? 0 : flag;
}

// the effective parameters of a call: the defaults where prm is NULL, the default cap for max_candidates <= 0
pfmpe_init_params effective_params(const pfmpe_init_params* prm) {
  pfmpe_init_params p;
  pfmpe_default_init_params(&p);
  if (prm) p = *prm;
  if (p.max_candidates <= 0) p.max_candidates = 1 << 20;
  return p;
}

// ---------------------------------------------------------------- the batch
// one stream of the batch on the host
struct MultiStream {
  pfmpe_ctx* c = nullptr;
  std::string at;                           // what this stream's error texts begin with
  const double* blobs = nullptr;
  int B = 0, N = 0;
  pfmpe_init_params p{};
  pfmpe_init_out o{};                       // becomes out[s] when the whole batch has succeeded
  std::vector<uint32_t> hist;               // stage 1 (B >= M only)
  std::vector<std::vector<uint32_t>> cands;
  std::vector<int> full;                    // candidates with M rows
  int flag = -1;
  size_t st_off = 0;                        // stage 3: this stream's first item in the batch's results
  std::vector<double> est;
};

// a stage's upload image: the head, the descriptors, then whatever the stage appends; offsets are the arena's
struct StageImage {
  std::vector<unsigned char> bytes;
  size_t o_head, o_desc;
  Arena ar;
  explicit StageImage(int S) {
    o_head = ar.take<InitHead>(1);
    o_desc = ar.take<InitDesc>(S);
  }
  InitHead* head() { return (InitHead*)(bytes.data() + o_head); }
  InitDesc* desc() { return (InitDesc*)(bytes.data() + o_desc); }
  // room for n elements of X in the upload part; the image grows to hold it
  template <typename X>
  size_t put(const X* src, size_t n) {
    const size_t o = ar.take<X>(n);
    bytes.resize(ar.off, 0);
    if (n) std::memcpy(bytes.data() + o, src, n * sizeof(X));
    return o;
  }
  void begin() { bytes.assign(ar.off, 0); }
};

// The leader's pinned read-back block, grown by half more than asked.  Pinned and kept: the check results of a batch
// come back as one block, and with a fresh pageable vector per call a B = 50 batch of 8 took twice the time
// (DESIGN.md §4.7a).
int ensure_readback(pfmpe_ctx* c, size_t bytes) { return c->h_init.grow(c, bytes, bytes + bytes / 2); }

// Stage 1 of the batch: the histograms of the streams with B >= M (at least one) into their MultiStream::hist.
// hist_only (pfmpe_p3p_histogram): of the streams with 3 <= B < M as well.
int multi_histograms(pfmpe_ctx* c0, std::vector<MultiStream>& st, bool hist_only) {
  const int S = (int)st.size();
  int32_t Ms[kInitMaxStreams], Bs[kInitMaxStreams], per_bucket[3];
  pfmpe_init_plan plan[kInitMaxStreams];
  for (int s = 0; s < S; ++s) {
    Ms[s] = st[s].c->M;
    Bs[s] = st[s].B;
  }
  pfmpe_plan::init_plan(Ms, Bs, S, c0->num_cu, plan, per_bucket, hist_only);
  StageImage im(S);
  im.begin();
  // upload part: per stream the blobs, the x-sorted list and its indices; device part: image vectors, filter
  // verdicts, and the histograms back to back (one memset, one read-back)
  struct Off {
    size_t blobs, sxy, sidx, iv, pass, hist;
  };
  std::vector<Off> off(S);
  for (int s = 0; s < S; ++s) {
    if (plan[s].items == 0) continue;
    const int B = st[s].B;
    const double* blobs = st[s].blobs;
    // host-built x-sorted blob list for the pruned search (a data-structure build, like the PF blob table)
    std::vector<int> order(B);
    for (int i = 0; i < B; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return blobs[2 * x] < blobs[2 * y]; });
    std::vector<double> sxy(2 * (size_t)B);
    for (int i = 0; i < B; ++i) {
      sxy[2 * i] = blobs[2 * order[i]];
      sxy[2 * i + 1] = blobs[2 * order[i] + 1];
    }
    off[s].blobs = im.put(blobs, 2 * (size_t)B);
    off[s].sxy = im.put(sxy.data(), sxy.size());
    off[s].sidx = im.put(order.data(), (size_t)B);
  }
  const size_t upload = im.ar.off;
  size_t hist_words = 0;
  for (int s = 0; s < S; ++s) {
    if (plan[s].items == 0) continue;
    off[s].iv = im.ar.take<double>(3 * (size_t)st[s].B);
    off[s].pass = im.ar.take<uint8_t>((size_t)(plan[s].items / (Ms[s] * (Ms[s] - 1) * (Ms[s] - 2))));
    off[s].hist = hist_words;
    hist_words += (size_t)st[s].B * Ms[s];
  }
  const size_t o_hist = im.ar.take<uint32_t>(hist_words);
  RET(ensure_init(c0, im.ar.off));
  RET(ensure_readback(c0, hist_words * sizeof(uint32_t)));
  unsigned char* d = c0->d_init.get();
  InitHead* hd = im.head();
  InitDesc* ds = im.desc();
  hd->S = S;
  size_t lds[3] = {0, 0, 0};
  for (int s = 0; s < S; ++s) {
    hd->pre[0][s + 1] = hd->pre[0][s];
    hd->pre[1][s + 1] = hd->pre[1][s];
    if (plan[s].items == 0) continue;
    const int B = st[s].B, M = Ms[s];
    InitDesc& e = ds[s];
    e.a = make_args(st[s].c, B);
    e.a.items = plan[s].items;
    e.blobs = (const double*)(d + off[s].blobs);
    e.sxy = (const double*)(d + off[s].sxy);
    e.sidx = (const int*)(d + off[s].sidx);
    e.iv = (double*)(d + off[s].iv);
    e.pass = d + off[s].pass;
    e.hist = (uint32_t*)(d + o_hist) + off[s].hist;
    e.first_block = plan[s].first_block;
    e.blocks = plan[s].blocks;
    e.lds_hist = plan[s].lds_hist;
    hd->pre[0][s + 1] += B;
    hd->pre[1][s + 1] += e.a.ncomb;
    const int b = plan[s].bucket;
    hd->hb_first[b][hd->hb_n[b]] = plan[s].first_block;
    hd->hb_stream[b][hd->hb_n[b]] = s;
    hd->hb_n[b] += 1;
    const size_t hist_bytes = (size_t)B * M * sizeof(uint32_t);
    lds[b] = std::max(lds[b], (size_t)128 + (size_t)B * 16 + (size_t)((B + 3) & ~3) * 4 + (e.lds_hist ? hist_bytes : 0));
  }
  for (int b = 0; b < 3; ++b) hd->hb_first[b][hd->hb_n[b]] = per_bucket[b];
  const InitHead* d_hd = (const InitHead*)(d + im.o_head);
  const InitDesc* d_ds = (const InitDesc*)(d + im.o_desc);
  HIPCHK(c0, hipMemcpyAsync(d, im.bytes.data(), upload, hipMemcpyHostToDevice, c0->stream));
  HIPCHK(c0, hipMemsetAsync(d + o_hist, 0, hist_words * sizeof(uint32_t), c0->stream));
  hipLaunchKernelGGL(k_init_prep_multi, dim3((unsigned)((hd->pre[0][S] + 255) / 256)), dim3(256), 0, c0->stream, d_hd,
                     d_ds);
  HIPCHK(c0, hipGetLastError());
  hipLaunchKernelGGL(k_p3p_filter_multi, dim3((unsigned)((hd->pre[1][S] + 255) / 256)), dim3(256), 0, c0->stream, d_hd,
                     d_ds);
  HIPCHK(c0, hipGetLastError());
  RET(launch(c0, PFMPE_K_P3P_HIST, [&] {
    if (per_bucket[0])
      hipLaunchKernelGGL((k_p3p_hist_multi<2>), dim3(per_bucket[0]), dim3(kInitBlock), lds[0], c0->stream, d_hd, d_ds, 0);
    if (per_bucket[1])
      hipLaunchKernelGGL((k_p3p_hist_multi<9>), dim3(per_bucket[1]), dim3(kInitBlock), lds[1], c0->stream, d_hd, d_ds, 1);
    if (per_bucket[2])
      hipLaunchKernelGGL((k_p3p_hist_multi<kMaxMarkers - 3>), dim3(per_bucket[2]), dim3(kInitBlock), lds[2], c0->stream,
                         d_hd, d_ds, 2);
  }));
  const uint32_t* all = (const uint32_t*)c0->h_init.get();
  HIPCHK(c0, hipMemcpyAsync(c0->h_init.get(), d + o_hist, hist_words * sizeof(uint32_t), hipMemcpyDeviceToHost,
                            c0->stream));
  HIPCHK(c0, hipStreamSynchronize(c0->stream));
  if (c0->timing_now) RET(harvest_timing(c0));
  for (int s = 0; s < S; ++s)
    if (plan[s].items != 0) st[s].hist.assign(all + off[s].hist, all + off[s].hist + (size_t)st[s].B * Ms[s]);
  return PFMPE_OK;
}

// Stage 3 of the batch: every candidate with M rows of every stream x every lexicographic 3-subset; the results in
// candidate order, stream after stream (MultiStream::st_off), in the leader's read-back block (null without items).
int multi_check(pfmpe_ctx* c0, std::vector<MultiStream>& st, const uint8_t** status, const double** invs) {
  const int S = (int)st.size();
  StageImage im(S);
  im.begin();
  struct Off {
    size_t blobs, cand, trip, iv;
  };
  std::vector<Off> off(S);
  size_t items = 0;
  int bucket = 0;
  for (int s = 0; s < S; ++s) {
    MultiStream& m = st[s];
    if (m.full.empty()) continue;
    const int M = m.c->M;
    std::vector<int> ctab(m.full.size() * 2 * M);
    for (size_t f = 0; f < m.full.size(); ++f)
      for (int k = 0; k < 2 * M; ++k) ctab[f * 2 * M + k] = (int)m.cands[m.full[f]][k];
    const std::vector<int> trip = lex_triples(M);
    off[s].blobs = im.put(m.blobs, 2 * (size_t)m.B);
    off[s].cand = im.put(ctab.data(), ctab.size());
    off[s].trip = im.put(trip.data(), trip.size());
    m.st_off = items;
    items += m.full.size() * trip.size();
    bucket = std::max(bucket, pfmpe_plan::init_bucket(M));
  }
  *status = nullptr;
  *invs = nullptr;
  if (items == 0) return PFMPE_OK;
  const size_t h_inv = (items + 255) & ~(size_t)255;  // read-back block: the status bytes, then the poses
  RET(ensure_readback(c0, h_inv + items * 12 * sizeof(double)));
  const size_t upload = im.ar.off;
  for (int s = 0; s < S; ++s)
    if (!st[s].full.empty()) off[s].iv = im.ar.take<double>(3 * (size_t)st[s].B);
  const size_t o_s = im.ar.take<uint8_t>(items), o_i = im.ar.take<double>(items * 12);
  RET(ensure_init(c0, im.ar.off));
  unsigned char* d = c0->d_init.get();
  InitHead* hd = im.head();
  InitDesc* ds = im.desc();
  hd->S = S;
  for (int s = 0; s < S; ++s) {
    const MultiStream& m = st[s];
    hd->pre[0][s + 1] = hd->pre[0][s];
    hd->pre[1][s + 1] = hd->pre[1][s];
    if (m.full.empty()) continue;
    InitDesc& e = ds[s];
    e.a = make_args(m.c, m.B);
    e.a.items = (int64_t)m.full.size() * e.a.ncomb_m;
    e.certainty_threshold = m.p.certainty_threshold;
    e.blobs = (const double*)(d + off[s].blobs);
    e.iv = (double*)(d + off[s].iv);
    e.cand = (const int*)(d + off[s].cand);
    e.triples = (const int*)(d + off[s].trip);
    e.status = d + o_s + m.st_off;
    e.out_inv = (double*)(d + o_i) + m.st_off * 12;
    hd->pre[0][s + 1] += m.B;
    hd->pre[1][s + 1] += e.a.items;
  }
  const InitHead* d_hd = (const InitHead*)(d + im.o_head);
  const InitDesc* d_ds = (const InitDesc*)(d + im.o_desc);
  HIPCHK(c0, hipMemcpyAsync(d, im.bytes.data(), upload, hipMemcpyHostToDevice, c0->stream));
  hipLaunchKernelGGL(k_init_prep_multi, dim3((unsigned)((hd->pre[0][S] + 255) / 256)), dim3(256), 0, c0->stream, d_hd,
                     d_ds);
  HIPCHK(c0, hipGetLastError());
  const dim3 grid((unsigned)((items + kInitBlock - 1) / kInitBlock));
  RET(launch(c0, PFMPE_K_P3P_CHECK, [&] {
    if (bucket == 0)
      hipLaunchKernelGGL((k_p3p_check_multi<2>), grid, dim3(kInitBlock), 0, c0->stream, d_hd, d_ds);
    else if (bucket == 1)
      hipLaunchKernelGGL((k_p3p_check_multi<9>), grid, dim3(kInitBlock), 0, c0->stream, d_hd, d_ds);
    else
      hipLaunchKernelGGL((k_p3p_check_multi<kMaxMarkers - 3>), grid, dim3(kInitBlock), 0, c0->stream, d_hd, d_ds);
  }));
  unsigned char* h = c0->h_init.get();
  HIPCHK(c0, hipMemcpyAsync(h, d + o_s, items, hipMemcpyDeviceToHost, c0->stream));
  HIPCHK(c0, hipMemcpyAsync(h + h_inv, d + o_i, items * 12 * sizeof(double), hipMemcpyDeviceToHost, c0->stream));
  HIPCHK(c0, hipStreamSynchronize(c0->stream));
  *status = h;
  *invs = (const double*)(h + h_inv);
  return PFMPE_OK;
}

// Stage 4 of the batch: seed every found member's transfer block in one launch, import each on the leader's stream,
// one synchronise.  The members' transfer blocks exist already (multi_run: nothing may fail between the first
// import and the last for a reason other than the device).
int multi_seed(pfmpe_ctx* c0, std::vector<MultiStream>& st) {
  const int S = (int)st.size();
  StageImage im(S);
  im.begin();
  std::vector<size_t> o_est(S, 0);
  for (int s = 0; s < S; ++s)
    if (st[s].o.found) o_est[s] = im.put(st[s].est.data(), st[s].est.size());
  RET(ensure_init(c0, im.ar.off));
  unsigned char* d = c0->d_init.get();
  InitHead* hd = im.head();
  InitDesc* ds = im.desc();
  hd->S = S;
  for (int s = 0; s < S; ++s) {
    MultiStream& m = st[s];
    hd->pre[0][s + 1] = hd->pre[0][s];
    if (!m.o.found) continue;
    InitDesc& e = ds[s];
    e.est = (const double*)(d + o_est[s]);
    e.poses = m.c->d_xfer.get();
    e.K = m.o.n_estimates;
    e.N = m.N;
    e.identity0 = m.c->has_prior ? 0 : 1;
    hd->pre[0][s + 1] += m.N;
    // slot 0 keeps the resident set's slot 0 when K < N (identity when there is none: the seeding kernel's)
    if (e.K < e.N && m.c->has_prior) RET(export_prior(m.c, 1, c0->stream, c0));
  }
  HIPCHK(c0, hipMemcpyAsync(d, im.bytes.data(), im.ar.off, hipMemcpyHostToDevice, c0->stream));
  hipLaunchKernelGGL(k_init_seed_multi, dim3((unsigned)((hd->pre[0][S] + 255) / 256)), dim3(256), 0, c0->stream,
                     (const InitHead*)(d + im.o_head), (const InitDesc*)(d + im.o_desc));
  HIPCHK(c0, hipGetLastError());
  for (int s = 0; s < S; ++s)
    if (st[s].o.found)  // anchor (fp16 state): the first stored estimate
      RET(import_enqueue(st[s].c, st[s].N, st[s].est.data(), c0->stream, c0));
  HIPCHK(c0, hipStreamSynchronize(c0->stream));
  for (int s = 0; s < S; ++s)
    if (st[s].o.found) import_done(st[s].c, st[s].N);
  return PFMPE_OK;
}

// The validated batch: stages 1 to 4 on the leader's stream, then out / the members' ordering state.  single: the
// batch of one of pfmpe_initialise, which reports a failed allocation of its transfer block as it is.
int multi_run(pfmpe_ctx* const* ctxs, std::vector<MultiStream>& st, pfmpe_init_out* out, uint32_t* const* hist_out,
              bool single) {
  pfmpe_ctx* c0 = ctxs[0];
  const int S = (int)st.size();
  RET(set_device(c0));
  // every member's work so far is ordered before the batch; a failure from here on gives the members their
  // ordering state back (the leader's own was set by set_device)
  OrderGuard members(ctxs, S);  // (not BatchMembers: a synchronise per stage, no single end for its finish())
  RET(members.order(1, c0->stream, c0));
  const uint8_t* status = nullptr;
  const double* invs = nullptr;
  // stages 1 to 3 are the timed ones: the seeding's exports and imports are not bracketed
  RET(timed(c0, [&] {
    RET(multi_histograms(c0, st, false));
    for (int s = 0; s < S; ++s)
      if (hist_out && hist_out[s] && !st[s].hist.empty())
        std::memcpy(hist_out[s], st[s].hist.data(), st[s].hist.size() * sizeof(uint32_t));
    for (int s = 0; s < S; ++s) {
      MultiStream& m = st[s];
      if (m.hist.empty()) continue;  // B < M: flag 10
      uint64_t tot = 0;
      for (uint32_t h : m.hist) tot += h;
      m.o.hist_total = tot;
      if (tot == 0) {
        m.o.flag_fail = 12;
        continue;
      }
      RET(candidates(c0, m.at, m.B, m.c->M, m.hist.data(), m.p.max_candidates, m.cands));
      m.o.n_candidates = (int)m.cands.size();
      m.flag = m.cands.empty() ? 11 : -1;
      for (size_t i = 0; i < m.cands.size(); ++i)
        if ((int)m.cands[i].size() == 2 * m.c->M) m.full.push_back((int)i);
    }
    RET(multi_check(c0, st, &status, &invs));
    return c0->timing_now ? harvest_timing(c0) : (int)PFMPE_OK;
  }));
  bool any_found = false;
  for (int s = 0; s < S; ++s) {
    MultiStream& m = st[s];
    if (m.hist.empty() || m.o.hist_total == 0) continue;
    book_keeping(m.c, m.cands, status + m.st_off, invs + m.st_off * 12, m.N, m.p, m.flag, &m.o, m.est);
    if (m.o.found) {
      any_found = true;
      if (const int rc = ensure_xfer(m.c)) return single ? rc : fail(c0, PFMPE_E_HIP, m.at + m.c->err);
    }
  }
  if (any_found) RET(multi_seed(c0, st));
  members.commit();  // nothing of the batch is pending: no member needs a fence
  for (int s = 0; s < S; ++s) out[s] = st[s].o;
  return PFMPE_OK;
}

// The checks of one stream's arguments, for the single call and the batch alike, into m; an error is reported on
// `rep` with the text `at` + ...  A stream with B < M gets flag 10 and never reaches the device (PE:1507-1512: the PF
// initialisation needs every marker detected).
int validate_stream(pfmpe_ctx* rep, const std::string& at, pfmpe_ctx* c, const double* blobs, int B,
                    const pfmpe_init_params* prm, MultiStream& m) {
  if (B < 0 || (B > 0 && !blobs)) return fail(rep, PFMPE_E_ARG, at + "bad arguments");
  if (!c->has_model) return fail(rep, PFMPE_E_STATE, at + "set_model first");
  if (c->M < 3) return fail(rep, PFMPE_E_ARG, at + "needs M >= 3 markers");
  if (B > c->max_blobs) return fail(rep, PFMPE_E_CAP, at + "B exceeds max_blobs");
  m.c = c;
  m.at = at;
  m.blobs = blobs;
  m.B = B;
  m.p = effective_params(prm);
  m.N = m.p.n_particles > 0 ? m.p.n_particles : (c->has_prior ? c->N : c->max_particles);
  if (m.N > c->max_particles) return fail(rep, PFMPE_E_CAP, at + "n_particles exceeds max_particles");
  m.o.first_match = -1;
  if (B < c->M) m.o.flag_fail = 10;
  return PFMPE_OK;
}

}  // namespace

extern "C" {

void pfmpe_default_init_params(pfmpe_init_params* p) {
  if (!p) return;
  p->certainty_threshold = 1.0;   // README.md:245, launch file README.md:340
  p->valid_corr_threshold = 0.5;  // README.md:249
  p->n_particles = 0;
  p->max_candidates = 1 << 20;
}

// stage 1 of a batch of one; unlike pfmpe_initialise it computes the histogram for 3 <= B < M too
int pfmpe_p3p_histogram(pfmpe_ctx* c, const double* blobs, int B, uint32_t* hist) {
  if (!c) return PFMPE_E_ARG;
  if (!blobs || !hist) return fail(c, PFMPE_E_ARG, "p3p_histogram: null blobs/hist");
  if (!c->has_model) return fail(c, PFMPE_E_STATE, "p3p_histogram: set_model first");
  if (c->M < 3) return fail(c, PFMPE_E_ARG, "p3p_histogram: needs M >= 3 markers");
  if (B < 3) return fail(c, PFMPE_E_ARG, "p3p_histogram: needs B >= 3 blobs");
  if (B > c->max_blobs) return fail(c, PFMPE_E_CAP, "p3p_histogram: B exceeds max_blobs");
  RET(set_device(c));
  std::vector<MultiStream> st(1);
  st[0].c = c;
  st[0].blobs = blobs;
  st[0].B = B;
  RET(timed(c, [&] { return multi_histograms(c, st, true); }));
  std::memcpy(hist, st[0].hist.data(), st[0].hist.size() * sizeof(uint32_t));
  return PFMPE_OK;
}

// the batch of one
int pfmpe_initialise(pfmpe_ctx* c, const double* blobs, int B, const pfmpe_init_params* prm, pfmpe_init_out* out,
                     uint32_t* hist_out) {
  if (!c) return PFMPE_E_ARG;
  if (!out) return fail(c, PFMPE_E_ARG, "initialise: bad arguments");
  std::vector<MultiStream> st(1);
  RET(validate_stream(c, "initialise: ", c, blobs, B, prm, st[0]));
  if (B < c->M) {  // nothing touches the device
    *out = st[0].o;
    return PFMPE_OK;
  }
  return multi_run(&c, st, out, &hist_out, true);
}

int pfmpe_initialise_multi(pfmpe_ctx* const* ctxs, int S, const pfmpe_init_in* in, const pfmpe_init_params* prm,
                           pfmpe_init_out* out, uint32_t* const* hist_out) {
  if (!ctxs || S < 1 || !ctxs[0]) return PFMPE_E_ARG;
  pfmpe_ctx* c0 = ctxs[0];
  if (!in || !out) return fail(c0, PFMPE_E_ARG, "initialise_multi: null in/out");
  if (S > PFMPE_INIT_MAX_STREAMS) return fail(c0, PFMPE_E_CAP, "initialise_multi: S exceeds PFMPE_INIT_MAX_STREAMS");
  std::vector<MultiStream> st(S);
  bool any = false;  // a stream that reaches the device
  for (int s = 0; s < S; ++s) {
    pfmpe_ctx* c = ctxs[s];
    const std::string at = "initialise_multi: stream " + std::to_string(s) + ": ";
    if (!c) return fail(c0, PFMPE_E_ARG, at + "null context");
    for (int e = 0; e < s; ++e)
      if (ctxs[e] == c) return fail(c0, PFMPE_E_ARG, at + "context appears twice");
    if (c->device != c0->device) return fail(c0, PFMPE_E_ARG, at + "device must match ctxs[0]");
    RET(validate_stream(c0, at, c, in[s].blobs, in[s].B, prm ? prm + s : nullptr, st[s]));
    any = any || in[s].B >= c->M;
  }
  if (!any) {  // nothing touches the device
    for (int s = 0; s < S; ++s) out[s] = st[s].o;
    return PFMPE_OK;
  }
  return multi_run(ctxs, st, out, hist_out, false);
}

}  // extern "C"
