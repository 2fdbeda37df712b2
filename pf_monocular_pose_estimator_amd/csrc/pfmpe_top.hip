// pfmpe_top.hip — pfmpe_top_particles (pf_top.hpp): its kernels, their launches and the entry point, and
// pfmpe_host_top_suppress.
//
// Selection: an exact radix select over the keys' bit patterns (pf_top.hpp TopKey), most significant digit first, 11
// bits a pass.  Every kernel is one launch over the same grid of contiguous strips; nothing waits on another block.
//   k_top_hist (one per digit pass): every block first derives the pass's state from the previous pass's finished
//     histogram (top_resolve, the same integers in every block; block 0 stores it for the next kernel), then counts
//     the digits of its strip's keys that carry the prefix: LDS atomics, then one device atomic per non-empty bin.
//     Integer adds: the order does not matter.  Once the keys that carry the prefix all fit the pool the later passes
//     return at once.
//   k_top_count: resolves the last pass into the threshold key and counts each strip's keys above / equal to it.
//   k_top_scatter: every block scans the per-block counts in block order (= index order), so the slots of its keys are
//     fixed numbers: every key above the threshold, and the lowest-index keys equal to it that fill the pool.  A block
//     that contributes nothing returns without reading a key.  Ranks within a strip come from an ordered block scan
//     per tile, never from an atomic's arrival order.
//   k_top_sort: one block sorts the <= 1024 candidates by (key descending, index ascending) in LDS (bitonic).
// Then the pool's poses are regenerated (k_regen_list, pfmpe_seq.hpp), and
//   k_top_near: the P x P near-matrix as bit rows (bit i of row j: kept candidate i would suppress j), in parallel;
//   k_top_walk: wave 0 walks the rows in rank order with the kept mask across its lanes (lane l holds word l), then
//     the block gathers the kept rows into the record.
#include "pf_top.hpp"
#include "pfmpe_ctx.hpp"

namespace pfmpe {

namespace {

// inclusive scan of one value per thread over the block, through LDS (sh: kBlock words); returns the thread's
// inclusive sum, *total the block's
__device__ __forceinline__ uint32_t top_block_scan(uint32_t v, uint32_t* sh, uint32_t* total) {
  const int t = threadIdx.x;
  __syncthreads();  // sh may still be read from an earlier use
  sh[t] = v;
  __syncthreads();
#pragma unroll
  for (int d = 1; d < kBlock; d <<= 1) {
    const uint32_t a = t >= d ? sh[t - d] : 0u;
    __syncthreads();
    sh[t] += a;
    __syncthreads();
  }
  *total = sh[kBlock - 1];
  return sh[t];
}

// The state entering pass q + 1 from the state entering pass q and pass q's finished histogram: the digit d with
// (keys in bins above d) < need <= (keys in bins d and above).  Every thread of the block returns the same state.
__device__ TopState top_resolve(const TopState prev, const uint32_t* __restrict__ hist, int q, int shift, uint32_t* sh,
                                uint32_t* res /* 3 words */) {
  if (prev.done) return prev;
  const int t = threadIdx.x;
  constexpr int kPer = kTopBins / kBlock;  // bins per thread, highest bins first
  uint32_t c[kPer], s = 0;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    c[k] = hist[kTopBins - 1 - (kPer * t + k)];
    s += c[k];
  }
  uint32_t total;
  const uint32_t incl = top_block_scan(s, sh, &total);
  TopState S = prev;
  if (q == 0) {
    S.n_positive = (int64_t)total;
    S.pool = total < (uint32_t)kTopPool ? total : (uint32_t)kTopPool;
    S.need = S.pool;
  }
  if (S.need == 0) {  // no eligible key
    S.done = 1;
    return S;
  }
  uint32_t above = incl - s;
  if (above < S.need && S.need <= incl) {
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      if (above < S.need && S.need <= above + c[k]) {
        res[0] = (uint32_t)(kTopBins - 1 - (kPer * t + k));
        res[1] = above;
        res[2] = c[k];
      }
      above += c[k];
    }
  }
  __syncthreads();
  const uint32_t d = res[0], ab = res[1], cd = res[2];
  __syncthreads();  // res is free again
  S.prefix = prev.prefix | ((uint64_t)d << shift);
  S.need = S.need - ab;
  S.done = cd == S.need ? 1u : 0u;
  return S;
}

// f(n, bits) for every key of this block's strip; 4 keys per lane and load
template <typename KT, typename F>
__device__ __forceinline__ void top_for_strip(const KT* __restrict__ keys, int N, F&& f) {
  typedef KT V4 __attribute__((ext_vector_type(4)));
  const int per = top_strip(N, (int)gridDim.x);
  const int64_t s0 = (int64_t)blockIdx.x * per;
  const int64_t s1 = s0 + per < N ? s0 + per : N;
  for (int64_t n = s0 + 4 * (int64_t)threadIdx.x; n < s1; n += 4 * kBlock) {
    if (n + 4 <= s1) {
      const V4 v = *(const V4*)(keys + n);
      f(n, TopKey<KT>::bits(v.x));
      f(n + 1, TopKey<KT>::bits(v.y));
      f(n + 2, TopKey<KT>::bits(v.z));
      f(n + 3, TopKey<KT>::bits(v.w));
    } else {
      for (int64_t m = n; m < s1; ++m) f(m, TopKey<KT>::bits(keys[m]));
    }
  }
}

template <typename KT>
__global__ __launch_bounds__(kBlock) void k_top_hist(const KT* __restrict__ keys, int N, int pass,
                                                    uint32_t* __restrict__ hist, TopState* __restrict__ state) {
  using U = typename TopKey<KT>::U;
  constexpr int kBits = TopKey<KT>::kBits;
  __shared__ uint32_t bins[kTopBins];
  __shared__ uint32_t sh[kBlock];
  __shared__ uint32_t res[3];
  TopState S = state[0];  // zeros: the host cleared it
  if (pass > 0) {
    S = top_resolve(state[pass - 1], hist + (size_t)(pass - 1) * kTopBins, pass - 1, top_shift(kBits, pass - 1), sh, res);
    if (blockIdx.x == 0 && threadIdx.x == 0) state[pass] = S;
    if (S.done) return;
  }
  for (int i = threadIdx.x; i < kTopBins; i += kBlock) bins[i] = 0u;
  __syncthreads();
  const int shift = top_shift(kBits, pass);
  const uint32_t mask = (1u << top_width(kBits, pass)) - 1u;
  const U prefix = (U)S.prefix;
  const int above = shift + top_width(kBits, pass);  // the decided digits sit above this bit (pass > 0: < kBits)
  top_for_strip<KT>(keys, N, [&](int64_t, U b) {
    const bool in = b != 0 && (pass == 0 || ((b ^ prefix) >> above) == 0);
    if (in) (void)__hip_atomic_fetch_add(bins + ((uint32_t)(b >> shift) & mask), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  });
  __syncthreads();
  uint32_t* out = hist + (size_t)pass * kTopBins;
  for (int i = threadIdx.x; i < kTopBins; i += kBlock) {
    const uint32_t x = bins[i];
    if (x) (void)__hip_atomic_fetch_add(out + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// the result state from the last pass: keys above `prefix` are taken, and the `need` lowest-index keys equal to it
template <typename KT>
__global__ __launch_bounds__(kBlock) void k_top_count(const KT* __restrict__ keys, int N, const uint32_t* __restrict__ hist,
                                                     TopState* __restrict__ state, TopBlockCount* __restrict__ bc) {
  using U = typename TopKey<KT>::U;
  constexpr int kBits = TopKey<KT>::kBits;
  constexpr int kLast = top_passes(kBits) - 1;
  __shared__ uint32_t sh[kBlock];
  __shared__ uint32_t res[3];
  __shared__ uint32_t cnt[2];
  TopState S = top_resolve(state[kLast], hist + (size_t)kLast * kTopBins, kLast, 0, sh, res);
  if (S.done) {  // every key that carries the prefix is taken: all keys >= prefix, none by the equal rule
    S.prefix = S.prefix ? S.prefix - 1 : 0;
    S.need = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) state[kTopMaxPasses] = S;
  if (threadIdx.x < 2) cnt[threadIdx.x] = 0u;
  __syncthreads();
  const U thr = (U)S.prefix;
  uint32_t gt = 0, eq = 0;
  top_for_strip<KT>(keys, N, [&](int64_t, U b) {
    gt += b > thr ? 1u : 0u;
    eq += (b == thr && b != 0) ? 1u : 0u;
  });
  if (gt) (void)__hip_atomic_fetch_add(&cnt[0], gt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (eq) (void)__hip_atomic_fetch_add(&cnt[1], eq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();
  if (threadIdx.x == 0) {
    TopBlockCount r;
    r.gt = cnt[0];
    r.eq = cnt[1];
    bc[blockIdx.x] = r;
  }
}

template <typename KT>
__global__ __launch_bounds__(kBlock) void k_top_scatter(const KT* __restrict__ keys, int N, const TopState* __restrict__ state,
                                                       const TopBlockCount* __restrict__ bc, uint64_t* __restrict__ cand_key,
                                                       uint32_t* __restrict__ cand_idx) {
  using U = typename TopKey<KT>::U;
  typedef KT V4 __attribute__((ext_vector_type(4)));
  __shared__ uint32_t sh[kBlock];
  __shared__ uint32_t mine[4];
  const TopState S = state[kTopMaxPasses];
  const int t = threadIdx.x, nblk = (int)gridDim.x, blk = (int)blockIdx.x;
  // the blocks' counts in block order: thread t holds blocks 4 t .. 4 t + 3
  constexpr int kPer = kTopMaxBlocks / kBlock;
  uint32_t g[kPer], e[kPer], gs = 0, es = 0;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int b = kPer * t + k;
    g[k] = b < nblk ? bc[b].gt : 0u;
    e[k] = b < nblk ? bc[b].eq : 0u;
    gs += g[k];
    es += e[k];
  }
  uint32_t tot;
  uint32_t gbase = top_block_scan(gs, sh, &tot) - gs;
  uint32_t ebase = top_block_scan(es, sh, &tot) - es;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    if (kPer * t + k == blk) {
      mine[0] = gbase;
      mine[1] = g[k];
      mine[2] = ebase;
      mine[3] = e[k];
    }
    gbase += g[k];
    ebase += e[k];
  }
  __syncthreads();
  const uint32_t g0 = mine[0], gn = mine[1], e0 = mine[2], en = mine[3];
  // equal keys of this strip that are taken: ranks e0 .. e0 + en - 1 among all equal keys, the first S.need count
  const uint32_t etake = e0 >= S.need ? 0u : (S.need - e0 < en ? S.need - e0 : en);
  if (gn == 0 && etake == 0) return;
  const uint32_t eslot0 = S.pool - S.need;  // the keys above the threshold fill the slots before it
  const U thr = (U)S.prefix;
  const int per = top_strip(N, nblk);
  const int64_t s0 = (int64_t)blk * per;
  const int64_t s1 = s0 + per < N ? s0 + per : N;
  uint32_t gr = 0, er = 0;  // ranks within the strip so far (the same in every thread)
  for (int64_t base = s0; base < s1 && (gr < gn || er < etake); base += 4 * kBlock) {
    const int64_t n = base + 4 * (int64_t)t;
    U b[4] = {0, 0, 0, 0};
    if (n + 4 <= s1) {
      const V4 v = *(const V4*)(keys + n);
      b[0] = TopKey<KT>::bits(v.x);
      b[1] = TopKey<KT>::bits(v.y);
      b[2] = TopKey<KT>::bits(v.z);
      b[3] = TopKey<KT>::bits(v.w);
    } else {
      for (int k = 0; k < 4; ++k)
        if (n + k < s1) b[k] = TopKey<KT>::bits(keys[n + k]);
    }
    uint32_t pk = 0;  // keys above in the low half, equal keys in the high half (at most 1024 of each per tile)
#pragma unroll
    for (int k = 0; k < 4; ++k) pk += (b[k] > thr ? 1u : 0u) + ((b[k] == thr && b[k] != 0) ? 0x10000u : 0u);
    uint32_t tile;
    const uint32_t ex = top_block_scan(pk, sh, &tile) - pk;
    uint32_t gi = gr + (ex & 0xffffu), ei = er + (ex >> 16);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (b[k] > thr) {
        const uint32_t slot = g0 + gi++;
        if (slot < (uint32_t)kTopPool) {
          cand_key[slot] = (uint64_t)b[k];
          cand_idx[slot] = (uint32_t)(n + k);
        }
      } else if (b[k] == thr && b[k] != 0) {
        const uint32_t r = e0 + ei++;
        const uint32_t slot = eslot0 + r;
        if (r < S.need && slot < (uint32_t)kTopPool) {
          cand_key[slot] = (uint64_t)b[k];
          cand_idx[slot] = (uint32_t)(n + k);
        }
      }
    }
    gr += tile & 0xffffu;
    er += tile >> 16;
  }
}

// (key descending, index ascending): a total order, the reference's first-max rule extended to the pool
__device__ __forceinline__ bool top_before(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
  return ka > kb || (ka == kb && ia < ib);
}
template <typename KT>
__global__ __launch_bounds__(kTopPool) void k_top_sort(const TopState* __restrict__ state, const uint64_t* __restrict__ cand_key,
                                                      const uint32_t* __restrict__ cand_idx, double* __restrict__ pool_key,
                                                      int32_t* __restrict__ pool_idx) {
  __shared__ uint64_t sk[kTopPool];
  __shared__ uint32_t si[kTopPool];
  const int t = threadIdx.x;
  const int P = (int)state[kTopMaxPasses].pool;
  sk[t] = t < P ? cand_key[t] : 0ull;  // the padding sorts behind every candidate
  si[t] = t < P ? cand_idx[t] : 0xffffffffu;
  __syncthreads();
  for (int k = 2; k <= kTopPool; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int o = t ^ j;
      if (o > t) {
        const uint64_t ka = sk[t], kb = sk[o];
        const uint32_t ia = si[t], ib = si[o];
        const bool up = (t & k) == 0;  // this pair's run is ranked first-to-last
        if (up ? top_before(kb, ib, ka, ia) : top_before(ka, ia, kb, ib)) {
          sk[t] = kb;
          sk[o] = ka;
          si[t] = ib;
          si[o] = ia;
        }
      }
      __syncthreads();
    }
  }
  if (t < P) {
    pool_key[t] = TopKey<KT>::value(sk[t]);
    pool_idx[t] = (int32_t)si[t];
  }
}

// word w of row j: bit i (candidate 32 w + i, ranked before j) set when candidate j is near it
__global__ __launch_bounds__(kBlock) void k_top_near(const TopState* __restrict__ state, const double* __restrict__ poses,
                                                    const TopThresholds th, uint32_t* __restrict__ near) {
  const int P = (int)state[kTopMaxPasses].pool;
  const int id = (int)(blockIdx.x * kBlock + threadIdx.x);
  const int j = id / kTopWords, w = id % kTopWords;
  if (j >= P) return;
  uint32_t bits = 0u;
  if (32 * w < j) {
    double pj[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) pj[q] = poses[12 * (size_t)j + q];
    for (int k = 0; k < 32; ++k) {
      const int i = 32 * w + k;
      if (i >= j) break;
      double pi[12];
#pragma unroll
      for (int q = 0; q < 12; ++q) pi[q] = poses[12 * (size_t)i + q];
      if (top_near(pj, pi, th)) bits |= 1u << k;
    }
  }
  near[(size_t)j * kTopWords + w] = bits;
}

struct TopOutArgs {
  const TopState* state;
  const double* pool_key;
  const int32_t* pool_idx;
  const double* pool_poses;
  const uint32_t* near;
  TopRecord* rec;
  double* key;     // the rows, `rows` of each
  double* poses;
  int32_t* index;
  int32_t K, rows;
  int32_t suppress, want_poses;
};
__global__ __launch_bounds__(kBlock) void k_top_walk(const TopOutArgs a) {
  __shared__ int32_t keep[kTopPool];
  __shared__ int32_t tot[2];
  const int t = threadIdx.x;
  const TopState S = a.state[kTopMaxPasses];
  const int P = (int)S.pool;
  if (!a.suppress) {
    const int n = a.K < P ? a.K : P;
    for (int r = t; r < n; r += kBlock) keep[r] = r;
    if (t == 0) tot[0] = tot[1] = n;
  } else if (t < 64) {
    constexpr int kAhead = 8;  // rows loaded ahead of the walk (their addresses do not depend on it)
    uint32_t kept = 0u;        // lane l < kTopWords: word l of the kept mask
    int nk = 0, j = 0;
    while (j < P && nk < a.K) {
      uint32_t row[kAhead];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) row[u] = (t < kTopWords && j + u < P) ? a.near[(size_t)(j + u) * kTopWords + t] : 0u;
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        if (j < P && nk < a.K) {
          const bool hit = __ballot((row[u] & kept) != 0u) != 0ull;
          if (!hit) {
            if (t == (j >> 5)) kept |= 1u << (j & 31);
            if (t == 0) keep[nk] = j;
            ++nk;
          }
          ++j;
        }
      }
    }
    if (t == 0) {
      tot[0] = nk;
      tot[1] = j;
    }
  }
  __syncthreads();
  const int n_out = tot[0];
  if (t == 0) {
    a.rec->n_positive = S.n_positive;
    a.rec->n_out = n_out;
    a.rec->n_examined = tot[1];
  }
  for (int r = t; r < n_out; r += kBlock) {
    a.key[r] = a.pool_key[keep[r]];
    a.index[r] = a.pool_idx[keep[r]];
  }
  if (a.want_poses) {
    for (int i = t; i < 12 * a.rows; i += kBlock) {
      const int r = i / 12, q = i % 12;
      // behind the kept rows: the identity one metre ahead, rows the pair kernel runs over and nobody reads
      a.poses[i] = r < n_out ? a.pool_poses[12 * (size_t)keep[r] + q] : ((q == 0 || q == 5 || q == 10 || q == 11) ? 1.0 : 0.0);
    }
  }
}

}  // namespace

}  // namespace pfmpe

namespace pfmpe_impl {

namespace {
template <typename KT>
int top_select_t(pfmpe_ctx* c, unsigned char* d, const KT* keys, int N) {
  constexpr int kPasses = top_passes(TopKey<KT>::kBits);
  uint32_t* hist = (uint32_t*)(d + TopBuf::kHist);
  TopState* state = (TopState*)(d + TopBuf::kState);
  TopBlockCount* bc = (TopBlockCount*)(d + TopBuf::kBlockCount);
  uint64_t* cand_key = (uint64_t*)(d + TopBuf::kCandKey);
  uint32_t* cand_idx = (uint32_t*)(d + TopBuf::kCandIdx);
  const dim3 grid(top_blocks(N)), block(kBlock);
  for (int p = 0; p < kPasses; ++p) hipLaunchKernelGGL((k_top_hist<KT>), grid, block, 0, c->stream, keys, N, p, hist, state);
  hipLaunchKernelGGL((k_top_count<KT>), grid, block, 0, c->stream, keys, N, (const uint32_t*)hist, state, bc);
  hipLaunchKernelGGL((k_top_scatter<KT>), grid, block, 0, c->stream, keys, N, (const TopState*)state,
                     (const TopBlockCount*)bc, cand_key, cand_idx);
  hipLaunchKernelGGL((k_top_sort<KT>), dim3(1), dim3(kTopPool), 0, c->stream, (const TopState*)state,
                     (const uint64_t*)cand_key, (const uint32_t*)cand_idx, (double*)(d + TopBuf::kPoolKey),
                     (int32_t*)(d + TopBuf::kPoolIdx));
  HIPCHK(c, hipGetLastError());
  return PFMPE_OK;
}

enum { kTopKeyF32 = 0, kTopKeyF64 = 1, kTopKeyU32 = 2 };
// The selection on the context's stream: the scratch cleared, then the radix select over the N keys (`key_type` says
// what they are), the compaction and the sort.  Leaves the result state (state[kTopMaxPasses]), the ranked
// pool's particle indices (kPoolIdx) and keys as doubles (kPoolKey).  *pool_count: the device address of the pool's
// size.
int top_select_launch(pfmpe_ctx* c, unsigned char* d_top, const void* keys, int key_type, int N,
                      const uint32_t** pool_count) {
  HIPCHK(c, hipMemsetAsync(d_top, 0, TopBuf::kClear, c->stream));
  *pool_count = (const uint32_t*)(d_top + TopBuf::kState + kTopMaxPasses * sizeof(TopState) + offsetof(TopState, pool));
  switch (key_type) {
    case kTopKeyF64: return top_select_t<double>(c, d_top, (const double*)keys, N);
    case kTopKeyU32: return top_select_t<uint32_t>(c, d_top, (const uint32_t*)keys, N);
    default: return top_select_t<float>(c, d_top, (const float*)keys, N);
  }
}

// The rest, behind the regeneration of the pool's poses into kPoolPoses (skipped when neither suppression nor a pose
// row is wanted: poses = false): the near-matrix (suppression only), then one block that walks it and writes the
// record and the rows of the kept candidates for `rows` rows; pose rows n_out .. rows - 1 get a harmless constant
// (the pair kernel runs over `rows` rows: n_out is not known to the host yet).
int top_finish_launch(pfmpe_ctx* c, unsigned char* d_top, int K, int rows, const TopThresholds& th, bool poses) {
  const bool suppress = th.min_trans != 0.0 || th.min_rot != 0.0;
  const TopState* state = (const TopState*)(d_top + TopBuf::kState);
  uint32_t* near = (uint32_t*)(d_top + TopBuf::kNear);
  const double* pool_poses = (const double*)(d_top + TopBuf::kPoolPoses);
  if (suppress)
    hipLaunchKernelGGL(k_top_near, dim3(kTopPool * kTopWords / kBlock), dim3(kBlock), 0, c->stream, state, pool_poses, th, near);
  unsigned char* rec = d_top + TopBuf::kRecord;
  TopOutArgs a{};
  a.state = state;
  a.pool_key = (const double*)(d_top + TopBuf::kPoolKey);
  a.pool_idx = (const int32_t*)(d_top + TopBuf::kPoolIdx);
  a.pool_poses = pool_poses;
  a.near = near;
  a.rec = (TopRecord*)rec;
  a.key = (double*)(rec + TopRows::kKey);
  a.poses = (double*)(rec + TopRows::poses(rows));
  a.index = (int32_t*)(rec + TopRows::index(rows));
  a.K = K;
  a.rows = rows;
  a.suppress = suppress ? 1 : 0;
  a.want_poses = poses ? 1 : 0;
  hipLaunchKernelGGL(k_top_walk, dim3(1), dim3(kBlock), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  return PFMPE_OK;
}
}  // namespace

}  // namespace pfmpe_impl

// ======================================================================================= C-ABI
using namespace pfmpe_impl;

void pfmpe_default_top_params(pfmpe_top_params* p) {
  if (!p) return;
  p->key = PFMPE_TOP_BY_WEIGHT;
  p->K = 8;
  p->min_trans = 0.0;
  p->min_rot = 0.0;
}

int pfmpe_top_particles(pfmpe_ctx* c, const pfmpe_top_params* params, const pfmpe_assoc_in* in, pfmpe_top_out* out,
                        int32_t* index, double* key_value, double* poses, uint32_t* corr, int32_t* n_corr) {
  if (!c) return PFMPE_E_ARG;
  if (!params || !out) return fail(c, PFMPE_E_ARG, "top_particles: null params or out");
  const pfmpe_top_params prm = *params;
  if (prm.key != PFMPE_TOP_BY_WEIGHT && prm.key != PFMPE_TOP_BY_COUNT) return fail(c, PFMPE_E_ARG, "top_particles: bad key");
  if (prm.K < 0 || prm.K > PFMPE_TOP_MAX) return fail(c, PFMPE_E_ARG, "top_particles: K out of range");
  if (!(prm.min_trans >= 0.0) || !std::isfinite(prm.min_trans))
    return fail(c, PFMPE_E_ARG, "top_particles: min_trans must be finite and >= 0");
  if (!(prm.min_rot >= 0.0 && prm.min_rot <= M_PI)) return fail(c, PFMPE_E_ARG, "top_particles: min_rot outside [0, pi]");
  const double* blobs = nullptr;
  int B = 0;
  if (in) RET(resolve_blobs(c, "top_particles", in, &blobs, &B));
  if (!c->has_prior || !c->has_last) return fail(c, PFMPE_E_STATE, "top_particles: no step yet");
  if (prm.key == PFMPE_TOP_BY_COUNT) {
    if (!c->record_counts || !c->d_counts.get()) return fail(c, PFMPE_E_STATE, "top_particles: PFMPE_OPT_RECORD_COUNTS off");
    if (!c->last_accepted) return fail(c, PFMPE_E_STATE, "top_particles: last step did not resample");
  }
  if (in && !c->has_model) return fail(c, PFMPE_E_STATE, "top_particles: blobs given without a model");
  RET(set_device(c));
  RET(c->d_top.ensure(c, TopBuf::bytes()));
  RET(c->h_top.ensure(c, TopRows::bytes(PFMPE_TOP_MAX)));
  const int N = c->N;
  const int rows = std::min(prm.K, N);  // n_out <= min(K, n_positive): the rows the record is laid out for
  const TopThresholds th = top_thresholds(prm.min_trans, prm.min_rot);
  const bool suppress = prm.min_trans != 0.0 || prm.min_rot != 0.0;
  const bool pairs = in && rows > 0;
  const bool want_poses = suppress || pairs || (poses && rows > 0);
  unsigned char* d = c->d_top.get();

  const void* keys = c->d_w[c->last_kept_slot].get();
  int key_type = c->state_dtype == PFMPE_STATE_F64 ? kTopKeyF64 : kTopKeyF32;
  if (prm.key == PFMPE_TOP_BY_COUNT) {
    keys = c->d_counts.get();
    key_type = kTopKeyU32;
  }
  const uint32_t* pool_count = nullptr;
  RET(top_select_launch(c, d, keys, key_type, N, &pool_count));
  // the poses of the ranked pool only (all of it for the suppression walk, else the rows wanted), as k_regen makes
  // them: bracketed as aux like every regeneration
  if (want_poses)
    RET(dispatch_regen_list(c, c->last_kept_iter, c->d_state[c->last_prior_idx].get(), (const int32_t*)(d + TopBuf::kPoolIdx),
                            pool_count, suppress ? kTopPool : rows, (double*)(d + TopBuf::kPoolPoses)));
  RET(top_finish_launch(c, d, prm.K, rows, th, want_poses));
  unsigned char* rec = d + TopBuf::kRecord;
  if (pairs) {
    // the rows' pairs as pfmpe_get_pairs derives them: the blob table as assoc_prepare builds it, the pair kernel in
    // rows mode over the dense list of the kept rows' poses (it bounds its range by first / count alone; count is `rows`, the rows behind
    // n_out hold a constant pose and are not returned)
    const size_t tbytes = build_table(c, blobs, B, c->h_table.get());
    const GridHdr gh = *(const GridHdr*)(c->h_table.get() + grid_off(c, B));
    HIPCHK(c, hipMemcpyAsync(c->d_table.get(), c->h_table.get(), tbytes, hipMemcpyHostToDevice, c->stream));
    AssocArgs aa{};
    aa.dense = (const double*)(rec + TopRows::poses(rows));
    aa.corr = (uint32_t*)(rec + TopRows::corr(rows));
    aa.n_corr = (int32_t*)(rec + TopRows::n_corr(rows));
    aa.first = 0;
    aa.count = rows;
    RET(assoc_rows_launch(c, B, c->d_table.get(), tbytes, gh, aa));
  }
  // one read-back: the record and the rows (without the pair rows when no blobs were given)
  unsigned char* h = c->h_top.get();
  const size_t bytes = pairs ? TopRows::bytes(rows) : TopRows::n_corr(rows);
  HIPCHK(c, hipMemcpyAsync(h, rec, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  RET(harvest_timing(c));
  const TopRecord r = *(const TopRecord*)h;
  if (r.n_out < 0 || r.n_out > rows) return fail(c, PFMPE_E_STATE, "top_particles: inconsistent record");
  out->n = N;
  out->n_positive = r.n_positive;
  out->n_out = r.n_out;
  out->n_examined = r.n_examined;
  const size_t n = (size_t)r.n_out;
  if (index) std::memcpy(index, h + TopRows::index(rows), n * sizeof(int32_t));
  if (key_value) std::memcpy(key_value, h + TopRows::kKey, n * sizeof(double));
  if (poses) std::memcpy(poses, h + TopRows::poses(rows), n * 12 * sizeof(double));
  if (pairs && corr) std::memcpy(corr, h + TopRows::corr(rows), n * kPairRow * sizeof(uint32_t));
  if (pairs && n_corr) std::memcpy(n_corr, h + TopRows::n_corr(rows), n * sizeof(int32_t));
  return PFMPE_OK;
}

int pfmpe_host_top_suppress(const double* poses, int32_t P, int32_t K, double min_trans, double min_rot, int32_t* keep,
                            int32_t* n_out, int32_t* n_examined) {
  if (!keep || !n_out || !n_examined || P < 0 || (P > 0 && !poses) || K < 0 || K > PFMPE_TOP_MAX) return PFMPE_E_ARG;
  if (!(min_trans >= 0.0) || !std::isfinite(min_trans) || !(min_rot >= 0.0 && min_rot <= M_PI)) return PFMPE_E_ARG;
  for (size_t q = 0; q < 12 * (size_t)P; ++q)
    if (!std::isfinite(poses[q])) return PFMPE_E_ARG;
  top_walk(poses, P, K, top_thresholds(min_trans, min_rot), keep, n_out, n_examined);
  return PFMPE_OK;
}
