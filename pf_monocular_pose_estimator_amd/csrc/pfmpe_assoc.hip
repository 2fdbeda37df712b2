// pfmpe_assoc.hip — the k_assoc_votes instantiations (pfmpe_assoc_stats / pfmpe_get_pairs) and their launch: state
// type x kept set / resident prior x marker bucket x pruning option; the same instances of k_assoc_votes_multi
// (pfmpe_assoc_stats_multi), their launch and the batch's plan.  A TU of its own so they build beside the others.
#include "pf_likelihood.hpp"
#include "pf_roi.hpp"  // roi_stream_of_block (the batch)
#include "pfmpe_args.hpp"

namespace pfmpe {

// ---- LED-blob association of the cloud (pfmpe_assoc_stats / pfmpe_get_pairs; the definition is in include/pfmpe.h):
// every particle's pairs by the weighing kernels' per-lane path (project_markers, the NaN-at-origin rule,
// column_minima, score_minima<PAIRS>), then either one vote per pair into integer bins or the particle's row.
// DENSE = false: the resident prior through StateIO / the owner indices (fa.owner, fa.anc_in, fa.ld), exactly the
// rows k_export writes.  DENSE = true: N x 12 doubles, narrowed to T (exact: they are widened T values).  The bins
// are integers, so the order of the adds does not matter: returnless LDS adds per vote, then one device-scope add
// per non-zero bin and block into the table the host cleared.  No waits on other blocks.
// One block's share of that work: block blk of nblk walks the particles blk * kBlock + lane, + nblk * kBlock, ... of
// aa.first .. + aa.count.  The body of k_assoc_votes (fa from the kernel arguments) and of k_assoc_votes_multi (fa from
// the entry's descriptor); fa_words: where the frame constants are staged from (the head of that FrameArgsT).
template <typename T, typename SP, bool DENSE, int MAXM, bool PRUNE>
__device__ __forceinline__ void assoc_block(const FrameArgsT<T>& fa, const uint32_t* fa_words, const AssocArgs& aa,
                                            const unsigned char* __restrict__ table, const SP* __restrict__ st,
                                            const int blk, const int nblk, unsigned char* smem, LdsConst<T>& sc) {
  const int M = fa.M, B = fa.B;
  const int nbins = assoc_bins(M, B);
  const bool lds = aa.votes && aa.lds_votes;
  uint32_t* bins = (uint32_t*)(smem + BlobTable<T>::lds_bytes((size_t)fa.tbytes));
  copy_table(table, smem, (size_t)fa.tbytes);
  stage_consts_from<T>(fa_words, sc);
  if (lds)
    for (int i = threadIdx.x; i < nbins; i += kBlock) bins[i] = 0u;
  __syncthreads();  // table, constants and cleared bins visible
  const LdsBlobs<T> tb = view_table<T>(smem, B);
  const int64_t stride = (int64_t)nblk * kBlock;
  for (int64_t i = (int64_t)blk * kBlock + threadIdx.x; i < aa.count; i += stride) {
    const int64_t n = (int64_t)aa.first + i;
    T P[12];
    if constexpr (DENSE) {
#pragma unroll
      for (int q = 0; q < 12; ++q) P[q] = (T)aa.dense[12 * n + q];
    } else {
      const int64_t r = fa.owner ? (int64_t)fa.owner[n] : n;
#pragma unroll
      for (int q = 0; q < 12; ++q) P[q] = StateIO<T, SP>::load(st[plane_index<SP>(q, r, fa.ld)], fa.anc_in[q]);
    }
    T u[MAXM], v[MAXM];
    project_markers<T, MAXM>(fa, sc, P, u, v);
    uint32_t pairs[2 * MAXM];
#pragma unroll
    for (int q = 0; q < 2 * MAXM; ++q) pairs[q] = 0u;
    int np = 0;
    if (B > 0 && !nan_at_origin_tb(fa, tb, u[0], v[0])) {  // else the step's likelihood short-circuits: no pairs
      T m[MAXM];
      int r[MAXM];
      (void)column_minima<T, MAXM, PRUNE>(fa, u, v, tb, m, r);
      (void)score_minima<T, MAXM, true>(fa, m, r, pairs, &np);
    }
    if (aa.votes) {
      // each add through its own pointer (the LDS add as ds_add_u32 without a return value, not a flat atomic)
      auto vote = [&](int idx) {
        if (lds)
          (void)__hip_atomic_fetch_add(bins + idx, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else
          (void)__hip_atomic_fetch_add(aa.votes + idx, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      };
#pragma unroll
      for (int k = 0; k < MAXM; ++k)
        if (k < np) vote(((int)pairs[2 * k] - 1) * B + ((int)pairs[2 * k + 1] - 1));
      vote(M * B + np);
    } else {
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
      u32x4* row = (u32x4*)(aa.corr + (size_t)i * (2 * kMaxMarkers));
#pragma unroll
      for (int g = 0; g < 2 * kMaxMarkers / 4; ++g) {
        u32x4 w = {0u, 0u, 0u, 0u};
        if (4 * g < 2 * MAXM) {
          w.x = pairs[4 * g];
          w.y = pairs[4 * g + 1];
        }
        if (4 * g + 2 < 2 * MAXM) {
          w.z = pairs[4 * g + 2];
          w.w = pairs[4 * g + 3];
        }
        row[g] = w;
      }
      aa.n_corr[i] = np;
    }
  }
  if (lds) {
    __syncthreads();  // every wave's votes are in the bins
    for (int i = threadIdx.x; i < nbins; i += kBlock) {
      const uint32_t x = bins[i];
      if (x) (void)__hip_atomic_fetch_add(aa.votes + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

template <typename T, typename SP, bool DENSE, int MAXM, bool PRUNE>
__global__ __launch_bounds__(kBlock) void k_assoc_votes(const FrameArgsT<T> fa, const AssocArgs aa,
                                                       const unsigned char* __restrict__ table,
                                                       const SP* __restrict__ st) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ LdsConst<T> sc;
  assoc_block<T, SP, DENSE, MAXM, PRUNE>(fa, (const uint32_t*)__builtin_amdgcn_kernarg_segment_ptr(), aa, table, st,
                                         (int)blockIdx.x, (int)gridDim.x, smem, sc);
}

// ---- the votes of S entries in one batch (pfmpe_assoc_stats_multi).  One flat grid per kernel instance the batch
// needs (set kind x marker bucket x pruning option): a launch's head names its entries and the prefix of their blocks
// (entry g of the launch owns blocks first[g] .. first[g + 1], the single call's grid for its N), and a block finds
// its entry by one wave-wide comparison (roi_stream_of_block: the index is block-uniform, so the head and the
// descriptor are read with scalar loads).  The descriptor holds what the single kernel gets as arguments: the frame
// arguments, the entry's table in the batch's device image, its slice of the batch's bins, its particles and whether
// its bins fit in LDS behind its table.  The block's LDS is laid out for its own entry; the launch allocates the
// largest need among its entries.  Bins are integers and every entry has its own slice, so an entry's table does not
// depend on its neighbours or on the grid.  No waits on other blocks.
constexpr int kAssocMaxStreams = 64;
constexpr int kAssocMaxLaunches = 16;  // 2 set kinds x 4 marker buckets x 2 pruning options
static_assert(kAssocMaxStreams <= kRoiMaxStreams, "AssocHead::first is read by roi_stream_of_block");
struct AssocHead {  // one launch of the batch
  int32_t S, pad;
  int32_t first[kAssocMaxStreams + 1];  // first block of the launch's entry g; first[S] = all its blocks
  int32_t pad2;
  int32_t entry[kAssocMaxStreams];      // the batch index (descriptor) of the launch's entry g
};
template <typename T>
struct alignas(16) AssocDesc {
  FrameArgsT<T> fa;            // first: stage_consts_from reads its head (LdsConst layout)
  const unsigned char* table;  // the entry's blob table (fa.tbytes) in the batch's device image
  const void* st;              // the context's resident prior (SP planes)
  const double* dense;         // DENSE: the context's regenerated kept set, N x 12
  uint32_t* votes;             // the entry's bins in the batch's device table
  int32_t lds_votes, pad[3];
};
static_assert(sizeof(AssocHead) % 16 == 0 && sizeof(AssocDesc<float>) % 16 == 0 && sizeof(AssocDesc<double>) % 16 == 0,
              "the image keeps every part 16-byte aligned");
template <typename P>
__device__ __forceinline__ P* uniform_ptr(P* p) {  // a block-uniform pointer into scalar registers
  const uint64_t v = (uint64_t)p;
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return (P*)(((uint64_t)hi << 32) | lo);
}
template <typename T, typename SP, bool DENSE, int MAXM, bool PRUNE>
__global__ __launch_bounds__(kBlock) void k_assoc_votes_multi(const AssocHead* __restrict__ hd,
                                                             const AssocDesc<T>* __restrict__ descs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ LdsConst<T> sc;
  const int g = roi_stream_of_block(hd->first, hd->S, blockIdx.x);
  const int b0 = __builtin_amdgcn_readfirstlane(hd->first[g]);
  const int b1 = __builtin_amdgcn_readfirstlane(hd->first[g + 1]);
  const AssocDesc<T>& d = descs[__builtin_amdgcn_readfirstlane(hd->entry[g])];
  AssocArgs aa{};
  aa.dense = uniform_ptr(d.dense);
  aa.votes = uniform_ptr(d.votes);
  aa.first = 0;
  aa.count = __builtin_amdgcn_readfirstlane(d.fa.N);
  aa.lds_votes = __builtin_amdgcn_readfirstlane(d.lds_votes);
  assoc_block<T, SP, DENSE, MAXM, PRUNE>(d.fa, (const uint32_t*)&d.fa, aa, uniform_ptr(d.table),
                                         (const SP*)uniform_ptr(d.st), (int)blockIdx.x - b0, b1 - b0, smem, sc);
}

}  // namespace pfmpe

namespace pfmpe_impl {

namespace {
template <typename T, typename SP, bool DENSE, int MAXM>
void assoc_launch_p(pfmpe_ctx* c, const FrameArgsT<T>& fa, const AssocArgs& aa, const unsigned char* table, dim3 grid,
                    size_t lds) {
  const SP* st = (const SP*)c->d_state[c->prior_idx].get();
  if (c->prune)
    hipLaunchKernelGGL((k_assoc_votes<T, SP, DENSE, MAXM, true>), grid, dim3(kBlock), lds, c->stream, fa, aa, table, st);
  else
    hipLaunchKernelGGL((k_assoc_votes<T, SP, DENSE, MAXM, false>), grid, dim3(kBlock), lds, c->stream, fa, aa, table, st);
}

// the marker buckets of dispatch_m
template <typename T, typename SP, bool DENSE>
void assoc_launch_m(pfmpe_ctx* c, const FrameArgsT<T>& fa, const AssocArgs& aa, const unsigned char* table, dim3 grid,
                    size_t lds) {
  visit_m(fa.M, fa.M == kExactM,
          [&](auto m) { assoc_launch_p<T, SP, DENSE, decltype(m)::value>(c, fa, aa, table, grid, lds); });
}

template <typename T, typename SP>
int assoc_launch_t(pfmpe_ctx* c, int B, const unsigned char* table, size_t tbytes, const GridHdr& gh, AssocArgs aa) {
  // the likelihood's arguments as a frame with these blobs would get them (model, K, tol, tol_PF, the pruning
  // window, the prior's owner indices and anchor); the motion-model part is not read
  pfmpe_frame_in fin{};
  fin.B = B;
  fin.it_since_init = 1;
  fin.dt = 1.0;
  FrameArgsT<T> fa = build_args<T>(c, &fin);
  fa.tbytes = (int32_t)tbytes;
  fa.grid = grid_args<T>(gh, B, (float)fa.tolq);
  const size_t tlds = BlobTable<T>::lds_bytes(tbytes);
  const size_t vbytes = (size_t)assoc_bins(fa.M, B) * sizeof(uint32_t);
  aa.lds_votes = (aa.votes && !(c->diag & kDiagAssocDirect) && tlds + vbytes + sizeof(LdsConst<T>) <= kAssocLdsLimit) ? 1 : 0;
  const size_t lds = tlds + (aa.lds_votes ? vbytes : 0);
  if (lds + sizeof(LdsConst<T>) > kAssocLdsLimit) return fail(c, PFMPE_E_CAP, "assoc: blob table exceeds the LDS");
  const int nb = (aa.count + kBlock - 1) / kBlock;
  const dim3 grid(nb < kAssocMaxBlocks ? nb : kAssocMaxBlocks);
  if (aa.dense)
    assoc_launch_m<T, T, true>(c, fa, aa, table, grid, lds);
  else
    assoc_launch_m<T, SP, false>(c, fa, aa, table, grid, lds);
  HIPCHK(c, hipGetLastError());
  return PFMPE_OK;
}
}  // namespace

int assoc_launch(pfmpe_ctx* c, int B, const unsigned char* table, size_t tbytes, const GridHdr& gh, AssocArgs aa) {
  if (aa.count < 1) return PFMPE_OK;
  return visit_state(c, [&](auto s) {
    return assoc_launch_t<typename decltype(s)::T, typename decltype(s)::SP>(c, B, table, tbytes, gh, aa);
  });
}

// ---- the batch (pfmpe_assoc_stats_multi)
namespace {
static_assert(PFMPE_ASSOC_MAX_STREAMS == kAssocMaxStreams && PFMPE_ASSOC_MAX_LAUNCHES == kAssocMaxLaunches,
              "batch capacity mismatch");
template <typename T, typename SP, bool DENSE>
void assoc_multi_launch_m(pfmpe_ctx* c0, int M, bool prune, dim3 grid, size_t lds, const AssocHead* hd,
                          const AssocDesc<T>* descs) {
  visit_m(M, M == kExactM, [&](auto m) {
    constexpr int MAXM = decltype(m)::value;
    if (prune)
      hipLaunchKernelGGL((k_assoc_votes_multi<T, SP, DENSE, MAXM, true>), grid, dim3(kBlock), lds, c0->stream, hd, descs);
    else
      hipLaunchKernelGGL((k_assoc_votes_multi<T, SP, DENSE, MAXM, false>), grid, dim3(kBlock), lds, c0->stream, hd, descs);
  });
}

template <typename T, typename SP>
int assoc_multi_run_t(pfmpe_ctx* c0, const AssocMultiEntry* e, int S, int launches, unsigned char* himg,
                      unsigned char* dimg, size_t img_bytes, uint32_t* dbins, size_t bins_words) {
  AssocHead* heads = (AssocHead*)himg;
  AssocDesc<T>* descs = (AssocDesc<T>*)(himg + kAssocMaxLaunches * sizeof(AssocHead));
  size_t lds[kAssocMaxLaunches] = {0};
  int lead[kAssocMaxLaunches];  // a launch's first entry: its instance
  std::memset(heads, 0, (size_t)launches * sizeof(AssocHead));
  for (int s = 0; s < S; ++s) {
    const AssocMultiEntry& en = e[s];
    const pfmpe_ctx* c = en.c;
    // the frame arguments and the LDS need as the single launch forms them (assoc_launch_t)
    pfmpe_frame_in fin{};
    fin.B = en.B;
    fin.it_since_init = 1;
    fin.dt = 1.0;
    AssocDesc<T>& d = descs[s];
    std::memset(&d, 0, sizeof(d));
    d.fa = build_args<T>(c, &fin);
    d.fa.tbytes = (int32_t)en.tbytes;
    d.fa.grid = grid_args<T>(en.gh, en.B, (float)d.fa.tolq);
    d.table = dimg + en.table_off;
    d.st = c->d_state[c->prior_idx].get();
    d.dense = en.which == PFMPE_ASSOC_PROPAGATED ? c->d_xfer.get() : nullptr;
    d.votes = dbins + en.bins_off;
    d.lds_votes = en.lds_votes;
    const size_t need = BlobTable<T>::lds_bytes(en.tbytes) +
                        (en.lds_votes ? (size_t)assoc_bins(c->M, en.B) * sizeof(uint32_t) : (size_t)0);
    AssocHead& h = heads[en.launch];
    if (h.S == 0) lead[en.launch] = s;
    h.first[h.S] = en.first_block;
    h.first[h.S + 1] = en.first_block + en.blocks;
    h.entry[h.S] = s;
    h.S += 1;
    lds[en.launch] = std::max(lds[en.launch], need);
  }
  // one upload (heads, descriptors, tables), one memset of all bins, one launch per instance
  HIPCHK(c0, hipMemcpyAsync(dimg, himg, img_bytes, hipMemcpyHostToDevice, c0->stream));
  HIPCHK(c0, hipMemsetAsync(dbins, 0, bins_words * sizeof(uint32_t), c0->stream));
  const AssocHead* dheads = (const AssocHead*)dimg;
  const AssocDesc<T>* ddescs = (const AssocDesc<T>*)(dimg + kAssocMaxLaunches * sizeof(AssocHead));
  for (int l = 0; l < launches; ++l) {
    const AssocHead& h = heads[l];
    const AssocMultiEntry& en = e[lead[l]];
    const dim3 grid(h.first[h.S]);
    if (en.which == PFMPE_ASSOC_PROPAGATED)
      assoc_multi_launch_m<T, T, true>(c0, en.c->M, en.c->prune, grid, lds[l], dheads + l, ddescs);
    else
      assoc_multi_launch_m<T, SP, false>(c0, en.c->M, en.c->prune, grid, lds[l], dheads + l, ddescs);
  }
  HIPCHK(c0, hipGetLastError());
  return PFMPE_OK;
}
}  // namespace

size_t assoc_multi_tables_off(const pfmpe_ctx* c0, int S) {
  return visit_state(c0, [&](auto s) {
    const size_t n = kAssocMaxLaunches * sizeof(AssocHead) + (size_t)S * sizeof(AssocDesc<typename decltype(s)::T>);
    return (n + 255) / 256 * 256;
  });
}

int assoc_multi_run(pfmpe_ctx* c0, const AssocMultiEntry* e, int S, int launches, unsigned char* himg,
                    unsigned char* dimg, size_t img_bytes, uint32_t* dbins, size_t bins_words) {
  return visit_state(c0, [&](auto s) {
    return assoc_multi_run_t<typename decltype(s)::T, typename decltype(s)::SP>(c0, e, S, launches, himg, dimg,
                                                                                img_bytes, dbins, bins_words);
  });
}

// ---- pfmpe_host_assoc_plan: the layout above, from the entries' shapes alone
int assoc_plan(const int32_t* N, const int32_t* M, const int32_t* B, const int32_t* which, const int32_t* prune,
               const int32_t* table_bytes, int S, int state_dtype, pfmpe_assoc_plan* plan, pfmpe_assoc_plan_total* total,
               int* bad) {
  if (!N || !M || !B || !plan || !total || S < 1) return PFMPE_E_ARG;
  if (state_dtype != PFMPE_STATE_F32 && state_dtype != PFMPE_STATE_F64 && state_dtype != PFMPE_STATE_F16) return PFMPE_E_ARG;
  if (S > PFMPE_ASSOC_MAX_STREAMS) return PFMPE_E_CAP;
  const bool f64 = state_dtype == PFMPE_STATE_F64;
  const size_t csize = f64 ? sizeof(LdsConst<double>) : sizeof(LdsConst<float>);
  pfmpe_assoc_plan out[PFMPE_ASSOC_MAX_STREAMS];
  pfmpe_assoc_plan_total tot{};
  int key_of[kAssocMaxLaunches];
  int64_t words = 0;
  for (int s = 0; s < S; ++s) {
    if (bad) *bad = s;
    if (N[s] < 1 || M[s] < 1 || M[s] > kMaxMarkers || B[s] < 0) return PFMPE_E_ARG;
    if (which && which[s] != PFMPE_ASSOC_PROPAGATED && which[s] != PFMPE_ASSOC_POSTERIOR) return PFMPE_E_ARG;
    if (table_bytes && table_bytes[s] < 0) return PFMPE_E_ARG;
    if (B[s] > kMaxBlobs) return PFMPE_E_CAP;
    // the table's size: the caller's (a built table), else that of a table without a grid
    const size_t tbytes = table_bytes ? (size_t)table_bytes[s]
                          : f64       ? BlobTable<double>::total_bytes(B[s], 0, 0)
                                      : BlobTable<float>::total_bytes(B[s], 0, 0);
    const size_t tlds = f64 ? BlobTable<double>::lds_bytes(tbytes) : BlobTable<float>::lds_bytes(tbytes);
    if (tlds + csize > kAssocLdsLimit) return PFMPE_E_CAP;
    const size_t vbytes = (size_t)assoc_bins(M[s], B[s]) * sizeof(uint32_t);
    const int nb = (N[s] + kBlock - 1) / kBlock;
    const int bucket = visit_m(M[s], M[s] == kExactM, [](auto m) { return (int)decltype(m)::value; });
    const int key = ((which ? which[s] : PFMPE_ASSOC_POSTERIOR) == PFMPE_ASSOC_PROPAGATED ? 64 : 0) + 2 * bucket +
                    ((prune ? prune[s] != 0 : true) ? 1 : 0);
    int l = 0;
    while (l < tot.launches && key_of[l] != key) ++l;
    if (l == tot.launches) key_of[tot.launches++] = key;
    pfmpe_assoc_plan& p = out[s];
    p.blocks = nb < kAssocMaxBlocks ? nb : kAssocMaxBlocks;
    p.first_block = tot.launch_blocks[l];
    p.launch = l;
    p.lds_votes = tlds + vbytes + csize <= kAssocLdsLimit ? 1 : 0;
    words = (words + 3) / 4 * 4;
    p.bins_offset = words;
    words += assoc_bins(M[s], B[s]);
    tot.launch_blocks[l] += p.blocks;
  }
  tot.bins_words = words;
  std::memcpy(plan, out, (size_t)S * sizeof(pfmpe_assoc_plan));
  *total = tot;
  return PFMPE_OK;
}

}  // namespace pfmpe_impl
