// pfmpe_assoc.hip — LED-blob association of the cloud: k_assoc_votes (in rows mode: pfmpe_get_pairs, and the rows
// launch that pfmpe_refine_cloud / pfmpe_top_particles use) and k_assoc_votes_multi (pfmpe_assoc_stats_multi;
// pfmpe_assoc_stats is a batch of one), each per state type x kept set / resident prior x marker bucket x pruning
// option; the batch's plan, the host summary and gate, and the entry points.  A TU of its own so the instances build
// beside the others.
#include "pf_batch.hpp"
#include "pf_likelihood.hpp"
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

// ---- the votes of S entries in one batch (pfmpe_assoc_stats_multi; S = 1: pfmpe_assoc_stats).  One flat grid per
// kernel instance the batch needs (set kind x marker bucket x pruning option): a launch's head names its entries and
// the prefix of their blocks (entry g of the launch owns blocks first[g] .. first[g + 1], a block per 256 of its N
// particles up to kAssocMaxBlocks), and a block finds its entry by one wave-wide comparison (batch_stream_of_block: the
// index is block-uniform, so the head and the descriptor are read with scalar loads).  The descriptor holds what
// k_assoc_votes gets as arguments: the frame arguments, the entry's table in the batch's device image, its slice of
// the batch's bins, its particles and whether its bins fit in LDS behind its table.  The block's LDS is laid out for
// its own entry; the launch allocates the largest need among its entries.  Bins are integers and every entry has its
// own slice, so an entry's table does not depend on its neighbours or on the grid.  No waits on other blocks.
constexpr int kAssocMaxStreams = 64;
constexpr int kAssocMaxLaunches = 16;  // 2 set kinds x 4 marker buckets x 2 pruning options
static_assert(kAssocMaxStreams <= kBatchMaxStreams, "AssocHead::first is read by batch_stream_of_block");
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
  const int g = batch_stream_of_block(hd->first, hd->S, blockIdx.x);
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
// The likelihood's arguments as a frame with these blobs would get them (model, K, tol, tol_PF, the pruning window,
// the prior's owner indices and anchor), for the blob table of tbytes with grid header gh; the motion-model part is not
// read.
template <typename T>
FrameArgsT<T> assoc_frame_args(const pfmpe_ctx* c, int B, size_t tbytes, const GridHdr& gh) {
  pfmpe_frame_in fin{};
  fin.B = B;
  fin.it_since_init = 1;
  fin.dt = 1.0;
  FrameArgsT<T> fa = build_args<T>(c, &fin);
  fa.tbytes = (int32_t)tbytes;
  fa.grid = grid_args<T>(gh, B, (float)fa.tolq);
  return fa;
}

// The workgroup's LDS for a table of tbytes and nbins bins (f64: the compute type is double): the table, behind it the
// bins when they fit and are wanted, and the frame constants, kAssocLdsLimit in all.
struct AssocLds {
  size_t table;   // the table's LDS bytes
  bool ok, bins;  // the table fits beside the constants; the bins fit behind it as well
  size_t launch;  // the launch's dynamic LDS
};
AssocLds assoc_lds(bool f64, size_t tbytes, int nbins, bool want_bins) {
  const size_t csize = f64 ? sizeof(LdsConst<double>) : sizeof(LdsConst<float>);
  const size_t vbytes = (size_t)nbins * sizeof(uint32_t);
  AssocLds l;
  l.table = f64 ? BlobTable<double>::lds_bytes(tbytes) : BlobTable<float>::lds_bytes(tbytes);
  l.ok = l.table + csize <= kAssocLdsLimit;
  l.bins = l.table + vbytes + csize <= kAssocLdsLimit;
  l.launch = l.table + (l.bins && want_bins ? vbytes : 0);
  return l;
}

// the marker buckets of dispatch_m and the pruning option
template <typename T, typename SP, bool DENSE>
void assoc_rows_launch_m(pfmpe_ctx* c, const FrameArgsT<T>& fa, const AssocArgs& aa, const unsigned char* table, dim3 grid,
                         size_t lds) {
  const SP* st = (const SP*)c->d_state[c->prior_idx].get();
  visit_m(fa.M, fa.M == kExactM, [&](auto m) {
    constexpr int MAXM = decltype(m)::value;
    if (c->prune)
      hipLaunchKernelGGL((k_assoc_votes<T, SP, DENSE, MAXM, true>), grid, dim3(kBlock), lds, c->stream, fa, aa, table, st);
    else
      hipLaunchKernelGGL((k_assoc_votes<T, SP, DENSE, MAXM, false>), grid, dim3(kBlock), lds, c->stream, fa, aa, table, st);
  });
}
}  // namespace

int assoc_rows_launch(pfmpe_ctx* c, int B, const unsigned char* table, size_t tbytes, const GridHdr& gh, AssocArgs aa) {
  if (aa.count < 1) return PFMPE_OK;
  aa.votes = nullptr;  // rows mode: no bins
  aa.lds_votes = 0;
  return visit_state(c, [&](auto s) {
    using T = typename decltype(s)::T;
    using SP = typename decltype(s)::SP;
    const FrameArgsT<T> fa = assoc_frame_args<T>(c, B, tbytes, gh);
    const AssocLds l = assoc_lds(sizeof(T) == 8, tbytes, 0, false);
    if (!l.ok) return fail(c, PFMPE_E_CAP, "assoc: blob table exceeds the LDS");
    const int nb = (aa.count + kBlock - 1) / kBlock;
    const dim3 grid(nb < kAssocMaxBlocks ? nb : kAssocMaxBlocks);
    if (aa.dense)
      assoc_rows_launch_m<T, T, true>(c, fa, aa, table, grid, l.launch);
    else
      assoc_rows_launch_m<T, SP, false>(c, fa, aa, table, grid, l.launch);
    HIPCHK(c, hipGetLastError());
    return (int)PFMPE_OK;
  });
}

int assoc_prepare(pfmpe_ctx* c, const char* who, int which, const pfmpe_assoc_in* in, const double** blobs_out,
                  int* B_out, size_t* tbytes, GridHdr* gh, AssocArgs* aa) {
  const std::string w(who);
  if (!in || (which != PFMPE_ASSOC_PROPAGATED && which != PFMPE_ASSOC_POSTERIOR))
    return fail(c, PFMPE_E_ARG, w + ": bad arguments");
  const double* blobs = nullptr;
  int B = 0;
  RET(resolve_blobs(c, w, in, &blobs, &B));
  if (!c->has_model || !c->has_prior) return fail(c, PFMPE_E_STATE, w + ": set_model and a particle set first");
  if (which == PFMPE_ASSOC_PROPAGATED && !c->has_last) return fail(c, PFMPE_E_STATE, w + "(propagated): no step yet");
  RET(set_device(c));
  *tbytes = build_table(c, blobs, B, c->h_table.get());
  *gh = *(const GridHdr*)(c->h_table.get() + grid_off(c, B));
  HIPCHK(c, hipMemcpyAsync(c->d_table.get(), c->h_table.get(), *tbytes, hipMemcpyHostToDevice, c->stream));
  *aa = AssocArgs{};
  if (which == PFMPE_ASSOC_PROPAGATED) {
    RET(ensure_xfer(c));
    RET(dispatch_regen(c, c->last_kept_iter, c->d_state[c->last_prior_idx].get(), c->d_xfer.get()));
    aa->dense = c->d_xfer.get();
  }
  *blobs_out = blobs;
  *B_out = B;
  return PFMPE_OK;
}

// ---- the batch (pfmpe_assoc_stats_multi, and pfmpe_assoc_stats as a batch of one)
namespace {
static_assert(PFMPE_ASSOC_MAX_STREAMS == kAssocMaxStreams && PFMPE_ASSOC_MAX_LAUNCHES == kAssocMaxLaunches,
              "batch capacity mismatch");
// The layout of a batch from the entries' shapes alone (pfmpe_host_assoc_plan; which, prune, table_bytes may be null);
// *bad, when given: the entry an error is about.  The only place that lays a batch out.
int assoc_plan(const int32_t* N, const int32_t* M, const int32_t* B, const int32_t* which, const int32_t* prune,
               const int32_t* table_bytes, int S, int state_dtype, pfmpe_assoc_plan* plan, pfmpe_assoc_plan_total* total,
               int* bad) {
  if (!N || !M || !B || !plan || !total || S < 1) return PFMPE_E_ARG;
  if (state_dtype != PFMPE_STATE_F32 && state_dtype != PFMPE_STATE_F64 && state_dtype != PFMPE_STATE_F16) return PFMPE_E_ARG;
  if (S > PFMPE_ASSOC_MAX_STREAMS) return PFMPE_E_CAP;
  const bool f64 = state_dtype == PFMPE_STATE_F64;
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
    const AssocLds l = assoc_lds(f64, tbytes, assoc_bins(M[s], B[s]), true);
    if (!l.ok) return PFMPE_E_CAP;
    const int nb = (N[s] + kBlock - 1) / kBlock;
    const int bucket = visit_m(M[s], M[s] == kExactM, [](auto m) { return (int)decltype(m)::value; });
    const int key = ((which ? which[s] : PFMPE_ASSOC_POSTERIOR) == PFMPE_ASSOC_PROPAGATED ? 64 : 0) + 2 * bucket +
                    ((prune ? prune[s] != 0 : true) ? 1 : 0);
    int ln = 0;
    while (ln < tot.launches && key_of[ln] != key) ++ln;
    if (ln == tot.launches) key_of[tot.launches++] = key;
    pfmpe_assoc_plan& p = out[s];
    p.blocks = nb < kAssocMaxBlocks ? nb : kAssocMaxBlocks;
    p.first_block = tot.launch_blocks[ln];
    p.launch = ln;
    p.lds_votes = l.bins ? 1 : 0;
    words = (words + 3) / 4 * 4;
    p.bins_offset = words;
    words += assoc_bins(M[s], B[s]);
    tot.launch_blocks[ln] += p.blocks;
  }
  tot.bins_words = words;
  std::memcpy(plan, out, (size_t)S * sizeof(pfmpe_assoc_plan));
  *total = tot;
  return PFMPE_OK;
}

// One checked entry of a batch: what it asks for, then its built table and its place in the batch.  The leader's
// pinned image and its device copy hold, in this order: a head for each launch the batch can need (assoc_heads_bytes),
// the S descriptors, then every entry's blob table (assoc_tables_off onwards, each 16-byte aligned); the bins of all
// entries follow as one table.
struct AssocEntry {
  int32_t which, B;
  const double* blobs;       // the B blobs the entry means (resolve_blobs)
  size_t tbytes, table_off;  // the entry's built table: size, byte offset in the image
  GridHdr gh;                // its grid header
  pfmpe_assoc_plan plan;     // its launch, blocks and bins (lds_votes: 0 also under kDiagAssocDirect)
};
size_t assoc_heads_bytes(int S) { return (size_t)std::min(S, kAssocMaxLaunches) * sizeof(AssocHead); }
size_t assoc_tables_off(const pfmpe_ctx* c0, int S) {
  return visit_state(c0, [&](auto s) {
    const size_t n = assoc_heads_bytes(S) + (size_t)S * sizeof(AssocDesc<typename decltype(s)::T>);
    return (n + 255) / 256 * 256;
  });
}
// the largest table build_table can write for B blobs of this context's type (the finest grid B may get, full lists)
size_t assoc_table_bound(const pfmpe_ctx* c, int B) {
  return visit_state(c, [&](auto s) {
    return BlobTable<typename decltype(s)::T>::total_bytes(B, B >= kGridFineMinBlobs ? kGridMaxCells : kGridCoarseCells,
                                                           kGridMaxEntries);
  });
}

template <typename T, typename SP, bool DENSE>
void assoc_votes_launch_m(pfmpe_ctx* c0, int M, bool prune, dim3 grid, size_t lds, const AssocHead* hd,
                          const AssocDesc<T>* descs) {
  visit_m(M, M == kExactM, [&](auto m) {
    constexpr int MAXM = decltype(m)::value;
    if (prune)
      hipLaunchKernelGGL((k_assoc_votes_multi<T, SP, DENSE, MAXM, true>), grid, dim3(kBlock), lds, c0->stream, hd, descs);
    else
      hipLaunchKernelGGL((k_assoc_votes_multi<T, SP, DENSE, MAXM, false>), grid, dim3(kBlock), lds, c0->stream, hd, descs);
  });
}

// The heads and descriptors of a planned batch into himg (device addresses: the image's copy at dimg, the bins at
// dbins); lds[l]: the dynamic LDS of launch l, the largest need among its entries.  A PROPAGATED entry reads its
// context's d_xfer.
template <typename T>
void assoc_votes_fill(pfmpe_ctx* const* ctxs, const AssocEntry* e, int S, int launches, unsigned char* himg,
                      unsigned char* dimg, uint32_t* dbins, size_t* lds) {
  AssocHead* heads = (AssocHead*)himg;
  AssocDesc<T>* descs = (AssocDesc<T>*)(himg + assoc_heads_bytes(S));
  std::memset(heads, 0, (size_t)launches * sizeof(AssocHead));
  for (int s = 0; s < S; ++s) {
    const AssocEntry& en = e[s];
    const pfmpe_ctx* c = ctxs[s];
    AssocDesc<T>& d = descs[s];
    std::memset(&d, 0, sizeof(d));
    d.fa = assoc_frame_args<T>(c, en.B, en.tbytes, en.gh);
    d.table = dimg + en.table_off;
    d.st = c->d_state[c->prior_idx].get();
    d.dense = en.which == PFMPE_ASSOC_PROPAGATED ? c->d_xfer.get() : nullptr;
    d.votes = dbins + en.plan.bins_offset;
    d.lds_votes = en.plan.lds_votes;
    AssocHead& h = heads[en.plan.launch];
    h.first[h.S] = en.plan.first_block;
    h.first[h.S + 1] = en.plan.first_block + en.plan.blocks;
    h.entry[h.S] = s;
    h.S += 1;
    lds[en.plan.launch] = std::max(lds[en.plan.launch],
                                   assoc_lds(sizeof(T) == 8, en.tbytes, assoc_bins(c->M, en.B), en.plan.lds_votes != 0).launch);
  }
}
// one k_assoc_votes_multi launch per planned launch on ctxs[0]'s stream: the instance of the launch's first entry
template <typename T, typename SP>
void assoc_votes_launch(pfmpe_ctx* const* ctxs, const AssocEntry* e, int S, int launches, const unsigned char* himg,
                        const unsigned char* dimg, const size_t* lds) {
  const AssocHead* heads = (const AssocHead*)himg;
  const AssocHead* dheads = (const AssocHead*)dimg;
  const AssocDesc<T>* ddescs = (const AssocDesc<T>*)(dimg + assoc_heads_bytes(S));
  for (int ln = 0; ln < launches; ++ln) {
    const AssocHead& h = heads[ln];
    const pfmpe_ctx* c = ctxs[h.entry[0]];
    const dim3 grid(h.first[h.S]);
    if (e[h.entry[0]].which == PFMPE_ASSOC_PROPAGATED)
      assoc_votes_launch_m<T, T, true>(ctxs[0], c->M, c->prune, grid, lds[ln], dheads + ln, ddescs);
    else
      assoc_votes_launch_m<T, SP, false>(ctxs[0], c->M, c->prune, grid, lds[ln], dheads + ln, ddescs);
  }
}

// The record and the table of one entry from its bins as the kernel leaves them (M x B votes, then the M + 1 bins of
// the pair count), for N particles; votes may be null.  false: the rows do not sum to one n.
bool assoc_epilogue(const uint32_t* bins, int M, int B, int N, pfmpe_assoc_out* out, uint32_t* votes) {
  // column 0 is not voted: n minus the row's votes
  std::vector<uint32_t> tab((size_t)M * (B + 1));
  for (int m = 0; m < M; ++m) {
    uint32_t sum = 0;
    for (int b = 0; b < B; ++b) {
      tab[(size_t)m * (B + 1) + 1 + b] = bins[(size_t)m * B + b];
      sum += bins[(size_t)m * B + b];
    }
    tab[(size_t)m * (B + 1)] = (uint32_t)N - sum;
  }
  pfmpe_assoc_out o;
  if (pfmpe_host_assoc_summary(tab.data(), M, B, &o) != PFMPE_OK) return false;
  for (int k = 0; k <= M; ++k) o.npairs_hist[k] = bins[(size_t)M * B + k];
  o.n_any = (int64_t)N - (int64_t)o.npairs_hist[0];
  *out = o;
  if (votes) std::memcpy(votes, tab.data(), tab.size() * sizeof(uint32_t));
  return true;
}

// The votes of S checked entries (e[s].which / B / blobs of ctxs[s]), 1 <= S <= kAssocMaxStreams, as one batch on
// ctxs[0]'s stream: pfmpe_assoc_stats_multi and, as a batch of one, pfmpe_assoc_stats.  Errors begin with `who`; about
// an entry, the batch's name the stream and the single call's are the texts it always had.
int assoc_run(pfmpe_ctx* const* ctxs, int S, AssocEntry* e, pfmpe_assoc_out* out, uint32_t* const* votes,
              const std::string& who, bool single) {
  pfmpe_ctx* c0 = ctxs[0];
  auto at = [&](int s) { return single ? who + ": " : who + ": stream " + std::to_string(s) + ": "; };
  BatchMembers members(who.c_str(), S);  // flagged: a context with a PROPAGATED entry (all its entries read one regenerated set)
  for (int s = 0; s < S; ++s) members.add(ctxs[s], e[s].which == PFMPE_ASSOC_PROPAGATED);
  RET(set_device(c0));
  // ---- the image: every entry's table, built in the leader's pinned block behind the heads and descriptors (host
  // work: nothing is on the device yet).  The block holds the largest table each entry can get.
  const size_t tables_off = assoc_tables_off(c0, S);
  size_t cap = tables_off;
  for (int s = 0; s < S; ++s) cap += align16(assoc_table_bound(c0, e[s].B));
  {
    size_t bins_bound = 0;  // the batch's bins, each entry's start rounded up to 4 words
    for (int s = 0; s < S; ++s) bins_bound += (((size_t)assoc_bins(ctxs[s]->M, e[s].B) + 3) & ~(size_t)3) * sizeof(uint32_t);
    const size_t need = (cap + 255) / 256 * 256 + bins_bound;
    RET(c0->h_assocm.grow(c0, need, need * 2));
  }
  unsigned char* himg = c0->h_assocm.get();
  int32_t Ns[PFMPE_ASSOC_MAX_STREAMS], Ms[PFMPE_ASSOC_MAX_STREAMS], Bs[PFMPE_ASSOC_MAX_STREAMS], Ws[PFMPE_ASSOC_MAX_STREAMS],
      Ps[PFMPE_ASSOC_MAX_STREAMS], Ts[PFMPE_ASSOC_MAX_STREAMS];
  size_t img_bytes = tables_off;
  for (int s = 0; s < S; ++s) {
    const pfmpe_ctx* c = ctxs[s];
    e[s].table_off = img_bytes;
    e[s].tbytes = build_table(c, e[s].blobs, e[s].B, himg + img_bytes);
    e[s].gh = *(const GridHdr*)(himg + img_bytes + grid_off(c, e[s].B));
    img_bytes += align16(e[s].tbytes);
    Ns[s] = c->N;
    Ms[s] = c->M;
    Bs[s] = e[s].B;
    Ws[s] = e[s].which;
    Ps[s] = c->prune ? 1 : 0;
    Ts[s] = (int32_t)e[s].tbytes;
  }
  pfmpe_assoc_plan plan[PFMPE_ASSOC_MAX_STREAMS];
  pfmpe_assoc_plan_total total{};
  int bad = 0;  // (S, the counts and B were checked by the caller: what is left is a table that exceeds the LDS)
  if (const int r_ = assoc_plan(Ns, Ms, Bs, Ws, Ps, Ts, S, c0->state_dtype, plan, &total, &bad))
    return fail(c0, r_, (single ? std::string("assoc: ") : at(bad)) + "blob table exceeds the LDS");
  for (int s = 0; s < S; ++s) {
    e[s].plan = plan[s];
    if (ctxs[s]->diag & kDiagAssocDirect) e[s].plan.lds_votes = 0;
  }
  // the device scratch: the image, then the bins (nothing of an earlier batch is pending: the call is blocking)
  const size_t bins_at = (img_bytes + 255) / 256 * 256;
  const size_t bins_bytes = (size_t)total.bins_words * sizeof(uint32_t);
  RET(c0->d_assocm.grow(c0, bins_at + bins_bytes, (bins_at + bins_bytes) * 2));
  // one upload (heads, descriptors, tables) and one memset of all bins, ahead of the leader's kernels: a copy behind
  // the regeneration launch would wait for it across engines, 11 us per PROPAGATED call at C2
  uint32_t* dbins = (uint32_t*)(c0->d_assocm.get() + bins_at);
  size_t lds[kAssocMaxLaunches] = {0};
  visit_state(c0, [&](auto s) {
    assoc_votes_fill<typename decltype(s)::T>(ctxs, e, S, total.launches, himg, c0->d_assocm.get(), dbins, lds);
  });
  HIPCHK(c0, hipMemcpyAsync(c0->d_assocm.get(), himg, img_bytes, hipMemcpyHostToDevice, c0->stream));
  HIPCHK(c0, hipMemsetAsync(dbins, 0, bins_bytes, c0->stream));
  if (const int r_ = members.regen()) {
    (void)hipStreamSynchronize(c0->stream);  // the upload reads the pinned image, which the next call rewrites
    return r_;
  }
  RET(members.order());
  visit_state(c0, [&](auto s) {
    assoc_votes_launch<typename decltype(s)::T, typename decltype(s)::SP>(ctxs, e, S, total.launches, himg,
                                                                          c0->d_assocm.get(), lds);
  });
  HIPCHK(c0, hipGetLastError());
  const uint32_t* hbins = (const uint32_t*)(himg + bins_at);
  HIPCHK(c0, hipMemcpyAsync((void*)hbins, dbins, bins_bytes, hipMemcpyDeviceToHost, c0->stream));
  RET(members.finish());
  // the tables are checked before any output is written
  for (int s = 0; s < S; ++s) {
    pfmpe_assoc_out o;
    if (!assoc_epilogue(hbins + e[s].plan.bins_offset, ctxs[s]->M, e[s].B, ctxs[s]->N, &o, nullptr))
      return fail(c0, PFMPE_E_STATE, at(s) + "inconsistent votes table");
  }
  for (int s = 0; s < S; ++s)
    (void)assoc_epilogue(hbins + e[s].plan.bins_offset, ctxs[s]->M, e[s].B, ctxs[s]->N, &out[s], votes ? votes[s] : nullptr);
  return PFMPE_OK;
}
}  // namespace

}  // namespace pfmpe_impl

// ======================================================================================= C-ABI
using namespace pfmpe_impl;

int pfmpe_host_assoc_summary(const uint32_t* votes, int M, int B, pfmpe_assoc_out* out) {
  if (!votes || !out || M < 1 || M > kMaxMarkers || B < 0) return PFMPE_E_ARG;
  std::memset(out, 0, sizeof(*out));
  out->M = M;
  out->B = B;
  for (int m = 0; m < M; ++m) {
    const uint32_t* row = votes + (size_t)m * (B + 1);
    int64_t sum = 0;
    uint32_t best = 0, second = 0, arg = 0;
    for (int b = 0; b <= B; ++b) sum += row[b];
    for (int b = 1; b <= B; ++b) {  // a strict test keeps the lowest blob index among equal vote counts
      if (row[b] > best) {
        second = best;
        best = row[b];
        arg = (uint32_t)b;
      } else if (row[b] > second) {
        second = row[b];
      }
    }
    if (m == 0) out->n = sum;
    if (sum != out->n) return PFMPE_E_ARG;
    out->matched[m] = (uint32_t)(sum - row[0]);
    out->mode_blob[m] = best ? arg : 0u;
    out->mode_votes[m] = best;
    out->second_votes[m] = second;
  }
  return PFMPE_OK;
}

int pfmpe_assoc_stats(pfmpe_ctx* c, int which, const pfmpe_assoc_in* in, pfmpe_assoc_out* out, uint32_t* votes) {
  if (!c) return PFMPE_E_ARG;
  if (!out) return fail(c, PFMPE_E_ARG, "assoc_stats: null out");
  if (!in || (which != PFMPE_ASSOC_PROPAGATED && which != PFMPE_ASSOC_POSTERIOR))
    return fail(c, PFMPE_E_ARG, "assoc_stats: bad arguments");
  AssocEntry e{};
  e.which = which;
  RET(resolve_blobs(c, "assoc_stats", in, &e.blobs, &e.B));
  if (!c->has_model || !c->has_prior) return fail(c, PFMPE_E_STATE, "assoc_stats: set_model and a particle set first");
  if (which == PFMPE_ASSOC_PROPAGATED && !c->has_last) return fail(c, PFMPE_E_STATE, "assoc_stats(propagated): no step yet");
  return assoc_run(&c, 1, &e, out, &votes, "assoc_stats", true);
}

int pfmpe_assoc_stats_multi(pfmpe_ctx* const* ctxs, int S, const pfmpe_assoc_multi_in* in, pfmpe_assoc_out* out,
                            uint32_t* const* votes) {
  static_assert(sizeof(pfmpe_assoc_multi_in) == 24 && sizeof(pfmpe_assoc_plan) == 24 && sizeof(pfmpe_assoc_plan_total) == 80,
                "ABI");
  if (!ctxs || S < 1 || !ctxs[0]) return PFMPE_E_ARG;
  pfmpe_ctx* c0 = ctxs[0];
  if (!in || !out) return fail(c0, PFMPE_E_ARG, "assoc_stats_multi: null in/out");
  if (S > PFMPE_ASSOC_MAX_STREAMS) return fail(c0, PFMPE_E_CAP, "assoc_stats_multi: S exceeds PFMPE_ASSOC_MAX_STREAMS");
  // every check, on host data alone
  AssocEntry e[PFMPE_ASSOC_MAX_STREAMS];
  for (int s = 0; s < S; ++s) {
    pfmpe_ctx* c = ctxs[s];
    const std::string at = "assoc_stats_multi: stream " + std::to_string(s) + ": ";
    if (!c) return fail(c0, PFMPE_E_ARG, at + "null context");
    if (c->device != c0->device || c->state_dtype != c0->state_dtype)
      return fail(c0, PFMPE_E_ARG, at + "device and state type must match ctxs[0]");
    const int which = in[s].which;
    if (which != PFMPE_ASSOC_PROPAGATED && which != PFMPE_ASSOC_POSTERIOR) return fail(c0, PFMPE_E_ARG, at + "bad which");
    e[s] = AssocEntry{};
    e[s].which = which;
    RET(resolve_blobs(c, at.substr(0, at.size() - 2), &in[s].blobs, &e[s].blobs, &e[s].B, c0));
    if (!c->has_model || !c->has_prior) return fail(c0, PFMPE_E_STATE, at + "set_model and a particle set first");
    if (which == PFMPE_ASSOC_PROPAGATED && !c->has_last) return fail(c0, PFMPE_E_STATE, at + "propagated: no step yet");
  }
  return assoc_run(ctxs, S, e, out, votes, "assoc_stats_multi", false);
}

int pfmpe_host_assoc_plan(const int32_t* N, const int32_t* M, const int32_t* B, const int32_t* which, const int32_t* prune,
                          const int32_t* table_bytes, int S, int state_dtype, pfmpe_assoc_plan* plan,
                          pfmpe_assoc_plan_total* total) {
  return assoc_plan(N, M, B, which, prune, table_bytes, S, state_dtype, plan, total, nullptr);
}

void pfmpe_default_gate_params(pfmpe_gate_params* p) {
  if (!p) return;
  p->min_share = 0.5;
  p->lead = 2.0;
  p->min_pairs = 4;
  p->pad = 0;
}

int pfmpe_host_gate_pairs(const uint32_t* votes, int M, int B, const uint32_t* corr, int n_corr,
                          const pfmpe_gate_params* params, uint32_t* gated, pfmpe_gate_out* out) {
  static_assert(sizeof(pfmpe_gate_params) == 24 && sizeof(pfmpe_gate_out) == 32, "ABI");
  if (!votes || !corr || !gated || !out || M < 1 || M > kMaxMarkers || B < 0 || B > kMaxBlobs || n_corr < 0 ||
      n_corr > kMaxMarkers)
    return PFMPE_E_ARG;
  pfmpe_gate_params prm;
  pfmpe_default_gate_params(&prm);
  if (params) prm = *params;
  for (const double v : {prm.min_share, prm.lead})
    if (!(v >= 0.0) || !std::isfinite(v)) return PFMPE_E_ARG;
  if (prm.min_pairs < 0) return PFMPE_E_ARG;
  for (int k = 0; k < n_corr; ++k)
    if (corr[2 * k] < 1u || corr[2 * k] > (uint32_t)M || corr[2 * k + 1] < 1u || corr[2 * k + 1] > (uint32_t)B)
      return PFMPE_E_ARG;
  pfmpe_assoc_out sum;
  if (pfmpe_host_assoc_summary(votes, M, B, &sum) != PFMPE_OK) return PFMPE_E_ARG;  // rows that do not all sum to n
  pfmpe_gate_out go{};
  uint32_t kept[2 * kMaxMarkers] = {0};
  go.n_in = n_corr;
  for (int k = 0; k < n_corr; ++k) {
    const uint32_t led = corr[2 * k], blob = corr[2 * k + 1];
    const uint32_t v = votes[(size_t)(led - 1) * (B + 1) + blob];
    uint8_t r = 0;
    if (!((double)v >= prm.min_share * (double)sum.n)) r |= 1;
    if (sum.mode_blob[led - 1] != blob) r |= 2;
    if (prm.lead * (double)sum.second_votes[led - 1] > (double)sum.mode_votes[led - 1]) r |= 4;
    go.reason[k] = r;
    if (r) continue;
    kept[2 * go.n_gated] = led;
    kept[2 * go.n_gated + 1] = blob;
    go.n_gated += 1;
  }
  go.fallback = go.n_gated < prm.min_pairs ? 1 : 0;
  if (go.fallback) {
    std::memset(kept, 0, sizeof(kept));
    std::memcpy(kept, corr, (size_t)n_corr * 2 * sizeof(uint32_t));
  }
  std::memcpy(gated, kept, sizeof(kept));  // (corr and gated may be the same row)
  *out = go;
  return PFMPE_OK;
}

int pfmpe_get_pairs(pfmpe_ctx* c, int which, const pfmpe_assoc_in* in, int64_t first, int32_t count, uint32_t* corr,
                    int32_t* n_corr) {
  if (!c) return PFMPE_E_ARG;
  if (first < 0 || count < 0 || (count > 0 && (!corr || !n_corr)))
    return fail(c, PFMPE_E_ARG, "get_pairs: bad range or null output");
  if (c->has_prior && first + (int64_t)count > (int64_t)c->N)
    return fail(c, PFMPE_E_ARG, "get_pairs: first + count exceeds the particle count");
  const double* blobs = nullptr;
  int B = 0;
  size_t tbytes = 0;
  GridHdr gh{};
  AssocArgs aa{};
  RET(assoc_prepare(c, "get_pairs", which, in, &blobs, &B, &tbytes, &gh, &aa));
  constexpr size_t kRow = kPairRow;
  const int cap = pairs_cap(c);
  RET(ensure_pairs(c));
  aa.corr = c->d_pairs.get();
  aa.n_corr = (int32_t*)(c->d_pairs.get() + (size_t)cap * kRow);
  for (int64_t done = 0; done < count; done += cap) {
    const int n = (int)std::min<int64_t>(cap, count - done);
    aa.first = (int32_t)(first + done);
    aa.count = n;
    RET(assoc_rows_launch(c, B, c->d_table.get(), tbytes, gh, aa));
    HIPCHK(c, hipMemcpyAsync(corr + (size_t)done * kRow, aa.corr, (size_t)n * kRow * sizeof(uint32_t),
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(n_corr + done, aa.n_corr, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the chunk buffer is reused
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  RET(harvest_timing(c));
  return PFMPE_OK;
}
