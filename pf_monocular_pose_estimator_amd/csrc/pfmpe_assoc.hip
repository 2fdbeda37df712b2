// pfmpe_assoc.hip — the k_assoc_votes instantiations (pfmpe_assoc_stats / pfmpe_get_pairs) and their launch: state
// type x kept set / resident prior x marker bucket x pruning option.  A TU of its own so they build beside the others.
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
template <typename T, typename SP, bool DENSE, int MAXM, bool PRUNE>
__global__ __launch_bounds__(kBlock) void k_assoc_votes(const FrameArgsT<T> fa, const AssocArgs aa,
                                                       const unsigned char* __restrict__ table,
                                                       const SP* __restrict__ st) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ LdsConst<T> sc;
  const int M = fa.M, B = fa.B;
  const int nbins = assoc_bins(M, B);
  const bool lds = aa.votes && aa.lds_votes;
  uint32_t* bins = (uint32_t*)(smem + BlobTable<T>::lds_bytes((size_t)fa.tbytes));
  copy_table(table, smem, (size_t)fa.tbytes);
  stage_consts(fa, sc);
  if (lds)
    for (int i = threadIdx.x; i < nbins; i += kBlock) bins[i] = 0u;
  __syncthreads();  // table, constants and cleared bins visible
  const LdsBlobs<T> tb = view_table<T>(smem, B);
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < aa.count; i += stride) {
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

}  // namespace pfmpe_impl
