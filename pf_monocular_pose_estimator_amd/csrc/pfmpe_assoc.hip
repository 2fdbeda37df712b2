// pfmpe_assoc.hip — the k_assoc_votes instantiations (pfmpe_assoc_stats / pfmpe_get_pairs) and their launch: state
// type x kept set / resident prior x marker bucket x pruning option.  A TU of its own so they build beside the others.
#include "pfmpe_ctx.hpp"

namespace pfmpe_impl {
using namespace pfmpe;

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
  if (fa.M == kExactM) return assoc_launch_p<T, SP, DENSE, kExactM>(c, fa, aa, table, grid, lds);
  if (fa.M <= 8) return assoc_launch_p<T, SP, DENSE, 8>(c, fa, aa, table, grid, lds);
  if (fa.M <= 12) return assoc_launch_p<T, SP, DENSE, 12>(c, fa, aa, table, grid, lds);
  return assoc_launch_p<T, SP, DENSE, 16>(c, fa, aa, table, grid, lds);
}

template <typename T, typename SP>
int assoc_launch_t(pfmpe_ctx* c, int B, const unsigned char* table, size_t tbytes, const GridHdr& gh, AssocArgs aa) {
  // the likelihood's arguments as a frame with these blobs would get them (model, K, tol, tol_PF, the pruning
  // window, the prior's owner indices); the motion-model part is not read
  pfmpe_frame_in fin{};
  fin.B = B;
  fin.it_since_init = 1;
  fin.dt = 1.0;
  FrameArgsT<T> fa = build_args<T>(c, &fin);
  fa.tbytes = (int32_t)tbytes;
  fa.grid = grid_args<T>(gh, B, (float)fa.tolq);
  for (int q = 0; q < 12; ++q) fa.anc_in[q] = (T)c->anchor[c->prior_idx][q];
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
