#pragma once
// pfmpe_prior.hpp — the resident particle set to and from the transfer buffer d_xfer (N x 12 doubles), for the
// three storage types.  Included only by the translation units that move particle sets (pfmpe_engine.hip,
// pfmpe_init.hip): each of them instantiates k_import / k_export, which are defined here.
#include "pf_state.hpp"
#include "pfmpe_ctx.hpp"

namespace pfmpe {

// ---- state import / export (API helpers, not on the timed path).  anchor: the set's
// anchor pose (fp16 state), ignored for fp32 / fp64 planes.
template <typename T>
struct Pose12 {
  T v[12];
};
template <typename T, typename SP>
__global__ void k_import(const double* __restrict__ poses, SP* __restrict__ st, int N, int64_t ld,
                         const Pose12<T> anchor) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  for (int q = 0; q < 12; ++q)
    st[plane_index<SP>(q, n, ld)] = StateIO<T, SP>::store((T)poses[12 * (int64_t)n + q], anchor.v[q]);
}
template <typename T, typename SP>
__global__ void k_export(const SP* __restrict__ st, double* __restrict__ poses, int N, int64_t ld,
                         const Pose12<T> anchor, const uint32_t* __restrict__ owner) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const int r = owner ? (int)owner[n] : n;  // a deferred prior: stored row owner[n]
  for (int q = 0; q < 12; ++q)
    poses[12 * (int64_t)n + q] = (double)StateIO<T, SP>::load(st[plane_index<SP>(q, r, ld)], anchor.v[q]);
}
// the weights widened into the transfer buffer (pfmpe_get_weights)
template <typename T>
__global__ void k_weights_export(const T* __restrict__ w, double* __restrict__ out, int N) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  out[n] = (double)w[n];
}

}  // namespace pfmpe

namespace pfmpe_impl {

// Install d_xfer's first N poses as the prior, stored in particle order, in two steps.  import_enqueue: the import
// launch (anchor: the fp16 state's anchor pose) and the hand-off state zeroed for the first frame, on stream `on`
// (the context's own, or a batch leader's); errors are reported on `err`.  import_done: the context's bookkeeping,
// once that work has been waited for.
inline int import_enqueue(pfmpe_ctx* c, int N, const double* anchor, hipStream_t on, pfmpe_ctx* err) {
  std::memcpy(c->anchor[c->prior_idx], anchor, 12 * sizeof(double));
  c->prior_owner = -1;
  visit_state(c, [&](auto s) {
    using T = typename decltype(s)::T;
    using SP = typename decltype(s)::SP;
    Pose12<T> a;
    for (int q = 0; q < 12; ++q) a.v[q] = (T)anchor[q];
    hipLaunchKernelGGL((k_import<T, SP>), dim3((N + 255) / 256), dim3(256), 0, on, c->d_xfer.get(),
                       (SP*)c->d_state[c->prior_idx].get(), N, c->ld, a);
  });
  HIPCHK(err, hipGetLastError());
  HIPCHK(err, hipMemsetAsync(c->d_ctrl.get(), 0, sizeof(Ctrl), on));
  HIPCHK(err, hipMemsetAsync(c->d_winkey.get(), 0, kWinBytes, on));
  HIPCHK(err, hipMemsetAsync(c->d_counters.get(), 0, counters_bytes(c), on));
  return PFMPE_OK;
}
inline void import_done(pfmpe_ctx* c, int N) {
  c->N = N;
  c->has_prior = true;
  c->has_last = false;
}
// both steps on the context's own stream, waited for
inline int import_prior(pfmpe_ctx* c, int N, const double* anchor) {
  RET(import_enqueue(c, N, anchor, c->stream, c));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  import_done(c, N);
  return PFMPE_OK;
}

// The prior's first `count` particles -> d_xfer (enqueued on `on`; through the owner indices of a deferred prior).
inline int export_prior(pfmpe_ctx* c, int count, hipStream_t on, pfmpe_ctx* err) {
  visit_state(c, [&](auto s) {
    using T = typename decltype(s)::T;
    using SP = typename decltype(s)::SP;
    Pose12<T> a;
    for (int q = 0; q < 12; ++q) a.v[q] = (T)c->anchor[c->prior_idx][q];
    hipLaunchKernelGGL((k_export<T, SP>), dim3((count + 255) / 256), dim3(256), 0, on,
                       (const SP*)c->d_state[c->prior_idx].get(), c->d_xfer.get(), count, c->ld, a, prior_owner_ptr(c));
  });
  HIPCHK(err, hipGetLastError());
  return PFMPE_OK;
}

}  // namespace pfmpe_impl
