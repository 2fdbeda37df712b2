#pragma once
// pfmpe_args.hpp — the kernel arguments of one frame from the host state and the frame inputs (build_args): shared by
// the step's launch sequences (pfmpe_seq.hpp) and the association launch (pfmpe_assoc.hip).
#include "pf_state.hpp"
#include "pfmpe_ctx.hpp"

namespace pfmpe_impl {

// iterations a frame may take: the forced count, else max_iter (at least one)
template <typename T>
inline int iter_cap(const FrameArgsT<T>& fa) {
  return fa.force_iters > 0 ? fa.force_iters : std::max(1, fa.max_iter);
}

inline bool is_identity12(const double* p) {
  static const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  for (int q = 0; q < 12; ++q)
    if (p[q] != I[q]) return false;
  return true;
}

// Kernel arguments from the host state + frame inputs (PE:488-531), pre-converted to T
template <typename T>
FrameArgsT<T> build_args(const pfmpe_ctx* c, const pfmpe_frame_in* in) {
  FrameArgsT<T> fa{};
  for (int q = 0; q < 12; ++q) {
    fa.cur[q] = (T)in->current_pose[q];
    fa.pred[q] = (T)in->predicted_pose[q];
    fa.predm[q] = (T)in->prediction[q];
    fa.cam[q] = (T)in->cam_move_inv[q];
    // fp16 state: anchors of the prior and of the new prior (current pose)
    fa.anc_in[q] = (T)c->anchor[c->prior_idx][q];
    fa.anc_out[q] = (T)in->current_pose[q];
  }
  for (int q = 0; q < kMaxMarkers * 3; ++q) fa.markers[q] = (T)c->markers[q];
  for (int q = 0; q < 9; ++q) fa.K[q] = (T)c->K[q];
  const pfmpe_params& p = c->params;
  double facT, facR;
  if (in->it_since_init == 1) {  // PE:488-496
    facT = 1;
    facR = 1;
  } else {                       // PE:499-505 (all three use predictionMatrix(0,3))
    facT = std::min(std::max(0.2, std::abs(in->prediction[3]) / in->dt), 1.0) / 4;
    facR = 0.2;
  }
  for (int q = 0; q < 3; ++q) {
    fa.dlo[q] = p.ang_min * facR;
    fa.dhi[q] = p.ang_max * facR;
    fa.dlo[3 + q] = p.trans_min * facT;
    fa.dhi[3 + q] = p.trans_max * facT;
  }
  for (int q = 0; q < 6; ++q) {
    fa.lo[q] = (T)fa.dlo[q];
    fa.hi[q] = (T)fa.dhi[q];
    // hi - lo in T (the value the device formed before: bit-identical draws), times 2^-21 (exact)
    fa.rgs[q] = (T)(fa.hi[q] - fa.lo[q]) * (T)0x1p-21;
  }
  fa.growth = p.growth;
  fa.max_iter = p.max_iter;
  fa.force_iters = in->force_iters;
  {  // fp32: every angle draw of the frame within kSmallAngle -> the short sincos polynomials (wave-uniform)
    const int cap = iter_cap(fa);
    // the noise factor 1 + growth * (iter / 10) is linear in the growth step, so its largest magnitude is at the
    // first iteration (1; the largest with a negative growth) or at the last
    const double gmax = std::max(1.0, std::abs(1.0 + p.growth * (double)((cap - 1) / 10)));
    double amax = 0.0;
    for (int q = 0; q < 3; ++q) amax = std::max(amax, std::max(std::abs(fa.dlo[q]), std::abs(fa.dhi[q])));
    fa.small_angles = (sizeof(T) == 4 && amax * gmax <= 0.999 * (double)kSmallAngle) ? 1 : 0;
  }
  fa.k_upper = (fa.K[3] == (T)0 && fa.K[6] == (T)0 && fa.K[7] == (T)0 && fa.K[8] == (T)1) ? 1 : 0;
  fa.tol = (T)p.tol;
  fa.tol_pf = (T)p.tol_pf;
  // every blob with sqrt(d2) <= tol_pf (in T arithmetic) has |dx| <= tolq
  fa.tolq = (T)(p.tol_pf * (1.0 + 1e-3) + 1e-3);
  const int B = in->B;
  fa.exit_thr = (double)((size_t)c->M * (size_t)std::min(p.exit_cap, B));
  fa.accept_thr = (double)((size_t)c->M * (size_t)std::min(p.accept_cap, B));
  fa.key0 = (uint32_t)in->seed;
  fa.key1 = (uint32_t)(in->seed >> 32);
  fa.flo = (uint32_t)in->frame_idx;
  fa.fhi = (uint32_t)(in->frame_idx >> 32);
  fa.lcg_x0 = lcg_seed((uint32_t)in->seed);
  fa.downgrade = c->downgrade;
  fa.N = c->N;
  fa.M = c->M;
  fa.B = B;
  fa.it = in->it_since_init;
  fa.cam_identity = is_identity12(in->cam_move_inv) ? 1 : 0;
  fa.nblk = (c->N + kBlock - 1) / kBlock;
  // groups of 64 whenever the frame can run as one flat launch (k_frame2 reduces one group per wave), so
  // the one-launch and two-launch shapes keep the same summation association; ~sqrt(nblk) beyond
  fa.gsz = (fa.nblk <= kFlatMaxGroups * kGroup && !(c->diag & kDiagSqrtGroups))
               ? kGroup
               : std::min(kGroup, std::max(1, (int)std::ceil(std::sqrt((double)std::max(1, fa.nblk)))));
  fa.ngrp = (fa.nblk + fa.gsz - 1) / fa.gsz;
  // (c->max_grp = max_blk >= ngrp for every N <= max_particles)
  fa.diag = c->diag;
  fa.wait_ticks = (uint32_t)std::min<int64_t>(c->wait_bound_us * 100, 0xffffffffll);  // s_memrealtime: 100 MHz
  fa.ld = c->ld;
  fa.owner = prior_owner_ptr(c);
  fa.owner_out = nullptr;
  return fa;
}

}  // namespace pfmpe_impl
