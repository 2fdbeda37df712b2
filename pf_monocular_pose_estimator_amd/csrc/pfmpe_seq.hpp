#pragma once
// pfmpe_seq.hpp — the launch sequences of pfmpe_step and pfmpe_step_multi (Seq) and their entry points for one
// (state type, RNG): dispatch_m, multi_m, regen_m, regen_list_m.  Included only by the pfmpe_k_<state>_<rng>.hip units,
// which instantiate them (PFMPE_DECLARE_INSTANCE); every other unit sees the declarations in pfmpe_ctx.hpp.
#include "pf_kernels.hpp"
#include "pf_weigh_pk.hpp"
#include "pfmpe_args.hpp"

namespace pfmpe_impl {

// Batch scratch layout (pfmpe_step_multi), the same in the pinned host image and in HBM: host-supplied blob
// tables [0, tbytes), then `na` stream descriptors from doff, then the uint16 block -> stream map of `total`
// blocks from boff; `need` bytes in all.
struct BatchLayout {
  size_t doff, boff, soff, need;
};
template <typename Desc>
inline BatchLayout batch_layout(int na, int64_t total, size_t tbytes) {
  BatchLayout L;
  L.doff = tbytes;
  L.boff = L.doff + ((size_t)na * sizeof(Desc) + 255) / 256 * 256;
  L.soff = L.boff + ((size_t)total * sizeof(uint16_t) + 255) / 256 * 256;  // uint32 status[na] (k_stage_multi)
  L.need = L.soff + (size_t)na * sizeof(uint32_t) + 256;
  return L;
}

// The frames the packed passes cover (pf_weigh_pk.hpp): fp32 compute, the Philox stream, exactly five markers
// (k_weigh_pk) or exactly twelve (k_weigh_pk12; C3), fp32 or fp16 pair-plane state, and per frame: the blob grid on
// (which implies pruning and fp32), the short sincos polynomials, an identity camMoveInv, an upper-triangular K,
// B >= M (the order-free score), blob 0 finite (the NaN-at-origin test by one comparison).  Everything else:
// k_weigh_stream.  kPkMarkers: the marker count of the instance's packed pass, 0 when it has none.
template <typename T, int RNG, int MAXM, typename SP>
constexpr int kPkMarkers = (std::is_same<T, float>::value && RNG == kRngPhilox && (MAXM == kExactM || MAXM == kPk12M) &&
                            (std::is_same<SP, float>::value || std::is_same<SP, __half>::value))
                               ? MAXM
                               : 0;
inline bool pk_eligible(const FrameArgsT<float>& fa, int markers) {
  return fa.grid.on && fa.grid.b0fin && fa.small_angles && fa.cam_identity && fa.k_upper && fa.M == markers &&
         fa.B >= fa.M && !(fa.diag & (kDiagNoPk | kDiagSortedScore));
}
template <typename T, int RNG, int MAXM, typename SP>
constexpr auto pk_kernel() {
  if constexpr (kPkMarkers<T, RNG, MAXM, SP> == kExactM)
    return &k_weigh_pk<SP>;
  else if constexpr (kPkMarkers<T, RNG, MAXM, SP> == kPk12M)
    return &k_weigh_pk12<SP>;
  else
    return nullptr;
}

// Resident blocks of kBlock threads per CU for (kernel, dynamic LDS bytes), asked of the runtime once per context;
// at_least: the floor of the answer kept (1 for a grid size, 0 for the residency test of the one-launch frames).
inline int occupancy(pfmpe_ctx* c, const void* fn, size_t lds, int at_least, int* blocks) {
  const auto key = std::make_pair(fn, lds);
  auto it = c->occ.find(key);
  if (it == c->occ.end()) {
    int per_cu = 0;
    HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kBlock, lds));
    it = c->occ.emplace(key, std::max(at_least, per_cu)).first;
  }
  *blocks = it->second;
  return PFMPE_OK;
}

// the hand-off counters of a context (d_counters): group and top of the weighing pass, group and top of the resampling
struct Counters {
  uint32_t *gcount_w, *tcount_w, *gcount_r, *tcount_r;
};
inline Counters counters(const pfmpe_ctx* c) {
  uint32_t* p = c->d_counters.get();
  return {p, p + c->max_grp, p + c->max_grp + 1, p + 2 * c->max_grp + 1};
}

// the next frame-record sequence number of a context
inline int32_t next_seq(pfmpe_ctx* c) { return c->seq = (c->seq + 1) & 0x3fffffff; }

// Deferred resampling of a two-launch frame: possible at all for this context, and the decision for
// its frame (kept: the frame has its kept propagated set).  The new prior's owner indices go to the owner buffer the
// current prior does not use: that buffer is returned and recorded as frame_owner_out; null: the frame materialises
// its new prior.
inline bool may_defer(const pfmpe_ctx* c) {
  return c->defer && c->d_owner[0].get() && c->d_owner[1].get() && !(c->diag & kDiagNoDefer);
}
inline uint32_t* defer_frame(pfmpe_ctx* c, bool kept) {
  c->frame_owner_out = -1;
  if (!kept || !may_defer(c)) return nullptr;
  c->frame_owner_out = c->prior_owner == 0 ? 1 : 0;
  return c->d_owner[c->frame_owner_out].get();
}

// A frame or batch that left no record (a bounded wait expired, or a HIP error): the control record, the hand-off
// counters, the winner keys, the fused finish's arrival shards and (flat: a one-launch frame) the flat arrival counters
// may hold the failed frame's partial state, which the next frame would take as its own (the control record's
// iteration state; a finisher that stops polling early).  Zero them once `on` has drained; the prior is untouched.
inline int reset_handoffs(pfmpe_ctx* c, hipStream_t on, bool flat = false) {
  HIPCHK(c, hipStreamSynchronize(on));
  HIPCHK(c, hipMemsetAsync(c->d_ctrl.get(), 0, sizeof(Ctrl), c->stream));
  HIPCHK(c, hipMemsetAsync(c->d_counters.get(), 0, counters_bytes(c), c->stream));
  HIPCHK(c, hipMemsetAsync(c->d_winkey.get(), 0, kWinBytes, c->stream));
  if (flat && c->d_flat.get()) HIPCHK(c, hipMemsetAsync(c->d_flat.get(), 0, kFlatWords * sizeof(uint32_t), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PFMPE_OK;
}

// A one-launch frame abandoned by a bounded wait (blocks not co-resident: other work on the device): clear the
// hand-off state, stop fusing on this context; the caller redoes the frame with two launches.
inline int abandoned(pfmpe_ctx* c) {
  RET(reset_handoffs(c, c->stream, true));
  c->flat_base_w = c->flat_base_c = 0;
  c->fused_fallbacks += 1;
  c->fused = 0;
  c->clean_since_fallback = 0;
  // not an error (the frame is redone and returns OK); the text and pfmpe_get_info report it
  c->err = "one-launch frame abandoned at the wait bound (blocks not co-resident: other work on the device?); "
           "redone with two launches, one-launch frames off" +
           std::string(c->fused_rearm > 0 ? " until PFMPE_OPT_FUSED_REARM clean frames" : "");
  return PFMPE_OK;
}
// This flat frame's granule tag base (FrameArgsT::gtag): frame count << 12, never 0.  On wrap the granule area is
// zeroed first, so no stored word carries a tag a later frame uses (the stream must be free: no server running).
constexpr uint32_t kGranFrames = 0xFFFFF;
inline int next_gtag(pfmpe_ctx* c, uint32_t* gtag) {
  if (c->gframe >= kGranFrames) {
    HIPCHK(c, hipMemsetAsync(c->d_gran.get(), 0, kGranBytes, c->stream));
    c->gframe = 0;
  }
  c->gframe += 1;
  *gtag = c->gframe << 12;
  return PFMPE_OK;
}
inline BlockPart* gran_part(const pfmpe_ctx* c, int parity) {
  return (BlockPart*)(c->d_gran.get() + (size_t)parity * kGranPartBytes);
}
inline CountPart* gran_count(const pfmpe_ctx* c) { return (CountPart*)(c->d_gran.get() + kGranCountOff); }

template <typename T, int RNG, int MAXM, typename SP>
struct Seq {
  static constexpr int kPkM = kPkMarkers<T, RNG, MAXM, SP>;
  static int iterate(pfmpe_ctx* c, const FrameArgsT<T>& fa, const unsigned char* table, int iter) {
    const SP* prior = (const SP*)c->d_state[c->prior_idx].get();
    const size_t lds = BlobTable<T>::lds_bytes(fa.tbytes);
    const Counters n = counters(c);
    RET(ensure_prop(c));
    SP* prop0 = c->keep_prop ? (SP*)c->d_prop[0].get() : nullptr;
    SP* prop1 = c->keep_prop ? (SP*)c->d_prop[1].get() : nullptr;
    T* w0 = (T*)c->d_w[0].get();
    T* w1 = (T*)c->d_w[1].get();
    // The streaming weighing pass (k_weigh_stream: resident blocks looping over the 256-particle blocks, the
    // next particle's state prefetched) with the group / top hand-off as two small launches.  It wins for
    // every marker bucket: C5 52 -> 31 us weighing (round 2), C4 265 -> 233 us; at 12 markers (C3) it lost while
    // the pass staged block partials through LDS behind two barriers per block, and wins since it stores wave
    // partials (round 3: C3 116-117 -> 111-113 us per frame, profiles/r03/ab_c3_stream.log).
    // kDiagNoStream / kDiagForceStream pick either pass for tests and A/B.
    const bool stream = !(c->diag & kDiagNoStream);
    // k_weigh_pk / k_weigh_pk12: the streaming pass with two particles per lane in packed fp32 (pf_weigh_pk.hpp), for
    // the frames it covers (pk_eligible); same outputs, same bits
    bool pk = false;
    if constexpr (kPkM != 0) pk = stream && c->prune && pk_eligible(fa, kPkM);
    c->last_weigh_pass = pk ? PFMPE_WEIGH_PK : (stream ? PFMPE_WEIGH_STREAM : PFMPE_WEIGH_BLOCKS);
    if (stream) {
      auto k = c->prune ? k_weigh_stream<T, RNG, MAXM, true, SP> : k_weigh_stream<T, RNG, MAXM, false, SP>;
      int per_cu = 0;
      RET(occupancy(c, pk ? (const void*)pk_kernel<T, RNG, MAXM, SP>() : (const void*)k, lds, 1, &per_cu));
      // k_weigh_pk: a wave per 128-particle task, 2 * nblk tasks
      const int grid = std::min(pk ? (fa.nblk + 1) / 2 : fa.nblk, per_cu * std::max(1, c->num_cu));
      RET(launch_ext(c, PFMPE_K_PROPAGATE, [&] {
        if constexpr (kPkM != 0) {
          if (pk) {
            klaunch(c, pk_kernel<T, RNG, MAXM, SP>(), dim3(grid), dim3(kBlock), lds, fa, table, prior, w0, w1,
                    c->d_part[0].get(), c->d_part[1].get(), (const Ctrl*)c->d_ctrl.get(), prop0, prop1, iter);
            return;
          }
        }
        klaunch(c, k, dim3(grid), dim3(kBlock), lds, fa, table, prior, w0, w1, c->d_part[0].get(), c->d_part[1].get(),
                c->d_ctrl.get(), prop0, prop1, iter);
      }));
      // the top's group partials fit LDS up to 1,365 groups (22M particles); beyond, it reads them from L2
      const size_t glds = fa.ngrp > 64 ? (size_t)fa.ngrp * sizeof(GroupPart) : 0;
      const bool staged = glds > 0 && glds <= 64 * 1024;
      if (fa.ngrp <= 64 && !(c->diag & kDiagSerialTop))  // one tile: group scans + top in one launch
        return launch_ext(c, PFMPE_K_AUX, [&] {
          klaunch(c, k_group_top<T, RNG>, dim3(fa.ngrp), dim3(64), 0, fa, c->d_part[0].get(), c->d_part[1].get(), c->d_bscan[0].get(),
                  c->d_bscan[1].get(), c->d_gpart[0].get(), c->d_gpart[1].get(), c->d_gscan.get(), c->d_ctrl.get(), n.tcount_w, iter);
        });
      return launch_ext(c, PFMPE_K_AUX, [&] {
        klaunch(c, k_group<T>, dim3(fa.ngrp), dim3(64), 0, fa, c->d_part[0].get(), c->d_part[1].get(),
                           c->d_bscan[0].get(), c->d_bscan[1].get(), c->d_gpart[0].get(), c->d_gpart[1].get(), (const Ctrl*)c->d_ctrl.get());
        if (staged && fa.ngrp <= 64 * kTopMaxTiles && !(c->diag & kDiagSerialTop))  // > 1 tile: k_top_wide
          klaunch(c, k_top_wide<T, RNG>, dim3(1), dim3(64 * kTopWaves), glds, fa, c->d_gpart[0].get(), c->d_gpart[1].get(),
                  c->d_gscan.get(), c->d_ctrl.get(), iter);
        else
          klaunch(c, k_top<T, RNG>, dim3(1), dim3(64), staged ? glds : 0, fa, c->d_gpart[0].get(),
                             c->d_gpart[1].get(), c->d_gscan.get(), c->d_ctrl.get(), iter, staged ? 1 : 0);
      });
    }
    auto k = c->prune ? k_propagate_weigh<T, RNG, MAXM, true, SP> : k_propagate_weigh<T, RNG, MAXM, false, SP>;
    return launch_ext(c, PFMPE_K_PROPAGATE, [&] {
      klaunch(c, k, dim3(fa.nblk), dim3(kBlock), lds, fa, table, prior, w0, w1, c->d_part[0].get(), c->d_part[1].get(),
              c->d_bscan[0].get(), c->d_bscan[1].get(), c->d_gpart[0].get(), c->d_gpart[1].get(), c->d_gscan.get(),
              c->d_ctrl.get(), n.gcount_w, n.tcount_w, prop0, prop1, iter, c->d_stamps.get());
    });
  }
  static int finish(pfmpe_ctx* c, const FrameArgsT<T>& fa, const unsigned char* table) {
    const SP* prior = (const SP*)c->d_state[c->prior_idx].get();
    SP* post = (SP*)c->d_state[1 - c->prior_idx].get();
    const Counters n = counters(c);
    const int32_t seq = next_seq(c);
    const bool kept = c->keep_prop && c->d_prop[0].get();  // iterate() allocated them
    FrameArgsT<T> far = fa;
    far.owner_out = defer_frame(c, kept);
    bool owners = false;
    RET(launch_ext(c, PFMPE_K_RESAMPLE, [&] {
      // a deferred frame: one wave per 256-particle block (k_resample_owners), same outputs; its
      // last wave finishes the frame (no k_resample_final)
      if (far.owner_out && !(c->diag & kDiagBlockResample)) {
        owners = true;
        klaunch(c, k_resample_owners<T, RNG, MAXM, SP>, dim3((unsigned)((fa.nblk + kWaves - 1) / kWaves)),
                dim3(kBlock), 0, far, c->d_ctrl.get(), prior, (const T*)c->d_w[0].get(), (const T*)c->d_w[1].get(), c->d_bscan[0].get(),
                c->d_bscan[1].get(), c->d_gscan.get(), c->record_counts ? c->d_counts.get() : nullptr, c->d_mlpose.get(), c->d_winkey.get(),
                win_arrive(c->d_winkey.get()), table, c->h_rec.dev(), seq, c->d_stamps.get());
        return;
      }
      // the kept-set variant compiles the regeneration path out (its registers spilled in the generic form)
      auto k = kept ? k_resample<T, RNG, MAXM, SP, true> : k_resample<T, RNG, MAXM, SP, false>;
      klaunch(c, k, dim3(fa.nblk), dim3(kBlock), 0, far, c->d_ctrl.get(), table,
                         prior, post, (const T*)c->d_w[0].get(), (const T*)c->d_w[1].get(), c->d_bscan[0].get(), c->d_bscan[1].get(),
                         c->d_gscan.get(), c->d_cpart.get(), c->d_cgroup.get(), n.gcount_r, n.tcount_r,
                         c->record_counts ? c->d_counts.get() : nullptr, c->d_cand.get(), c->d_mlpose.get(), c->h_rec.dev(), seq,
                         c->d_stamps.get(), kept ? (const SP*)c->d_prop[0].get() : nullptr,
                         kept ? (const SP*)c->d_prop[1].get() : nullptr, c->d_winkey.get());
    }));
    c->last_resample = owners ? PFMPE_RESAMPLE_OWNERS : PFMPE_RESAMPLE_BLOCKS;
    if (!owners)
      RET(launch_ext(c, PFMPE_K_FINAL, [&] {
        klaunch(c, k_resample_final<T, RNG, MAXM, SP>, dim3(1), dim3(kFinalBlock), BlobTable<T>::bytes(fa.B), fa,
                c->d_ctrl.get(), table, prior, c->d_cpart.get(), c->d_cand.get(), c->d_mlpose.get(), c->h_rec.dev(), seq, c->d_stamps.get(), kept ? 1 : 0,
                c->d_winkey.get());
      }));
    RET(tail_after(c));
    if (const int rc = wait_frame(c); rc != PFMPE_OK) {
      const std::string err = c->err;
      (void)reset_handoffs(c, c->stream);
      return fail(c, rc, err);
    }
    return PFMPE_OK;
  }
  // the whole frame as one launch, if every block can be resident at once: k_frame2 (flat hand-offs,
  // c->fused == 2, <= 512 blocks) or k_frame (tree hand-offs)
  template <bool PRUNE>
  static int frame_fused(pfmpe_ctx* c, const FrameArgsT<T>& fa_in, const unsigned char* table, bool* launched) {
    *launched = false;
    const bool flat = c->fused == 2 && fa_in.nblk <= kFlatMaxGroups * kGroup && fa_in.gsz == kGroup && c->d_flat.get();
    const void* fn = flat ? (const void*)k_frame2<T, RNG, MAXM, PRUNE, SP> : (const void*)k_frame<T, RNG, MAXM, PRUNE, SP>;
    const size_t lds = BlobTable<T>::lds_bytes(fa_in.tbytes);
    int occ = 0;
    RET(occupancy(c, fn, lds, 0, &occ));
    // Residency by grid size alone (cdna_hip_programming.md §1): at most 2 blocks per CU and one below the
    // occupancy answer (which over-reports by one for SGPR-heavy kernels).  A plain launch: the
    // cooperative launch would only add this check at +15-19 us per frame (MI355X_MICROARCH.md
    // "coop-launch"); every in-kernel wait is bounded anyway.
    const int per_cu = std::min(2, occ - 1);
    if (per_cu < 1 || (int64_t)per_cu * c->num_cu < fa_in.nblk) return PFMPE_OK;  // two-launch path
    std::atomic<int>& busy = fused_inflight(c->device);
    int expect = 0;
    if (!busy.compare_exchange_strong(expect, 1)) {  // another context's one-launch frame is on the device
      c->guard_skips += 1;
      return PFMPE_OK;
    }
    struct Release {
      std::atomic<int>& b;
      ~Release() { b.store(0); }
    } release{busy};
    FrameArgsT<T> a = fa_in;
    a.flat_base_w = c->flat_base_w;
    a.flat_base_c = c->flat_base_c;
    // granule tags: k_frame2's hand-offs, and k_frame's count barrier unless it runs as a tree (kDiagTreeCount)
    // (the flat count barrier's poll covers <= kFlatMaxGroups * kGroup blocks: at most 2 per CU on 256 CUs)
    const bool tree_count = !flat && ((c->diag & kDiagTreeCount) || a.nblk > kFlatMaxGroups * kGroup);
    if (!tree_count) RET(next_gtag(c, &a.gtag));
    const SP* prior = (const SP*)c->d_state[c->prior_idx].get();
    SP* post = (SP*)c->d_state[1 - c->prior_idx].get();
    T* w0 = (T*)c->d_w[0].get();
    T* w1 = (T*)c->d_w[1].get();
    const Counters n = counters(c);
    uint32_t* counts = c->record_counts ? c->d_counts.get() : nullptr;
    const int32_t seq = next_seq(c);
    RET(launch_ext(c, PFMPE_K_FRAME, [&] {
      if (flat)
        klaunch(c, k_frame2<T, RNG, MAXM, PRUNE, SP>, dim3(a.nblk), dim3(kBlock), lds, a, table,
                           prior, post, w0, w1, gran_part(c, 0), gran_part(c, 1), c->d_ctrl.get(), gran_count(c), c->d_flat.get(),
                           counts, c->d_cand.get(), c->d_mlpose.get(), c->h_rec.dev(), seq, c->d_stamps.get());
      else
        klaunch(c, k_frame<T, RNG, MAXM, PRUNE, SP>, dim3(a.nblk), dim3(kBlock), lds, a, table,
                           prior, post, w0, w1, c->d_part[0].get(), c->d_part[1].get(), c->d_bscan[0].get(), c->d_bscan[1].get(),
                           c->d_gpart[0].get(), c->d_gpart[1].get(), c->d_gscan.get(), c->d_ctrl.get(),
                           tree_count ? c->d_cpart.get() : gran_count(c), c->d_cgroup.get(), n.gcount_w,
                           n.tcount_w, n.gcount_r, n.tcount_r, c->d_gen.get(), counts, c->d_cand.get(), c->d_mlpose.get(), c->h_rec.dev(), seq,
                           c->d_stamps.get(), tree_count ? nullptr : c->d_flat.get());
    }));
    RET(tail_after(c));
    *launched = true;
    if (wait_frame(c) != PFMPE_OK) {
      RET(abandoned(c));
      *launched = false;
      return PFMPE_OK;
    }
    if (flat || !(c->diag & kDiagTreeCount)) {  // the flat counters' new running totals (k_frame: the count set only)
      const OutDev& o = *c->h_out;
      if (flat) c->flat_base_w += (uint32_t)o.iters * (uint32_t)a.nblk;
      if (o.resampled) c->flat_base_c += (uint32_t)a.nblk;
    }
    return PFMPE_OK;
  }

  static int step(pfmpe_ctx* c, const FrameArgsT<T>& fa, const unsigned char* table) {
    if (!c->fused && c->fused_user && c->fused_rearm > 0 && c->clean_since_fallback >= c->fused_rearm)
      c->fused = c->fused_user;  // re-armed after enough clean two-launch frames
    const int64_t fallbacks0 = c->fused_fallbacks;
    if (c->fused) {
      bool launched = false;
      RET(c->prune ? frame_fused<true>(c, fa, table, &launched) : frame_fused<false>(c, fa, table, &launched));
      if (launched) {
        if (!frame_done(c)) return fail(c, PFMPE_E_STATE, "fused frame did not finish");
        c->last_shape = (c->fused == 2 && fa.nblk <= kFlatMaxGroups * kGroup && fa.gsz == kGroup) ? PFMPE_SHAPE_FRAME2
                                                                                                   : PFMPE_SHAPE_FRAME;
        last_args<T>(c) = fa;
        return PFMPE_OK;
      }
    }
    c->last_shape = PFMPE_SHAPE_TWO_LAUNCH;
    const int cap = iter_cap(fa);
    int iter = 0;
    RET(iterate(c, fa, table, iter++));
    RET(finish(c, fa, table));
    // Rare path: the exit rule did not fire on iteration 0.  Later iterations are queued in growing
    // batches; launches past the exit are no-ops (they read ctrl->done).
    int batch = 1;
    while (!frame_done(c)) {
      if (iter >= cap) return fail(c, PFMPE_E_STATE, "PF iteration loop did not terminate");
      for (int b = 0; b < batch && iter < cap; ++b) RET(iterate(c, fa, table, iter++));
      RET(finish(c, fa, table));
      batch = std::min(batch * 2, 16);
    }
    if (!c->fused && c->fused_fallbacks == fallbacks0) c->clean_since_fallback += 1;  // not the redone frame
    last_args<T>(c) = fa;
    return PFMPE_OK;
  }
  // A stream of a batch left no frame record.  If some descriptor failed the staging check (status != gen),
  // report it as PFMPE_E_STATE with the words the device read that differ from the ones the host wrote (the
  // HBM copy k_stage_multi made); otherwise it is the wait's own error.  No kernel followed a pointer of a
  // failed descriptor, and a failed batch changes no context's prior (take_step is not reached).
  static int batch_failure(pfmpe_ctx* c0, pfmpe_ctx* const* cs, const std::vector<int>& act,
                           const std::vector<StreamDesc<T, SP>>& want, const unsigned char* ddesc, const uint32_t* dstat,
                           uint32_t gen, const std::string& wait_err) {
    using Desc = StreamDesc<T, SP>;
    const int na = (int)act.size();
    std::vector<uint32_t> st(na, 0);
    std::vector<Desc> seen(na);
    if (hipStreamSynchronize(c0->stream) != hipSuccess ||
        hipMemcpy(st.data(), dstat, (size_t)na * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy((void*)seen.data(), ddesc, (size_t)na * sizeof(Desc), hipMemcpyDeviceToHost) != hipSuccess)
      return fail(c0, PFMPE_E_HIP, "step_multi: " + wait_err);
    static const std::pair<size_t, const char*> kFields[] = {
        {offsetof(Desc, table), "table"},   {offsetof(Desc, prior), "prior"},   {offsetof(Desc, post), "post"},
        {offsetof(Desc, w0), "w0"},         {offsetof(Desc, w1), "w1"},         {offsetof(Desc, part0), "part0"},
        {offsetof(Desc, part1), "part1"},   {offsetof(Desc, bscan0), "bscan0"}, {offsetof(Desc, bscan1), "bscan1"},
        {offsetof(Desc, gpart0), "gpart0"}, {offsetof(Desc, gpart1), "gpart1"}, {offsetof(Desc, gscan), "gscan"},
        {offsetof(Desc, ctrl), "ctrl"},     {offsetof(Desc, gcount_w), "gcount_w"}, {offsetof(Desc, tcount_w), "tcount_w"},
        {offsetof(Desc, gcount_r), "gcount_r"}, {offsetof(Desc, tcount_r), "tcount_r"}, {offsetof(Desc, prop0), "prop0"},
        {offsetof(Desc, prop1), "prop1"},   {offsetof(Desc, cpart), "cpart"},   {offsetof(Desc, cgroup), "cgroup"},
        {offsetof(Desc, counts), "counts"}, {offsetof(Desc, cand), "cand"},     {offsetof(Desc, mlpose), "mlpose"},
        {offsetof(Desc, out), "out"},       {offsetof(Desc, winkey), "winkey"},
        {offsetof(Desc, seq), "seq|first_blk"}, {offsetof(Desc, gen), "gen"},
        {offsetof(Desc, tag), "tag"},       {offsetof(FrameArgsT<T>, key0), "fa.key0|key1"},
        {offsetof(FrameArgsT<T>, flo), "fa.flo|fhi"}};
    auto name = [&](size_t off) -> std::string {
      for (const auto& f : kFields)
        if (f.first == off) return f.second;
      return off < sizeof(FrameArgsT<T>) ? "fa+" + std::to_string(off) : "+" + std::to_string(off);
    };
    for (int i = 0; i < na; ++i) {
      if (st[i] == gen) continue;
      std::string msg = "step_multi: stream " + std::to_string(act[i]) + ": descriptor failed the staging check (gen " +
                        std::to_string(gen) + ", status " + std::to_string(st[i]) + "); words read != written:";
      const uint64_t* a = (const uint64_t*)&want[i];
      const uint64_t* b = (const uint64_t*)&seen[i];
      int shown = 0;
      for (size_t k = 0; k < sizeof(Desc) / 8 && shown < 8; ++k)
        if (a[k] != b[k]) {
          char buf[96];
          std::snprintf(buf, sizeof buf, " %s host 0x%llx device 0x%llx;", name(8 * k).c_str(), (unsigned long long)a[k],
                        (unsigned long long)b[k]);
          msg += buf;
          ++shown;
        }
      if (!shown) msg += " none (the tag or generation check failed on words equal to the host's)";
      cs[act[i]]->err = msg;
      return fail(c0, PFMPE_E_STATE, msg);
    }
    return fail(c0, PFMPE_E_HIP, "step_multi: " + wait_err);
  }
  // S contexts' frames as ONE batch on cs[0]'s HIP stream (pfmpe_step_multi): one weighing launch over every
  // stream's blocks, one resampling launch, one finishing launch with a block per stream.  Streams whose exit
  // rule did not fire on the first iteration get further iteration batches (the others are not relaunched),
  // exactly as step()'s two-launch path does for one stream.  h / d: the batch scratch, whose first
  // `tbytes` bytes already hold the host-supplied blob tables; tables[s] are device addresses.  The caller
  // (multi_m) audited the layout of the whole batch (audit_batch); every later round is a subset of it.
  static int step_multi(pfmpe_ctx* const* cs, int S, const FrameArgsT<T>* fas, const unsigned char* const* tables,
                        unsigned char* h, const unsigned char* hdev, unsigned char* d, size_t tbytes) {
    using Desc = StreamDesc<T, SP>;
    pfmpe_ctx* c0 = cs[0];
    std::vector<int> act(S);
    for (int s = 0; s < S; ++s) act[s] = s;
    int iter = 0, nb = 1;
    for (int round = 0;; ++round) {
      const int na = (int)act.size();
      const BatchLayout L = batch_layout<Desc>(na, 0, tbytes);
      Desc* hd = (Desc*)(h + L.doff);
      int64_t total = 0;
      size_t lds_w = 0, lds_f = 0;
      bool all_kept = true;  // every stream has its kept propagated set: k_resample_multi<KEPT = true>
      bool all_owners = true;  // ... and defers its new prior: k_resample_owners_multi
      if (++c0->multi_gen == 0u || c0->multi_gen == ~0u) c0->multi_gen = 1u;  // never 0 / ~0 (status words)
      const uint32_t gen = c0->multi_gen;
      std::vector<Desc> want(na);  // the descriptors as written (the staging check's reference for a report)
      auto write_desc = [&](int i) {  // tagged, into the pinned image
        Desc& x = want[i];
        x.tag = desc_tag((const uint64_t*)&x, (int)(offsetof(Desc, tag) / 8));
        std::memcpy((void*)&hd[i], (const void*)&x, sizeof(Desc));
        if (i == 0 && (c0->diag & kDiagCorruptDesc)) hd[0].fa.key0 ^= 1u;  // test: altered after the tag
      };
      for (int i = 0; i < na; ++i) {
        pfmpe_ctx* c = cs[act[i]];
        const FrameArgsT<T>& fa = fas[act[i]];
        Desc& x = want[i];
        std::memset((void*)&x, 0, sizeof(Desc));
        x.fa = fa;
        x.table = tables[act[i]];
        x.prior = (const SP*)c->d_state[c->prior_idx].get();
        x.post = (SP*)c->d_state[1 - c->prior_idx].get();
        x.w0 = (T*)c->d_w[0].get();
        x.w1 = (T*)c->d_w[1].get();
        x.part0 = c->d_part[0].get();
        x.part1 = c->d_part[1].get();
        x.bscan0 = c->d_bscan[0].get();
        x.bscan1 = c->d_bscan[1].get();
        x.gpart0 = c->d_gpart[0].get();
        x.gpart1 = c->d_gpart[1].get();
        x.gscan = c->d_gscan.get();
        x.ctrl = c->d_ctrl.get();
        const Counters n = counters(c);
        x.gcount_w = n.gcount_w;
        x.tcount_w = n.tcount_w;
        x.gcount_r = n.gcount_r;
        x.tcount_r = n.tcount_r;
        // The stored set with deferred resampling (k_resample_multi writes owner indices; the kept buffer becomes the
        // stream's prior at take_step, as in finish()) for every state type; without deferral it pays in batches only
        // for fp16 state (round-3 A/B, DESIGN.md §4.2: 8 x C5 batches 5-8 % faster regenerating).  No choice here
        // changes a result.
        const bool kept = c->keep_prop && c->d_prop[0].get() && (may_defer(c) || std::is_same<SP, __half>::value);
        x.prop0 = kept ? (SP*)c->d_prop[0].get() : nullptr;
        x.prop1 = kept ? (SP*)c->d_prop[1].get() : nullptr;
        all_kept = all_kept && kept;
        x.fa.owner_out = defer_frame(c, kept);
        all_owners = all_owners && x.fa.owner_out;
        x.cpart = c->d_cpart.get();
        x.cgroup = c->d_cgroup.get();
        x.counts = c->record_counts ? c->d_counts.get() : nullptr;
        x.cand = c->d_cand.get();
        x.mlpose = c->d_mlpose.get();
        x.out = c->h_rec.dev();
        x.winkey = c->d_winkey.get();
        x.seq = next_seq(c);
        x.first_blk = (int32_t)total;
        x.gen = gen;
        write_desc(i);
        total += fa.nblk;
        lds_w = std::max(lds_w, BlobTable<T>::lds_bytes(fa.tbytes));
        lds_f = std::max(lds_f, BlobTable<T>::bytes(fa.B));
      }
      // The streaming packed pass for the whole batch (k_weigh_pk_multi + the batched group / top hand-off) when
      // every stream's frame is one k_weigh_pk covers; otherwise the one-block pass with its in-launch hand-off
      // (k_propagate_weigh_multi).  Each stream gets a share of the resident workgroups in proportion to its
      // particles (at least one, at most one per four tasks), written into its descriptor before the tag.
      bool pk = false;
      int pk_grid_x = 0, max_ngrp = 0;
      if constexpr (kPkM == kExactM) {
        pk = c0->prune && !(c0->diag & (kDiagNoStream | kDiagNoPk));
        for (int i = 0; i < na && pk; ++i) pk = pk_eligible(fas[act[i]], kExactM);
        if (pk) {
          int per_cu = 0;
          RET(occupancy(c0, (const void*)k_weigh_pk_multi<SP>, lds_w, 1, &per_cu));
          const int64_t cap = (int64_t)per_cu * std::max(1, c0->num_cu);
          for (int i = 0; i < na; ++i) {
            const FrameArgsT<T>& fa = fas[act[i]];
            const int64_t tasks = 2 * (int64_t)fa.nblk;
            const int64_t share = std::max<int64_t>(1, cap * fa.nblk / std::max<int64_t>(1, total));
            const int wg = (int)std::max<int64_t>(1, std::min<int64_t>(share, (tasks + kWaves - 1) / kWaves));
            want[i].wg = wg;
            write_desc(i);
            pk_grid_x = std::max(pk_grid_x, wg);
            max_ngrp = std::max(max_ngrp, fa.ngrp);
          }
        }
      }
      const BatchLayout Lt = batch_layout<Desc>(na, total, tbytes);
      uint32_t* dstat = (uint32_t*)(d + Lt.soff);
      // iterations of this round: no launch past the largest remaining cap of the active streams (a launch past
      // a stream's own cap would be a no-op on its ctrl->done, but it also runs with an iteration number the
      // host's small-angle bound did not cover)
      int room = 0;
      for (int i = 0; i < na; ++i) room = std::max(room, iter_cap(fas[act[i]]) - iter);
      const int nit = std::max(1, std::min(nb, room));
      // descriptors, host tables (first round) and the block map go to HBM by a staging launch in the same
      // stream (k_stage_multi reads the pinned image once), not by a copy-engine transfer
      const Desc* dd = (const Desc*)(d + Lt.doff);
      const uint16_t* db = (const uint16_t*)(d + Lt.boff);
      // the block map is rewritten only when this batch's layout differs from the one staged last (a steady
      // multi-stream loop stages it once: 2 x C4's 78k entries were most of k_stage_multi's 8 us)
      std::vector<int64_t> sig;
      sig.reserve(2 + 2 * (size_t)na);
      sig.push_back((int64_t)Lt.boff);
      sig.push_back(total);
      for (int i = 0; i < na; ++i) {
        sig.push_back(want[i].first_blk);
        sig.push_back(want[i].fa.nblk);
      }
      const bool map_kept = sig == c0->map_sig;
      c0->map_sig.swap(sig);
      const int64_t t_l0 = now_ns();
      if (round == 0) c0->mt_ns[0] += t_l0 - c0->mt_enter;
      RET(launch_ext(c0, PFMPE_K_AUX, [&] {
        klaunch(c0, k_stage_multi<T, SP>, dim3((unsigned)na), dim3(kBlock), 0, hdev, d, (uint32_t)Lt.doff,
                (uint32_t)(round == 0 ? tbytes : 0), map_kept ? kMapKept : (uint32_t)Lt.boff, dstat, gen);
      }));
      for (int k = 0; k < nit; ++k, ++iter) {
        if constexpr (kPkM == kExactM) {
          if (pk) {
            const uint32_t* cst = dstat;
            RET(launch_ext(c0, PFMPE_K_PROPAGATE, [&] {
              klaunch(c0, k_weigh_pk_multi<SP>, dim3((unsigned)pk_grid_x, (unsigned)na), dim3(kBlock), lds_w, dd, na,
                      cst, gen, iter);
            }));
            // the group / top hand-off: one launch when every stream's groups fit one tile, else group scans +
            // the wide top (group partials staged in LDS) or, beyond its LDS, the one-wave top
            const size_t glds = (size_t)max_ngrp * sizeof(GroupPart);
            const bool wide = glds <= 64 * 1024 && max_ngrp <= 64 * kTopMaxTiles && !(c0->diag & kDiagSerialTop);
            RET(launch_ext(c0, PFMPE_K_AUX, [&] {
              if (max_ngrp <= 64 && !(c0->diag & kDiagSerialTop)) {
                klaunch(c0, k_group_top_multi<T, RNG, SP>, dim3((unsigned)max_ngrp, (unsigned)na), dim3(64), 0, dd, na,
                        cst, gen, iter);
              } else {
                klaunch(c0, k_group_multi<T, SP>, dim3((unsigned)max_ngrp, (unsigned)na), dim3(64), 0, dd, na, cst, gen);
                if (wide)
                  klaunch(c0, k_top_wide_multi<T, RNG, SP>, dim3((unsigned)na), dim3(64 * kTopWaves), glds, dd, na, cst,
                          gen, iter);
                else
                  klaunch(c0, k_top_multi<T, RNG, SP>, dim3((unsigned)na), dim3(64), 0, dd, na, cst, gen, iter);
              }
            }));
            continue;
          }
        }
        auto kw = c0->prune ? k_propagate_weigh_multi<T, RNG, MAXM, true, SP>
                            : k_propagate_weigh_multi<T, RNG, MAXM, false, SP>;
        RET(launch_ext(c0, PFMPE_K_PROPAGATE, [&] {
          klaunch(c0, kw, dim3((unsigned)total), dim3(kBlock), lds_w, dd, db, na, (const uint32_t*)dstat, gen, iter);
        }));
      }
      const bool owners = all_owners && !(c0->diag & kDiagBlockResample);
      for (int i = 0; i < na; ++i) {
        cs[act[i]]->last_weigh_pass = pk ? PFMPE_WEIGH_PK : PFMPE_WEIGH_BLOCKS;
        cs[act[i]]->last_resample = owners ? PFMPE_RESAMPLE_OWNERS : PFMPE_RESAMPLE_BLOCKS;
      }
      RET(launch_ext(c0, PFMPE_K_RESAMPLE, [&] {
        if (owners)  // a wave per block (§4.2d), each stream finished by its last block's wave
          klaunch(c0, k_resample_owners_multi<T, RNG, MAXM, SP>, dim3((unsigned)((total + kWaves - 1) / kWaves)),
                  dim3(kBlock), 0, dd, db, na, (const uint32_t*)dstat, gen, (int)total);
        else
          klaunch(c0, all_kept ? k_resample_multi<T, RNG, MAXM, SP, true> : k_resample_multi<T, RNG, MAXM, SP, false>,
                  dim3((unsigned)total), dim3(kBlock), 0, dd, db, na, (const uint32_t*)dstat, gen);
      }));
      if (!owners)
        RET(launch_ext(c0, PFMPE_K_FINAL, [&] {
          klaunch(c0, k_resample_final_multi<T, RNG, MAXM, SP>, dim3((unsigned)na), dim3(kFinalBlock), lds_f, dd,
                  (const uint32_t*)dstat, gen);
        }));
      if (c0->tail_S) RET(tail_launch(c0, round + 1));  // a stream active in this round was active in every earlier one
      const int64_t t_l1 = now_ns();
      c0->mt_ns[1] += t_l1 - t_l0;
      std::vector<int> next;
      for (int i = 0; i < na; ++i) {
        pfmpe_ctx* c = cs[act[i]];
        if (wait_frame(c, c0->stream) != PFMPE_OK) {
          const std::string err = c->err;
          for (int k = 0; k < na; ++k) (void)reset_handoffs(cs[act[k]], c0->stream);
          return batch_failure(c0, cs, act, want, d + Lt.doff, dstat, gen, err);
        }
        if (!frame_done(c)) next.push_back(act[i]);
      }
      c0->mt_ns[2] += now_ns() - t_l1;
      if (next.empty()) break;
      for (int s : next)
        if (iter >= iter_cap(fas[s])) return fail(c0, PFMPE_E_STATE, "step_multi: PF iteration loop did not terminate");
      act.swap(next);
      nb = round == 0 ? 1 : std::min(nb * 2, 16);
    }
    for (int s = 0; s < S; ++s) {
      cs[s]->last_shape = PFMPE_SHAPE_TWO_LAUNCH;
      last_args<T>(cs[s]) = fas[s];
    }
    return PFMPE_OK;
  }
  static int regen(pfmpe_ctx* c, int kept_iter, const void* prior, double* out) {
    const FrameArgsT<T>& fa = last_args<T>(c);
    return launch_ext(c, PFMPE_K_AUX, [&] {
      klaunch(c, k_regen<T, RNG, SP>, dim3((fa.N + 255) / 256), dim3(256), 0, fa, kept_iter,
                         (const SP*)prior, out);
    });
  }
  static int regen_list(pfmpe_ctx* c, int kept_iter, const void* prior, const int32_t* list, const uint32_t* count,
                        int limit, double* out) {
    const FrameArgsT<T>& fa = last_args<T>(c);
    if (limit < 1) return PFMPE_OK;
    return launch_ext(c, PFMPE_K_AUX, [&] {
      klaunch(c, k_regen_list<T, RNG, SP>, dim3((limit + kBlock - 1) / kBlock), dim3(kBlock), 0, fa, kept_iter,
              (const SP*)prior, list, count, limit, out);
    });
  }
};

template <typename T, int RNG, typename SP>
int dispatch_m(pfmpe_ctx* c, const pfmpe_frame_in* in, const unsigned char* table, size_t tbytes, const GridHdr& gh) {
  c->frame_owner_out = -1;  // one-launch frames materialise the new prior (finish() may set it)
  FrameArgsT<T> fa = build_args<T>(c, in);
  fa.tbytes = (int32_t)tbytes;
  fa.grid = grid_args<T>(gh, fa.B, (float)fa.tolq);
  c->last_grid = fa.grid.on;
  // marker capacity buckets: the per-particle loops are unrolled to MAXM (5: the 5-LED configs C1/C2/C4, exact; 12: C3)
  return visit_m(fa.M, fa.M == kExactM, [&](auto m) { return Seq<T, RNG, decltype(m)::value, SP>::step(c, fa, table); });
}

// Host-side bounds audit of a batch (the batched fault at 8 x 10M fp16 streams).  Everything a
// batched kernel indexes is derived here from the descriptors it will read, and checked against what each
// context allocated at create (pfmpe_create: max_blk blocks, max_grp = max_blk groups, ld-element planes,
// a blob bank of bank_off.back() bytes) and against the batch scratch: a stream's blocks, groups, planes,
// table, count partials and candidates all stay inside its own buffers, the block map covers [0, total)
// exactly once, and the scratch holds tables + descriptors + map.  A failing check returns PFMPE_E_STATE
// (a bug, never an input error: check_step validated the inputs) instead of launching.
template <typename T, typename SP>
int audit_batch(pfmpe_ctx* const* cs, int S, const FrameArgsT<T>* fas, const pfmpe_frame_in* in,
                const std::vector<size_t>& toff, size_t tbytes, int64_t total, size_t cap) {
  pfmpe_ctx* c0 = cs[0];
  auto bad = [&](int s, const char* what) {
    return fail(c0, PFMPE_E_STATE, "step_multi: batch audit failed for stream " + std::to_string(s) + ": " + what);
  };
  int64_t first = 0;
  for (int s = 0; s < S; ++s) {
    const pfmpe_ctx* c = cs[s];
    const FrameArgsT<T>& fa = fas[s];
    if (fa.N != c->N || fa.N < 1 || fa.N > c->max_particles || (int64_t)fa.N > c->ld) return bad(s, "particle count");
    if (fa.nblk != (fa.N + kBlock - 1) / kBlock || fa.nblk > c->max_blk) return bad(s, "block count");
    if (fa.gsz < 1 || fa.gsz > kGroup || fa.ngrp != (fa.nblk + fa.gsz - 1) / fa.gsz || fa.ngrp > c->max_grp)
      return bad(s, "group count");
    if (fa.ld != c->ld) return bad(s, "plane stride");
    if (c->state_dtype != PFMPE_STATE_F64 && (int64_t)kPlanes * c->ld * (int64_t)c->es >= ((int64_t)1 << 32))
      return bad(s, "plane buffer resource range");
    if (fa.M != c->M || fa.M < 1 || fa.M > c->max_markers || fa.B < 0 || fa.B > c->max_blobs) return bad(s, "M / B");
    if (c->keep_prop && (!c->d_prop[0].get() || !c->d_prop[1].get())) return bad(s, "kept propagated set not allocated");
    if (c->record_counts && !c->d_counts.get()) return bad(s, "count buffer not allocated");
    if (in[s].bank_frame >= 0) {
      const size_t f = (size_t)in[s].bank_frame;
      if (!c->d_bank.get() || f >= c->bank_B.size() || c->bank_B[f] != fa.B ||
          c->bank_off[f] + (size_t)fa.tbytes != c->bank_off[f + 1] || fa.tbytes < (int)BlobTable<T>::bytes(fa.B))
        return bad(s, "bank table");
    } else if (toff[s] + (size_t)fa.tbytes > tbytes || fa.tbytes < (int)BlobTable<T>::bytes(fa.B)) {
      return bad(s, "host table");
    }
    first += fa.nblk;
  }
  if (first != total || total < 1 || total > kMultiMaxBlocks) return bad(0, "block total");
  if (batch_layout<StreamDesc<T, SP>>(S, total, tbytes).need > cap) return bad(0, "batch scratch");
  return PFMPE_OK;
}

// pfmpe_step_multi for S validated contexts of one (state type, RNG): frame arguments and blob tables
// (host-supplied tables staged into the batch scratch of cs[0]), the bounds audit, the order after each
// member's latest work on other streams, then Seq::step_multi on the marker bucket of the largest M, then the
// fence every member's next work on its own stream is ordered after.
template <typename T, int RNG, typename SP>
int multi_m(pfmpe_ctx* const* cs, int S, const pfmpe_frame_in* in) {
  using Desc = StreamDesc<T, SP>;
  pfmpe_ctx* c0 = cs[0];
  std::vector<FrameArgsT<T>> fas(S);
  std::vector<size_t> toff(S, 0);
  std::vector<std::vector<unsigned char>> hosttab(S);
  size_t tbytes = 0;
  int64_t total = 0;
  int maxM = 1;
  bool all5 = true;  // every stream has exactly kExactM markers: the exact 5-slot bucket serves the batch
  for (int s = 0; s < S; ++s) {
    pfmpe_ctx* c = cs[s];
    c->frame_owner_out = -1;  // step_multi sets it for the streams it defers
    all5 = all5 && c->M == kExactM;
    fas[s] = build_args<T>(c, &in[s]);
    if (in[s].bank_frame < 0) {  // host blobs: the table is built now (its size depends on the blobs)
      hosttab[s].resize(BlobTable<T>::max_bytes());
      fas[s].tbytes = (int32_t)build_blob_table_host<T>(in[s].blobs, in[s].B, (double)fas[s].tolq, hosttab[s].data());
      fas[s].grid = grid_args<T>(*(const GridHdr*)(hosttab[s].data() + BlobTable<T>::off_grid(in[s].B)), in[s].B,
                                 (float)fas[s].tolq);
      toff[s] = tbytes;
      tbytes += ((size_t)fas[s].tbytes + 255) / 256 * 256;
    } else {
      const size_t f = (size_t)in[s].bank_frame;
      fas[s].tbytes = (int32_t)(c->bank_off[f + 1] - c->bank_off[f]);
      fas[s].grid = grid_args<T>(c->bank_grid[f], in[s].B, (float)fas[s].tolq);
    }
    c->last_grid = fas[s].grid.on;
    total += fas[s].nblk;
    maxM = std::max(maxM, c->M);
  }
  const int64_t max_blocks = std::min(kMultiMaxBlocks, c0->multi_max_blocks);
  if (total > max_blocks)
    return fail(c0, PFMPE_E_CAP, "step_multi: " + std::to_string(total) + " blocks in one batch (at most " +
                                     std::to_string(max_blocks) + " = " + std::to_string(max_blocks * kBlock) +
                                     " particles, PFMPE_OPT_MULTI_MAX_BLOCKS)");
  const size_t need = batch_layout<Desc>(S, total, tbytes).need;
  if (need > std::min(c0->d_multi.bytes(), c0->h_multi.bytes())) {
    c0->map_sig.clear();  // a new scratch holds no map
    const size_t cap = std::max(need * 2, (size_t)1 << 16);
    RET(c0->d_multi.grow(c0, need, cap));
    // read by k_stage_multi over PCIe: mapped, coherent (the host rewrites it between batches)
    RET(c0->h_multi.grow(c0, need, cap));
  }
  for (int s = 0; s < S; ++s) RET(ensure_prop(cs[s]));
  RET((audit_batch<T, SP>(cs, S, fas.data(), in, toff, tbytes, total, c0->d_multi.bytes())));
  if (!c0->lead_fence) {  // created before any member's ordering state changes (no early return after)
    auto f = std::make_shared<BatchFence>();
    HIPCHK(c0, hipEventCreateWithFlags(&f->ev, hipEventDisableTiming));
    f->stream = c0->stream;
    c0->lead_fence = f;
  } else {
    // a context of the leader's previous batch that is not in this one: its fence ends before this batch (members of
    // both batches need no fence: their work stays on this stream; a steady loop of batches records nothing)
    long held = 0;
    for (int s = 0; s < S; ++s) held += cs[s]->last_fence.get() == c0->lead_fence.get();
    if (c0->lead_fence.use_count() - 1 > held) RET(seal_lead_fence(c0));
  }
  // every member's work so far is ordered before the batch (its own stream, or an earlier batch led elsewhere).
  // order_after clears a member's ordering state; if a later member's ordering fails, the earlier ones get their
  // state back (their pending work is still unordered with their own streams)
  {
    OrderGuard members(cs, S);
    RET(members.order(0, c0->stream, c0));
    members.commit();  // from here to the fence below there is no return
  }
  std::vector<const unsigned char*> tables(S);
  for (int s = 0; s < S; ++s) {
    pfmpe_ctx* c = cs[s];
    if (in[s].bank_frame >= 0) {
      tables[s] = c->d_bank.get() + c->bank_off[in[s].bank_frame];
    } else {
      std::memcpy(c0->h_multi.get() + toff[s], hosttab[s].data(), (size_t)fas[s].tbytes);
      tables[s] = c0->d_multi.get() + toff[s];
    }
  }
  const int rc = visit_m(maxM, all5, [&](auto m) {
    return Seq<T, RNG, decltype(m)::value, SP>::step_multi(cs, S, fas.data(), tables.data(), c0->h_multi.get(),
                                                           c0->h_multi.dev(), c0->d_multi.get(), tbytes);
  });
  // the batch's kernels may still be retiring when the records are in (or when a step failed part-way): each
  // member's next work on its own stream is ordered after the leader's stream through the fence, recorded when
  // that work comes (the leader's own stream is the batch stream).  Set whatever step_multi returned.
  for (int s = 0; s < S; ++s) {
    cs[s]->last_stream = c0->stream;
    cs[s]->last_fence = s == 0 ? nullptr : c0->lead_fence;
  }
  c0->lead_fence->recorded = false;  // this batch is not in the event yet
  return rc;
}

template <typename T, int RNG, typename SP>
int regen_m(pfmpe_ctx* c, int kept_iter, const void* prior, double* out) {
  return Seq<T, RNG, 8, SP>::regen(c, kept_iter, prior, out);
}
template <typename T, int RNG, typename SP>
int regen_list_m(pfmpe_ctx* c, int kept_iter, const void* prior, const int32_t* list, const uint32_t* count, int limit,
                 double* out) {
  return Seq<T, RNG, 8, SP>::regen_list(c, kept_iter, prior, list, count, limit, out);
}

}  // namespace pfmpe_impl
