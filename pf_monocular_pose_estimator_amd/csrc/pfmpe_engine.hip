// pfmpe_engine.hip — host side of the MI355X PF engine: context, buffers, C-ABI (include/pfmpe.h).
//
// Replaces the PF block of PoseEstimator::estimateBodyPose (pf_mpe_lib/src/pose_estimator.cpp:475-733).
// The launch sequences live in pfmpe_seq.hpp (Seq) and are instantiated per (state type, RNG) in the
// pfmpe_k_*.hip translation units; this unit holds the context's life, the step with its tail, the read-backs, the
// statistics of the timing brackets, and builds the blob tables.  Every side call (ROI, cloud statistics,
// association, refinement, top-K, initialisation, detector) is in the unit of its kernels.
#include "pf_gn.hpp"
#include "pf_likelihood.hpp"
#include "pf_tail.hpp"
#include "pfmpe_prior.hpp"

using namespace pfmpe_impl;

PFMPE_DECLARE_INSTANCE(float, kRngReference, float, extern)
PFMPE_DECLARE_INSTANCE(float, kRngPhilox, float, extern)
PFMPE_DECLARE_INSTANCE(double, kRngReference, double, extern)
PFMPE_DECLARE_INSTANCE(double, kRngPhilox, double, extern)
PFMPE_DECLARE_INSTANCE(float, kRngReference, __half, extern)
PFMPE_DECLARE_INSTANCE(float, kRngPhilox, __half, extern)

// ---- used by the side calls' units as well (declared in pfmpe_ctx.hpp)
namespace pfmpe_impl {

int dispatch_regen(pfmpe_ctx* c, int kept_iter, const void* prior, double* out) {
  return visit_state_rng(c, [&](auto s) {
    using S = decltype(s);
    return regen_m<typename S::T, S::RNG, typename S::SP>(c, kept_iter, prior, out);
  });
}

int dispatch_regen_list(pfmpe_ctx* c, int kept_iter, const void* prior, const int32_t* list, const uint32_t* count,
                        int limit, double* out) {
  return visit_state_rng(c, [&](auto s) {
    using S = decltype(s);
    return regen_list_m<typename S::T, S::RNG, typename S::SP>(c, kept_iter, prior, list, count, limit, out);
  });
}

// byte offset of a table's GridHdr
size_t grid_off(const pfmpe_ctx* c, int B) {
  return visit_state(c, [&](auto s) { return BlobTable<typename decltype(s)::T>::off_grid(B); });
}
// the frame's blob table for the context's current parameters (pruning half-window as build_args computes
// it); returns its size
size_t build_table(const pfmpe_ctx* c, const double* blobs, int B, unsigned char* dst) {
  return visit_state(c, [&](auto s) {
    using T = typename decltype(s)::T;
    return build_blob_table_host<T>(blobs, B, (double)(T)(c->params.tol_pf * (1.0 + 1e-3) + 1e-3), dst);
  });
}

int export_prior(pfmpe_ctx* c, int count) { return export_prior(c, count, c->stream, c); }

}  // namespace pfmpe_impl

namespace {

int dispatch_step(pfmpe_ctx* c, const pfmpe_frame_in* in, const unsigned char* table, size_t tbytes,
                  const GridHdr& gh) {
  return visit_state_rng(c, [&](auto s) {
    using S = decltype(s);
    return dispatch_m<typename S::T, S::RNG, typename S::SP>(c, in, table, tbytes, gh);
  });
}

// largest blob table of this context's type (base part at kMaxBlobs + the largest grid)
size_t table_max_bytes(const pfmpe_ctx* c) {
  return visit_state(c, [&](auto s) { return BlobTable<typename decltype(s)::T>::max_bytes(); });
}

// pfmpe_step's argument and state checks (also per stream of pfmpe_step_multi)
int check_step(pfmpe_ctx* c, const pfmpe_frame_in* in, const pfmpe_frame_out* out) {
  if (!c) return PFMPE_E_ARG;
  if (!in || !out) return fail(c, PFMPE_E_ARG, "step: null in/out");
  if (!c->has_model || !c->has_prior) return fail(c, PFMPE_E_STATE, "step: set_model and set_prior first");
  if (in->B < 0) return fail(c, PFMPE_E_ARG, "step: B < 0");
  if (in->force_iters < 0 || in->force_iters > kMaxIter) return fail(c, PFMPE_E_ARG, "step: force_iters out of range");
  if (in->B > c->max_blobs) return fail(c, PFMPE_E_CAP, "step: B exceeds max_blobs");
  if (in->it_since_init >= 2 && !(in->dt != 0.0))
    return fail(c, PFMPE_E_ARG, "step: dt must be non-zero in steady state");
  if (in->bank_frame >= 0) {
    if (!c->d_bank.get() || in->bank_frame >= (int)c->bank_B.size())
      return fail(c, PFMPE_E_ARG, "step: bank_frame out of range");
    if (c->bank_B[in->bank_frame] != in->B) return fail(c, PFMPE_E_ARG, "step: B does not match the staged bank frame");
  } else if (in->B > 0 && !in->blobs) {
    return fail(c, PFMPE_E_ARG, "step: null blobs");
  }
  return PFMPE_OK;
}

// the frame record into pfmpe_frame_out, and the context's state after the frame (PE:681, 727)
void take_step(pfmpe_ctx* c, const pfmpe_frame_in* in, pfmpe_frame_out* out) {
  const OutDev& o = *c->h_out;
  out->iters = o.iters;
  out->kept_iter = o.kept_iter;
  out->most_likely_idx = o.most_likely_idx;
  out->accepted = o.accepted;
  out->resampled = o.resampled;
  out->winner_idx = o.winner_idx;
  out->n_corr = o.n_corr;
  out->flag_fail = o.flag_fail;
  out->highest_prob = o.highest_prob;
  out->prob_sum = o.prob_sum;
  std::memcpy(out->winner_pose, o.winner_pose, sizeof(out->winner_pose));
  std::memcpy(out->most_likely_pose, o.most_likely_pose, sizeof(out->most_likely_pose));
  std::memcpy(out->corr, o.corr, sizeof(out->corr));

  c->has_last = true;
  c->last_prior_idx = c->prior_idx;
  c->last_accepted = o.resampled != 0;
  c->last_kept_slot = o.kept_slot;
  c->last_kept_iter = o.kept_iter;
  if (o.resampled) {  // newPoseEstimation = resampled set (PE:681, 727), anchored at this frame's current pose
    if (c->frame_owner_out >= 0 && c->d_owner[c->frame_owner_out] && o.kept_slot >= 0 && o.kept_slot < 2 &&
        c->d_prop[o.kept_slot]) {
      // deferred resampling: the kept buffer is the new prior's storage (read through the owner indices k_resample
      // wrote); the unused post buffer becomes that weight slot's kept buffer for the next frame
      c->d_prop[o.kept_slot].swap(c->d_state[1 - c->prior_idx]);
      c->prior_owner = c->frame_owner_out;
    } else {
      c->prior_owner = -1;
    }
    c->frame_owner_out = -1;
    c->prior_idx = 1 - c->prior_idx;
    std::memcpy(c->anchor[c->prior_idx], in->current_pose, 12 * sizeof(double));
  }
}

}  // namespace

// ======================================================================================= C-ABI
extern "C" {

int pfmpe_abi_version(void) { return PFMPE_ABI_VERSION; }

void pfmpe_default_params(pfmpe_params* p) {
  if (!p) return;
  // README.md:338-361 launch defaults; constants of PE:563, 616, 633
  p->tol = 5.0;
  p->tol_pf = 4.0;
  p->ang_min = -0.015;
  p->ang_max = 0.015;
  p->trans_min = -0.035;
  p->trans_max = 0.035;
  p->growth = 0.025;
  p->max_iter = 80;
  p->exit_cap = 5;
  p->accept_cap = 3;
  p->rng_mode = PFMPE_RNG_PHILOX;
}

int pfmpe_create(pfmpe_ctx** out, int hip_device, int max_particles, int max_markers, int max_blobs,
                 int state_dtype) {
  if (!out) return PFMPE_E_ARG;
  *out = nullptr;
  if (max_particles < 1 || max_markers < 1 || max_markers > kMaxMarkers || max_blobs < 0 ||
      max_blobs > kMaxBlobs ||
      (state_dtype != PFMPE_STATE_F32 && state_dtype != PFMPE_STATE_F64 && state_dtype != PFMPE_STATE_F16))
    return PFMPE_E_ARG;
  pfmpe_ctx* c = new pfmpe_ctx();
  c->device = hip_device;
  c->max_particles = max_particles;
  c->max_markers = max_markers;
  c->max_blobs = max_blobs;
  c->state_dtype = state_dtype;
  c->es = state_dtype == PFMPE_STATE_F64 ? 8 : (state_dtype == PFMPE_STATE_F16 ? 2 : 4);
  c->ws = state_dtype == PFMPE_STATE_F64 ? 8 : 4;
  c->ld = ((int64_t)max_particles + 63) / 64 * 64;

  c->max_blk = (max_particles + kBlock - 1) / kBlock;
  // fp32 / fp16 planes are addressed through one 32-bit buffer resource per state buffer
  // (pf_state.hpp BufPlanes): 12 planes must stay below 4 GiB (89M fp32 / 178M fp16 particles)
  if (state_dtype != PFMPE_STATE_F64 && (int64_t)kPlanes * c->ld * (int64_t)c->es >= ((int64_t)1 << 32)) {
    delete c;
    return PFMPE_E_CAP;
  }
  pfmpe_default_params(&c->params);
  auto bad = [&](int code) {
    delete c;
    return code;
  };
  if (hipSetDevice(hip_device) != hipSuccess) return bad(PFMPE_E_HIP);
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return bad(PFMPE_E_HIP);
  const size_t state_bytes = (size_t)kPlanes * c->ld * c->es;
  bool ok = true;
  auto got = [&](int rc) { ok = ok && rc == PFMPE_OK; };
  c->max_grp = c->max_blk;  // groups hold ~sqrt(blocks) blocks (build_args): size group buffers per block
  for (int i = 0; i < 2; ++i) {
    got(c->d_state[i].alloc(c, state_bytes));
    got(c->d_w[i].alloc(c, (size_t)c->max_blk * kBlock * c->ws));  // whole blocks: k_resample_owners
    // kWaves entries per block: the streaming weighing pass stores wave partials (k_group combines them)
    got(c->d_part[i].alloc(c, (size_t)c->max_blk * kWaves * sizeof(BlockPart)));
    got(c->d_bscan[i].alloc(c, (size_t)c->max_blk * sizeof(BlockScan)));
    got(c->d_gpart[i].alloc(c, (size_t)c->max_grp * sizeof(GroupPart)));
  }
  got(c->d_gscan.alloc(c, (size_t)c->max_grp * sizeof(GroupScan)));
  got(c->d_cpart.alloc(c, (size_t)(c->max_blk + 1) * sizeof(CountPart)));  // +1: 16-B reads
  got(c->d_cgroup.alloc(c, (size_t)c->max_grp * sizeof(CountPart)));
  got(c->d_winkey.alloc(c, kWinBytes));
  got(c->d_counters.alloc(c, counters_bytes(c)));
  got(c->d_ctrl.alloc(c, sizeof(Ctrl)));
  got(c->d_gen.alloc(c, sizeof(uint32_t)));
  got(c->d_cand.alloc(c, (size_t)c->max_blk * sizeof(Cand)));
  got(c->d_mlpose.alloc(c, 12 * sizeof(double)));
  got(c->d_flat.alloc(c, kFlatWords * sizeof(uint32_t)));
  got(c->d_gran.alloc(c, kGranBytes));
  {
    int coop = 0;
    ok = ok && hipDeviceGetAttribute(&c->num_cu, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess;
    ok = ok && hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, c->device) == hipSuccess;
    c->coop = coop != 0;
  }
  got(c->h_rec.alloc(c, sizeof(RecOut)));
  if (ok) {
    memset(c->h_rec.get(), 0, sizeof(RecOut));
    c->h_out.reset(new OutDev());
  }
  got(c->d_table.alloc(c, table_max_bytes(c)));
  got(c->h_table.alloc(c, table_max_bytes(c)));
  if (!ok) return bad(PFMPE_E_HIP);
  // Zeroed in the context's own stream and waited for: the stream is non-blocking, so a null-stream
  // hipMemset could still be in flight when the first frame's kernels read these words (freed memory of an
  // earlier context: a stale control record, counters or candidate tags).
  ok = ok && hipMemsetAsync(c->d_gen.get(), 0, sizeof(uint32_t), c->stream) == hipSuccess;
  ok = ok && hipMemsetAsync(c->d_ctrl.get(), 0, sizeof(Ctrl), c->stream) == hipSuccess;
  ok = ok && hipMemsetAsync(c->d_cand.get(), 0, (size_t)c->max_blk * sizeof(Cand), c->stream) == hipSuccess;
  ok = ok && hipMemsetAsync(c->d_counters.get(), 0, counters_bytes(c), c->stream) == hipSuccess;
  ok = ok && hipMemsetAsync(c->d_flat.get(), 0, kFlatWords * sizeof(uint32_t), c->stream) == hipSuccess;
  ok = ok && hipMemsetAsync(c->d_gran.get(), 0, kGranBytes, c->stream) == hipSuccess;  // no stale word holds a live tag
  ok = ok && hipMemsetAsync(c->d_winkey.get(), 0, kWinBytes, c->stream) == hipSuccess;
  ok = ok && hipMemsetAsync(c->d_state[0].get(), 0, state_bytes, c->stream) == hipSuccess;
  ok = ok && hipMemsetAsync(c->d_state[1].get(), 0, state_bytes, c->stream) == hipSuccess;
  ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;
  if (!ok) return bad(PFMPE_E_HIP);
  *out = c;
  return PFMPE_OK;
}

void pfmpe_destroy(pfmpe_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->last_fence && c->last_fence->stream) {  // a batch led by another context: its stream up to its end
    if (c->last_fence->recorded || hipEventRecord(c->last_fence->ev, c->last_fence->stream) == hipSuccess)
      (void)hipEventSynchronize(c->last_fence->ev);
    else
      (void)hipStreamSynchronize(c->last_fence->stream);
  }
  c->last_fence.reset();
  if (c->lead_fence) c->lead_fence->stream = nullptr;  // drained above; members find nothing pending
  c->lead_fence.reset();
  delete c;  // the buffers, then the events, the stream last (CtxQueue)
}

const char* pfmpe_last_error(const pfmpe_ctx* c) { return c ? c->err.c_str() : "null context"; }

int pfmpe_set_model(pfmpe_ctx* c, const double* markers_xyz, int M, const double* K, const uint8_t* downgrade) {
  if (!c) return PFMPE_E_ARG;
  if (!markers_xyz || !K || M < 1) return fail(c, PFMPE_E_ARG, "set_model: null markers/K or M < 1");
  if (M > c->max_markers) return fail(c, PFMPE_E_CAP, "set_model: M exceeds max_markers");
  c->M = M;
  std::memset(c->markers, 0, sizeof(c->markers));
  std::memcpy(c->markers, markers_xyz, sizeof(double) * 3 * M);
  std::memcpy(c->K, K, sizeof(c->K));
  c->downgrade = 0;
  if (downgrade)
    for (int j = 0; j < M; ++j)
      if (downgrade[j]) c->downgrade |= 1u << j;
  c->has_model = true;
  return PFMPE_OK;
}

static int build_bank(pfmpe_ctx* c);

int pfmpe_set_params(pfmpe_ctx* c, const pfmpe_params* p) {
  if (!c || !p) return PFMPE_E_ARG;
  if (!(p->tol > 0) || !(p->tol_pf >= 0) || p->max_iter < 1 || p->max_iter > kMaxIter || p->exit_cap < 0 ||
      p->accept_cap < 0 ||
      (p->rng_mode != PFMPE_RNG_REFERENCE && p->rng_mode != PFMPE_RNG_PHILOX))
    return fail(c, PFMPE_E_ARG, "set_params: invalid parameter");
  const bool retable = c->d_bank && p->tol_pf != c->bank_tol_pf;
  const pfmpe_params prev = c->params;
  c->params = *p;
  if (retable) {  // the staged bank's grids were built for another tol_PF
    int r = set_device(c);
    if (r == PFMPE_OK) r = build_bank(c);  // builds the new bank aside; the old one stays until it succeeds
    if (r != PFMPE_OK) c->params = prev;   // all or nothing: the previous parameters and bank stay in force
    return r;
  }
  return PFMPE_OK;
}

int pfmpe_set_option(pfmpe_ctx* c, int option, int64_t value) {
  if (!c) return PFMPE_E_ARG;
  switch (option) {
    case PFMPE_OPT_RECORD_COUNTS:
      c->record_counts = value != 0;
      if (c->record_counts && !c->d_counts) {
        RET(set_device(c));
        RET(c->d_counts.alloc(c, (size_t)c->max_blk * kBlock * sizeof(uint32_t)));  // whole blocks
      }
      return PFMPE_OK;
    case PFMPE_OPT_FUSED:
      if (value < 0 || value > 2) return fail(c, PFMPE_E_ARG, "set_option: FUSED is 0, 1 or 2");
      c->fused = c->fused_user = (int)value;
      c->clean_since_fallback = 0;
      return PFMPE_OK;
    case PFMPE_OPT_WAIT_BOUND_US:
      if (value < 1 || value > 40000000) return fail(c, PFMPE_E_ARG, "set_option: WAIT_BOUND_US is 1 .. 4e7");
      c->wait_bound_us = value;
      return PFMPE_OK;
    case PFMPE_OPT_FUSED_REARM:
      if (value < 0) return fail(c, PFMPE_E_ARG, "set_option: FUSED_REARM >= 0");
      c->fused_rearm = value;
      return PFMPE_OK;
    case PFMPE_OPT_PRUNE:
      c->prune = value != 0;
      return PFMPE_OK;
    case PFMPE_OPT_KEEP_PROPAGATED:
      c->keep_prop = value != 0;
      return PFMPE_OK;
    case PFMPE_OPT_DEFER_RESAMPLE:
      c->defer = value != 0;
      return PFMPE_OK;
    case PFMPE_OPT_MULTI_MAX_BLOCKS:
      if (value < 1 || value > kMultiMaxBlocks) return fail(c, PFMPE_E_ARG, "set_option: MULTI_MAX_BLOCKS is 1 .. 160000");
      c->multi_max_blocks = value;
      return PFMPE_OK;
    case PFMPE_OPT_TIMING:
      if (value < 0 || value > (1 << 20)) return fail(c, PFMPE_E_ARG, "set_option: timing period out of range");
      c->timing = (int)value;
      c->timing_frame = 0;
      // the brackets' events are created now, not by the first timed frames: hipEventCreate inside a timed frame
      // had added its cost to every bracket of a short run (the pool starts empty)
      if (value > 0 && c->ev_pool.size() < kEventPrealloc) {
        RET(set_device(c));
        while (c->ev_pool.size() < kEventPrealloc) {
          EventPair p{};
          HIPCHK(c, hipEventCreate(&p.a));
          HIPCHK(c, hipEventCreate(&p.b));
          c->ev_pool.push_back(p);
        }
      }
      return PFMPE_OK;
    case 99:  // undocumented: diagnostic kernel switches for timing experiments
      c->diag = (int)value;
      if ((c->diag & kDiagStamps) && !c->d_stamps) {
        RET(set_device(c));
        RET(c->d_stamps.alloc(c, (1 + (size_t)c->max_blk) * kStamps * sizeof(uint64_t)));
        HIPCHK(c, hipMemsetAsync(c->d_stamps.get(), 0, (1 + (size_t)c->max_blk) * kStamps * sizeof(uint64_t), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
      }
      return PFMPE_OK;
    default:
      return fail(c, PFMPE_E_ARG, "set_option: unknown option");
  }
}

int pfmpe_set_prior(pfmpe_ctx* c, const double* poses, int N) {
  if (!c) return PFMPE_E_ARG;
  if (!poses || N < 1) return fail(c, PFMPE_E_ARG, "set_prior: null poses or N < 1");
  if (N > c->max_particles) return fail(c, PFMPE_E_CAP, "set_prior: N exceeds max_particles");
  RET(set_device(c));
  RET(ensure_xfer(c));
  HIPCHK(c, hipMemcpyAsync(c->d_xfer.get(), poses, (size_t)N * 12 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  // fp16 state: the set's anchor is its first particle (deltas of a concentrated set stay small)
  return import_prior(c, N, poses);
}

// (Re)builds the device bank from c->bank_blobs / bank_offsets with the parameters current now.  The table of a
// frame carries a grid whose window is tol_PF's: set_params rebuilds the bank when tol_PF changes, so a bank
// staged before set_params (or a later change) never leaves the frames on the slower x-bucket path
// (ADVICE r03).
// The new bank is built beside the old one and swapped in only once it is on the device, so a failure (an
// allocation or copy error) leaves the previous bank, its tables and its tol_PF in force.
static int build_bank(pfmpe_ctx* c) {
  const int nframes = (int)c->bank_offsets.size() - 1;
  std::vector<size_t> off(nframes + 1, 0);
  std::vector<int32_t> nb(nframes, 0);
  std::vector<GridHdr> grid(nframes, GridHdr{});
  std::vector<unsigned char> host, one(table_max_bytes(c));
  for (int f = 0; f < nframes; ++f) {
    nb[f] = c->bank_offsets[f + 1] - c->bank_offsets[f];
    const size_t n = build_table(c, c->bank_blobs.data() + 2 * (size_t)c->bank_offsets[f], nb[f], one.data());
    host.insert(host.end(), one.begin(), one.begin() + n);
    off[f + 1] = off[f] + n;
    grid[f] = *(const GridHdr*)(one.data() + grid_off(c, nb[f]));
  }
  Buf<unsigned char> d;
  RET(d.alloc(c, host.size()));
  hipError_t e = hipMemcpyAsync(d.get(), host.data(), host.size(), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // `host` goes out of scope; frames read in this stream
  if (e != hipSuccess) return fail(c, PFMPE_E_HIP, std::string("build_bank: ") + hipGetErrorString(e));
  c->d_bank.swap(d);  // the old bank is freed with `d`: the stream is idle (synchronised above)
  c->bank_off.swap(off);
  c->bank_B.swap(nb);
  c->bank_grid.swap(grid);
  c->bank_tol_pf = c->params.tol_pf;
  return PFMPE_OK;
}

int pfmpe_stage_blob_bank(pfmpe_ctx* c, const double* blobs, const int32_t* offsets, int nframes) {
  if (!c) return PFMPE_E_ARG;
  if (!blobs || !offsets || nframes < 1) return fail(c, PFMPE_E_ARG, "stage_blob_bank: bad arguments");
  for (int f = 0; f < nframes; ++f) {
    const int B = offsets[f + 1] - offsets[f];
    if (B < 0 || offsets[f] < 0) return fail(c, PFMPE_E_ARG, "stage_blob_bank: offsets not monotone");
    if (B > c->max_blobs) return fail(c, PFMPE_E_CAP, "stage_blob_bank: frame exceeds max_blobs");
  }
  RET(set_device(c));
  c->bank_offsets.assign(offsets, offsets + nframes + 1);
  c->bank_blobs.assign(blobs + 2 * (size_t)offsets[0], blobs + 2 * (size_t)offsets[nframes]);
  for (auto& o : c->bank_offsets) o -= offsets[0];
  return build_bank(c);
}

// pfmpe_step behind its checks (also pfmpe_step_refine's frame)
static int step_run(pfmpe_ctx* c, const pfmpe_frame_in* in, pfmpe_frame_out* out) {
  RET(set_device(c));
  const unsigned char* table = c->d_table.get();
  const int B = in->B;
  size_t tbytes = 0;
  GridHdr gh{};
  if (in->bank_frame >= 0) {
    table = c->d_bank.get() + c->bank_off[in->bank_frame];
    tbytes = c->bank_off[in->bank_frame + 1] - c->bank_off[in->bank_frame];
    gh = c->bank_grid[in->bank_frame];
  } else {
    // the x-bucketed table is built here, O(B), and travels in the same copy the blobs would
    tbytes = build_table(c, in->blobs, B, c->h_table.get());
    gh = *(const GridHdr*)(c->h_table.get() + grid_off(c, B));
    HIPCHK(c, hipMemcpyAsync(c->d_table.get(), c->h_table.get(), tbytes, hipMemcpyHostToDevice, c->stream));
  }
  c->timing_now = c->timing > 0 && (c->timing_frame++ % c->timing) == 0;
  const size_t ev_mark = c->ev_used;  // brackets of earlier frames still pending (harvested lazily)
  const int rs = dispatch_step(c, in, table, tbytes, gh);
  c->timing_now = false;
  if (rs != PFMPE_OK) c->ev_used = ev_mark;  // only the failed frame's own brackets are dropped
  else if (c->ev_used >= kHarvestPairs) RET(harvest_timing(c));  // pending brackets: harvest_timing
  RET(rs);
  take_step(c, in, out);
  return PFMPE_OK;
}

int pfmpe_step(pfmpe_ctx* c, const pfmpe_frame_in* in, pfmpe_frame_out* out) {
  RET(check_step(c, in, out));
  return step_run(c, in, out);
}

// pfmpe_step_multi's checks under the entry point's name `who` (also pfmpe_step_refine_multi's), and the batch behind
// them
static int step_multi_check(pfmpe_ctx* const* ctxs, int S, const pfmpe_frame_in* in, pfmpe_frame_out* out,
                            const std::string& who) {
  if (!ctxs || S < 1 || !ctxs[0]) return PFMPE_E_ARG;
  pfmpe_ctx* c0 = ctxs[0];
  if (!in || !out) return fail(c0, PFMPE_E_ARG, who + ": null in/out");
  if (S > 65535) return fail(c0, PFMPE_E_CAP, who + ": at most 65535 streams per batch");
  return check_members(
      ctxs, S, who.c_str(), "device, state type, RNG mode and pruning",
      [&](const pfmpe_ctx* c) { return c->params.rng_mode == c0->params.rng_mode && c->prune == c0->prune; },
      [&](int s, const std::string& at) {
        const int rc = check_step(ctxs[s], &in[s], &out[s]);
        return rc == PFMPE_OK ? rc : fail(c0, rc, at + ctxs[s]->err);  // the per-stream code (E_ARG / E_CAP / E_STATE)
      });
}
static int step_multi_run(pfmpe_ctx* const* ctxs, int S, const pfmpe_frame_in* in, pfmpe_frame_out* out) {
  pfmpe_ctx* c0 = ctxs[0];
  c0->mt_enter = now_ns();
  RET(set_device(c0));
  c0->timing_now = c0->timing > 0 && (c0->timing_frame++ % c0->timing) == 0;  // batches timed on the leader
  const size_t ev_mark = c0->ev_used;
  const int rs = visit_state_rng(c0, [&](auto s) {
    using S_ = decltype(s);
    return multi_m<typename S_::T, S_::RNG, typename S_::SP>(ctxs, S, in);
  });
  c0->timing_now = false;
  if (rs != PFMPE_OK) c0->ev_used = ev_mark;  // only the failed batch's own brackets are dropped
  else if (c0->ev_used >= kHarvestPairs) RET(harvest_timing(c0));
  RET(rs);
  const int64_t t_r = now_ns();
  for (int s = 0; s < S; ++s) {
    take_step(ctxs[s], &in[s], &out[s]);
    if (!ctxs[s]->fused) ctxs[s]->clean_since_fallback += 1;  // a clean two-launch frame (PFMPE_OPT_FUSED_REARM)
  }
  c0->mt_ns[3] += now_ns() - t_r;
  c0->mt_batches += 1;
  return PFMPE_OK;
}

int pfmpe_step_multi(pfmpe_ctx* const* ctxs, int S, const pfmpe_frame_in* in, pfmpe_frame_out* out) {
  RET(step_multi_check(ctxs, S, in, out, "step_multi"));
  return step_multi_run(ctxs, S, in, out);
}

int pfmpe_step_multi_batch(pfmpe_ctx* const* ctxs, int S, const pfmpe_frame_in* in, int n, pfmpe_frame_out* out,
                           int* done) {
  if (done) *done = 0;
  if (!ctxs || S < 1 || !ctxs[0]) return PFMPE_E_ARG;
  if ((!in || !out) && n > 0) return fail(ctxs[0], PFMPE_E_ARG, "step_multi_batch: null in/out");
  for (int f = 0; f < n; ++f) {
    RET(pfmpe_step_multi(ctxs, S, in + (size_t)f * S, out + (size_t)f * S));
    if (done) *done = f + 1;
  }
  return PFMPE_OK;
}

int pfmpe_step_batch(pfmpe_ctx* c, const pfmpe_frame_in* in, int n, pfmpe_frame_out* out, int* done) {
  if (!c) return PFMPE_E_ARG;
  if (done) *done = 0;
  if ((!in || !out) && n > 0) return fail(c, PFMPE_E_ARG, "step_batch: null in/out");
  for (int f = 0; f < n; ++f) {
    RET(pfmpe_step(c, in + f, out + f));
    if (done) *done = f + 1;
  }
  return PFMPE_OK;
}

int pfmpe_get_particles(pfmpe_ctx* c, int which, double* out) {
  if (!c) return PFMPE_E_ARG;
  if (!out || (which != 0 && which != 1)) return fail(c, PFMPE_E_ARG, "get_particles: bad arguments");
  if (!c->has_prior) return fail(c, PFMPE_E_STATE, "get_particles: no particle set");
  if (which == 0 && !c->has_last) return fail(c, PFMPE_E_STATE, "get_particles(0): no step yet");
  RET(set_device(c));
  RET(ensure_xfer(c));
  const int N = c->N;
  if (which == 0)
    RET(dispatch_regen(c, c->last_kept_iter, c->d_state[c->last_prior_idx].get(), c->d_xfer.get()));
  else
    RET(export_prior(c, N));
  HIPCHK(c, hipMemcpyAsync(out, c->d_xfer.get(), (size_t)N * 12 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  RET(harvest_timing(c));
  return PFMPE_OK;
}

int pfmpe_get_weights(pfmpe_ctx* c, double* out) {
  if (!c) return PFMPE_E_ARG;
  if (!out) return fail(c, PFMPE_E_ARG, "get_weights: null out");
  if (!c->has_last) return fail(c, PFMPE_E_STATE, "get_weights: no step yet");
  RET(set_device(c));
  RET(ensure_xfer(c));
  const int N = c->N;
  visit_state(c, [&](auto s) {
    using T = typename decltype(s)::T;
    hipLaunchKernelGGL((k_weights_export<T>), dim3((N + 255) / 256), dim3(256), 0, c->stream,
                       (const T*)c->d_w[c->last_kept_slot].get(), c->d_xfer.get(), N);
  });
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out, c->d_xfer.get(), (size_t)N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PFMPE_OK;
}

int pfmpe_get_counts(pfmpe_ctx* c, uint32_t* out) {
  if (!c) return PFMPE_E_ARG;
  if (!out) return fail(c, PFMPE_E_ARG, "get_counts: null out");
  if (!c->record_counts || !c->d_counts.get()) return fail(c, PFMPE_E_STATE, "get_counts: PFMPE_OPT_RECORD_COUNTS off");
  if (!c->has_last || !c->last_accepted) return fail(c, PFMPE_E_STATE, "get_counts: last step did not resample");
  RET(set_device(c));
  // in the context's stream: the frame's kernel may still be retiring after its record reached the host
  HIPCHK(c, hipMemcpyAsync(out, c->d_counts.get(), (size_t)c->N * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PFMPE_OK;
}

// ---- the step with its refinement (pf_tail.hpp; k_step_tail in pfmpe_refine.hip)
namespace {
// pfmpe_refine_poses' summary of one hypothesis from its row and covariance (k_refine + k_refine_fold for K = 1)
void tail_summary(const pfmpe_refine_row& r, const double* cov, pfmpe_refine_out* o) {
  std::memset(o, 0, sizeof(*o));
  o->n = 1;
  o->n_with_pairs = r.n_pairs > 0 ? 1 : 0;
  o->n_converged = r.status == PFMPE_REFINE_CONVERGED ? 1 : 0;
  o->n_cap_kept = r.status == PFMPE_REFINE_CAP_KEPT ? 1 : 0;
  o->n_cap_reverted = r.status == PFMPE_REFINE_CAP_REVERTED ? 1 : 0;
  o->iters_total = r.iters;
  o->iters_max = r.iters;
  o->best = -1;
  if (gn_eligible(r)) {
    o->best = 0;
    o->best_row = r;
    std::memcpy(o->best_cov, cov, sizeof(o->best_cov));
  }
}
// its K = 0 summary
void tail_empty(pfmpe_refine_out* o) {
  std::memset(o, 0, sizeof(*o));
  o->best = -1;
}

// The staging block of S streams: the descriptors, the tail records, then every stream's model and blobs.
struct TailLayout {
  size_t rec_off, in_off;
  static size_t align(size_t x) { return (x + 255) / 256 * 256; }
  explicit TailLayout(int S) : rec_off(align((size_t)S * sizeof(TailDesc))), in_off(rec_off + (size_t)S * sizeof(TailRec)) {}
  static size_t stream_bytes(int B) { return align(kTailModelBytes + 2 * (size_t)B * sizeof(double)); }
};
struct TailStream {
  const pfmpe_ctx* c;
  const double* blobs;  // the caller's list, or the bank frame's host copy
  int B;
  pfmpe_refine_params prm;
};
// the step's blobs in fp64 (check_step has validated the request)
void tail_blobs(const pfmpe_ctx* c, const pfmpe_frame_in* in, TailStream* st) {
  st->c = c;
  st->B = in->B;
  st->blobs = in->bank_frame >= 0 ? c->bank_blobs.data() + 2 * (size_t)c->bank_offsets[in->bank_frame] : in->blobs;
}
// Written once per call, before the first launch: every record's granules zeroed (no word of an earlier call carries
// a tag this call waits for), the descriptors, the models and the blobs.  Nothing of an earlier call is pending on
// the leader's stream (the calls are blocking; a failed frame drained it).
int tail_stage(pfmpe_ctx* c0, const std::vector<TailStream>& st) {
  const int S = (int)st.size();
  const TailLayout L(S);
  size_t need = L.in_off;
  for (const TailStream& t : st) need += TailLayout::stream_bytes(t.B);
  if (need > UINT32_MAX) return fail(c0, PFMPE_E_CAP, "step_refine: the staging block exceeds 4 GiB");
  RET(c0->h_tail.grow(c0, need, need + need / 2));
  unsigned char* h = c0->h_tail.get();
  unsigned char* d = c0->h_tail.dev();
  std::memset(h + L.rec_off, 0, (size_t)S * sizeof(TailRec));
  size_t off = L.in_off;
  for (int s = 0; s < S; ++s) {
    const pfmpe_ctx* c = st[s].c;
    TailDesc x{};
    x.rec = ((const RecOut*)c->h_rec.dev())->g;
    x.out = ((TailRec*)(d + L.rec_off) + s)->g;
    x.model_off = (uint32_t)off;
    x.blobs_off = (uint32_t)(off + kTailModelBytes);
    x.seq0 = c->seq;
    x.M = c->M;
    x.B = st[s].B;
    x.max_iter = st[s].prm.max_iter;
    x.revert = st[s].prm.revert_on_divergence ? 1 : 0;
    x.converged = st[s].prm.converged;
    std::memcpy(h + (size_t)s * sizeof(TailDesc), &x, sizeof(x));
    std::memcpy(h + off, c->markers, sizeof(c->markers));
    std::memcpy(h + off + sizeof(c->markers), c->K, sizeof(c->K));
    if (st[s].B > 0) std::memcpy(h + x.blobs_off, st[s].blobs, 2 * (size_t)st[s].B * sizeof(double));
    off += TailLayout::stream_bytes(st[s].B);
  }
  __atomic_thread_fence(__ATOMIC_RELEASE);
  return PFMPE_OK;
}
static_assert(sizeof(((pfmpe_ctx*)nullptr)->markers) + sizeof(((pfmpe_ctx*)nullptr)->K) <= kTailModelBytes, "tail model");

// Stream s's tail record of frame sequence `want`, awaited like the frame record (wait_frame): a bounded spin on the
// tags with the hipStreamQuery backstop.  Returns the record's state with row / cov unpacked for kTailRefined;
// kTailNotReady also when the stream is idle (or in error) without a record.
uint32_t tail_wait(pfmpe_ctx* c0, int S, int s, int32_t want, pfmpe_refine_row* row, double* cov) {
  volatile const uint64_t* g = ((const TailRec*)(c0->h_tail.get() + TailLayout(S).rec_off) + s)->g;
  auto take = [&](uint32_t* state) {
    const uint32_t t = (uint32_t)(g[0] >> 32);
    if (t == 0u || (int32_t)(t >> 2) != want) return false;
    *state = t & 3u;
    if (*state != kTailRefined) return true;
    for (int k = kTailWords - 1; k > 0; --k)
      if ((uint32_t)(g[k] >> 32) != t) return false;
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    uint32_t w[kTailWords];
    for (int k = 0; k < kTailWords; ++k) w[k] = (uint32_t)g[k];
    std::memcpy(row, w + 1, sizeof(*row));
    std::memcpy(cov, w + 1 + kTailRowWords, 36 * sizeof(double));
    return true;
  };
  uint32_t state = kTailNotReady;
  int64_t next_query = 0;
  for (uint64_t spin = 0;; ++spin) {
    if (take(&state)) return state;
    if ((spin & 63u) != 63u) {
      __builtin_ia32_pause();
      continue;
    }
    const int64_t t = now_ns();
    if (next_query == 0) next_query = t + kQueryAfterNs;
    if (t >= next_query) {
      next_query = t + kQueryAfterNs;
      if (hipStreamQuery(c0->stream) != hipErrorNotReady) return take(&state) ? state : (uint32_t)kTailNotReady;
    }
    __builtin_ia32_pause();
  }
}

// One stream's results from its tail record; the recovery path (never an error of its own, never a retry) when the
// record is "not ready" or absent: the host-driven refinement of the frame's winner, the same bytes.
int tail_collect(pfmpe_ctx* c0, int S, int s, pfmpe_ctx* c, const TailStream& st, const pfmpe_frame_out* out,
                 pfmpe_refine_out* gn, pfmpe_refine_row* row, double* cov36) {
  pfmpe_refine_row r;
  double cov[36];
  const uint32_t state = tail_wait(c0, S, s, c->seq, &r, cov);
  if (state == kTailRefined) {
    tail_summary(r, cov, gn);
    if (row) *row = r;
    if (cov36) std::memcpy(cov36, cov, sizeof(cov));
    return PFMPE_OK;
  }
  if (state == kTailEmpty) {
    tail_empty(gn);
    return PFMPE_OK;
  }
  c->tail_fallbacks += 1;
  if (!tail_wanted(out->flag_fail, out->winner_pose)) {
    tail_empty(gn);
    return PFMPE_OK;
  }
  pfmpe_assoc_in ain{};
  ain.blobs = st.blobs;
  ain.B = st.B;
  ain.bank_frame = -1;
  return pfmpe_refine_poses(c, &ain, &st.prm, out->winner_pose, out->corr, 1, gn, row, cov36);
}
// the fused call in flight on c's stream, ended on every path
struct TailScope {
  pfmpe_ctx* c;
  TailScope(pfmpe_ctx* c_, int S) : c(c_) {
    c->tail_S = S;
    c->tail_seq0 = c->seq;
  }
  ~TailScope() { c->tail_S = 0; }
};
}  // namespace

int pfmpe_step_refine(pfmpe_ctx* c, const pfmpe_frame_in* in, const pfmpe_refine_params* params, pfmpe_frame_out* out,
                      pfmpe_refine_out* gn, pfmpe_refine_row* row, double* cov36) {
  RET(check_step(c, in, out));
  std::vector<TailStream> st(1);
  pfmpe_default_refine_params(&st[0].prm);
  if (params) st[0].prm = *params;
  if (!gn) return fail(c, PFMPE_E_ARG, "step_refine: null gn");
  if (!refine_params_ok(st[0].prm)) return fail(c, PFMPE_E_ARG, "step_refine: bad parameters");
  tail_blobs(c, in, &st[0]);
  HIPCHK(c, hipSetDevice(c->device));
  RET(tail_stage(c, st));
  {
    TailScope scope(c, 1);
    RET(step_run(c, in, out));
  }
  return tail_collect(c, 1, 0, c, st[0], out, gn, row, cov36);
}

int pfmpe_step_refine_multi(pfmpe_ctx* const* ctxs, int S, const pfmpe_frame_in* in, const pfmpe_refine_params* params,
                            pfmpe_frame_out* out, pfmpe_refine_out* gn, pfmpe_refine_row* rows, double* cov) {
  RET(step_multi_check(ctxs, S, in, out, "step_refine_multi"));
  pfmpe_ctx* c0 = ctxs[0];
  if (!gn) return fail(c0, PFMPE_E_ARG, "step_refine_multi: null gn");
  std::vector<TailStream> st(S);
  for (int s = 0; s < S; ++s) {
    pfmpe_default_refine_params(&st[s].prm);
    if (params) st[s].prm = params[s];
    if (!refine_params_ok(st[s].prm))
      return fail(c0, PFMPE_E_ARG, "step_refine_multi: stream " + std::to_string(s) + ": bad parameters");
    tail_blobs(ctxs[s], &in[s], &st[s]);
  }
  HIPCHK(c0, hipSetDevice(c0->device));
  RET(tail_stage(c0, st));
  {
    TailScope scope(c0, S);
    RET(step_multi_run(ctxs, S, in, out));
  }
  for (int s = 0; s < S; ++s)
    RET(tail_collect(c0, S, s, ctxs[s], st[s], &out[s], &gn[s], rows ? rows + s : nullptr,
                     cov ? cov + 36 * (size_t)s : nullptr));
  return PFMPE_OK;
}

int pfmpe_host_step_tail(const double* markers_xyz, int M, const double* K, const double* blobs, int B,
                         const pfmpe_frame_out* frame, const pfmpe_refine_params* params, pfmpe_refine_out* gn,
                         pfmpe_refine_row* row, double* cov36) {
  pfmpe_refine_params prm;
  pfmpe_default_refine_params(&prm);
  if (params) prm = *params;
  if (!markers_xyz || !K || !frame || !gn || M < 1 || M > kMaxMarkers || B < 0 || (B > 0 && !blobs)) return PFMPE_E_ARG;
  if (!refine_params_ok(prm)) return PFMPE_E_ARG;
  if (!tail_wanted(frame->flag_fail, frame->winner_pose)) {
    tail_empty(gn);
    return PFMPE_OK;
  }
  double model[kMaxMarkers * 3] = {0}, zb[2 * kMaxMarkers] = {0}, c36[36];
  uint32_t lcorr[2 * kMaxMarkers];
  std::memcpy(model, markers_xyz, (size_t)M * 3 * sizeof(double));
  for (int j = 0; j < kMaxMarkers; ++j) {
    if (!tail_pair(frame->corr, j, M, B, lcorr + 2 * j)) return PFMPE_E_ARG;
    if (lcorr[2 * j + 1] != 0u) {
      zb[2 * j] = blobs[2 * (size_t)(frame->corr[2 * j + 1] - 1u)];
      zb[2 * j + 1] = blobs[2 * (size_t)(frame->corr[2 * j + 1] - 1u) + 1];
    }
  }
  pfmpe_refine_row r;
  tail_refine(model, K, zb, lcorr, prm.max_iter, prm.revert_on_divergence ? 1 : 0, prm.converged, frame->winner_pose, r,
              c36);
  tail_summary(r, c36, gn);
  if (row) *row = r;
  if (cov36) std::memcpy(cov36, c36, sizeof(c36));
  return PFMPE_OK;
}

// Undocumented diagnostic: reset (out == NULL) or read the kStamps stamps of the last frame (diag & 4).
int pfmpe_debug_stamps(pfmpe_ctx* c, uint64_t* out) {
  if (!c || !c->d_stamps) return PFMPE_E_STATE;
  RET(set_device(c));
  hipStream_t st = c->stream;
  const size_t rows = 1 + (size_t)c->max_blk;
  if (!out) {
    HIPCHK(c, hipMemsetAsync(c->d_stamps.get(), 0, rows * kStamps * sizeof(uint64_t), st));
    HIPCHK(c, hipStreamSynchronize(st));
    return PFMPE_OK;
  }
  std::vector<uint64_t> h(rows * kStamps);
  HIPCHK(c, hipMemcpyAsync(h.data(), c->d_stamps.get(), h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  for (int i = 0; i < kStamps; ++i) {
    const bool is_min = i == 0 || i == 4 || i == 19;
    uint64_t v = h[i];
    for (size_t r = 1; r < rows; ++r) {
      const uint64_t x = h[r * kStamps + i];
      if (!x) continue;
      if (!v || (is_min ? x < v : x > v)) v = x;
    }
    out[i] = v;
  }
  return PFMPE_OK;
}

int pfmpe_get_kernel_stats(pfmpe_ctx* c, int kernel, int64_t* launches, double* total_ms) {
  if (!c || kernel < 0 || kernel >= PFMPE_K_COUNT) return PFMPE_E_ARG;
  if (c->ev_used) {  // pending brackets of timed frames
    HIPCHK(c, hipSetDevice(c->device));
    RET(harvest_timing(c));
  }
  if (launches) *launches = c->k_launches[kernel];
  if (total_ms) *total_ms = c->k_ms[kernel];
  return PFMPE_OK;
}

int pfmpe_get_info(const pfmpe_ctx* c, int key, int64_t* value) {
  if (!c || !value) return PFMPE_E_ARG;
  switch (key) {
    case PFMPE_INFO_FUSED: *value = c->fused; return PFMPE_OK;
    case PFMPE_INFO_FUSED_FALLBACKS: *value = c->fused_fallbacks; return PFMPE_OK;
    case PFMPE_INFO_LAST_SHAPE: *value = c->last_shape; return PFMPE_OK;
    case PFMPE_INFO_LAST_WEIGH_PASS: *value = c->last_weigh_pass; return PFMPE_OK;
    case PFMPE_INFO_LAST_RESAMPLE: *value = c->last_resample; return PFMPE_OK;
    case PFMPE_INFO_LAST_GRID: *value = c->last_grid; return PFMPE_OK;
    case PFMPE_INFO_GUARD_SKIPS: *value = c->guard_skips; return PFMPE_OK;
    case PFMPE_INFO_N: *value = c->N; return PFMPE_OK;
    case PFMPE_INFO_NUM_CU: *value = c->num_cu; return PFMPE_OK;
    case PFMPE_INFO_TAIL_FALLBACKS: *value = c->tail_fallbacks; return PFMPE_OK;
    case 110: case 111: case 112: case 113: *value = c->mt_ns[key - 110]; return PFMPE_OK;  // batch host timing
    case 114: *value = c->mt_batches; return PFMPE_OK;
    case 115: *value = live_blocks().load(); return PFMPE_OK;  // buffers alive in this process (any context)
    default: return PFMPE_E_ARG;
  }
}

int pfmpe_reset_kernel_stats(pfmpe_ctx* c) {
  if (!c) return PFMPE_E_ARG;
  if (c->ev_used) {  // pending brackets belong to the statistics being reset
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventSynchronize(c->ev_pool[c->ev_used - 1].b));  // before their events are recorded again
    c->ev_used = 0;
  }
  for (int k = 0; k < PFMPE_K_COUNT; ++k) {
    c->k_launches[k] = 0;
    c->k_ms[k] = 0;
  }
  return PFMPE_OK;
}

const char* pfmpe_kernel_name(int kernel) {
  static const char* names[PFMPE_K_COUNT] = {"k_propagate_weigh", "k_resample", "aux", "k_frame", "k_roi",
                                                 "k_resample_final", "k_p3p_hist", "k_p3p_check",
                                                 "k_det (detector pipeline)"};
  return (kernel >= 0 && kernel < PFMPE_K_COUNT) ? names[kernel] : "?";
}

// ---- host-side evaluation of the device RNG code (CPU tests pin it against the oracle)
double pfmpe_host_ref_uniform(uint32_t seed, uint64_t j, double a, double b) {
  const uint32_t x0 = lcg_seed(seed);
  const uint32_t g1 = lcg_output(x0, 2 * j + 1);
  const uint32_t g2 = lcg_next(g1);
  return ref_uniform(ref_canonical(g1, g2), a, b);
}

void pfmpe_host_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  const U32x4 o = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
  out[0] = o.x;
  out[1] = o.y;
  out[2] = o.z;
  out[3] = o.w;
}

}  // extern "C"
