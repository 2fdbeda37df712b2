// pfmpe_engine.hip — host side of the MI355X PF engine: context, buffers, C-ABI (include/pfmpe.h).
//
// Replaces the PF block of PoseEstimator::estimateBodyPose (pf_mpe_lib/src/pose_estimator.cpp:475-733).
// The launch sequences live in pfmpe_seq.hpp (Seq) and are instantiated per (state type, RNG) in the
// pfmpe_k_*.hip translation units; this unit launches the side calls' kernels and builds the blob tables.
#include "pf_cloud.hpp"
#include "pf_gn.hpp"
#include "pf_likelihood.hpp"
#include "pf_roi.hpp"
#include "pf_tail.hpp"
#include "pf_top.hpp"
#include "pfmpe_prior.hpp"
#include "pfmpe_refine_plan.hpp"

using namespace pfmpe_impl;

PFMPE_DECLARE_INSTANCE(float, kRngReference, float, extern)
PFMPE_DECLARE_INSTANCE(float, kRngPhilox, float, extern)
PFMPE_DECLARE_INSTANCE(double, kRngReference, double, extern)
PFMPE_DECLARE_INSTANCE(double, kRngPhilox, double, extern)
PFMPE_DECLARE_INSTANCE(float, kRngReference, __half, extern)
PFMPE_DECLARE_INSTANCE(float, kRngPhilox, __half, extern)

namespace {

int dispatch_step(pfmpe_ctx* c, const pfmpe_frame_in* in, const unsigned char* table, size_t tbytes,
                  const GridHdr& gh) {
  return visit_state_rng(c, [&](auto s) {
    using S = decltype(s);
    return dispatch_m<typename S::T, S::RNG, typename S::SP>(c, in, table, tbytes, gh);
  });
}

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
// largest blob table of this context's type (base part at kMaxBlobs + the largest grid)
size_t table_max_bytes(const pfmpe_ctx* c) {
  return visit_state(c, [&](auto s) { return BlobTable<typename decltype(s)::T>::max_bytes(); });
}
// the frame's blob table for the context's current parameters (pruning half-window as build_args computes
// it); returns its size
size_t build_table(const pfmpe_ctx* c, const double* blobs, int B, unsigned char* dst) {
  return visit_state(c, [&](auto s) {
    using T = typename decltype(s)::T;
    return build_blob_table_host<T>(blobs, B, (double)(T)(c->params.tol_pf * (1.0 + 1e-3) + 1e-3), dst);
  });
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

namespace {
// project2d (PE:1017-1034) in double on the host: (K34 * T) * [X;1], then / z
void host_project(const double* K, const double* T12, const double* X, double* uv) {
  double Q[12];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = K[i * 3 + 0] * T12[0 * 4 + j];
      s = s + K[i * 3 + 1] * T12[1 * 4 + j];
      s = s + K[i * 3 + 2] * T12[2 * 4 + j];
      Q[i * 4 + j] = s;
    }
  double p[3];
  for (int i = 0; i < 3; ++i) {
    double s = Q[i * 4 + 0] * X[0];
    s = s + Q[i * 4 + 1] * X[1];
    s = s + Q[i * 4 + 2] * X[2];
    p[i] = s + Q[i * 4 + 3];
  }
  uv[0] = p[0] / p[2];
  uv[1] = p[1] / p[2];
}
// LEDDetector::distortPoints (led_detector.cpp:371-414) on cv::Point2f inputs, result back to float
void host_distort(const double* K, const double* D, float xin, float yin, float* xo, float* yo) {
  const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  const double k1 = D[0], k2 = D[1], p1 = D[2], p2 = D[3], k3 = D[4];
  const double x = ((double)xin - cx) / fx;
  const double y = ((double)yin - cy) / fy;
  const double r2 = x * x + y * y;
  double xc = x * (1. + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2);
  double yc = y * (1. + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2);
  xc = xc + (2. * p1 * x * y + p2 * (r2 + 2. * x * x));
  yc = yc + (p1 * (r2 + 2. * y * y) + 2. * p2 * x * y);
  *xo = (float)(xc * fx + cx);
  *yo = (float)(yc * fy + cy);
}
// The host end of every ROI entry point: bb = the particles' box {x_min, x_max, y_min, y_max} -> out.
void roi_epilogue(const double* K, const double* markers, int M, const pfmpe_roi_in* in, double* bb,
                  pfmpe_roi_out* out) {
  // + the markers at predicted_pose_ (PE:1049-1052)
  for (int m = 0; m < M; ++m) {
    double uv[2];
    host_project(K, in->predicted_pose, markers + 3 * m, uv);
    if (uv[0] < bb[0]) bb[0] = uv[0];
    if (uv[0] > bb[1]) bb[1] = uv[0];
    if (uv[1] < bb[2]) bb[2] = uv[1];
    if (uv[1] > bb[3]) bb[3] = uv[1];
  }
  std::memcpy(out->bbox, bb, 4 * sizeof(double));
  // determineROI (led_detector.cpp:317-368): corners as cv::Point2f, distorted, border, clamp, cv::Rect
  float x0f, y0f, x1f, y1f;
  host_distort(K, in->D, (float)bb[0], (float)bb[2], &x0f, &y0f);
  host_distort(K, in->D, (float)bb[1], (float)bb[3], &x1f, &y1f);
  const double W = in->image_w, H = in->image_h, b = in->border;
  const double x0 = std::max(0.0, std::min(W, (double)x0f - b));
  const double x1 = std::max(0.0, std::min(W, (double)x1f + b));
  const double y0 = std::max(0.0, std::min(H, (double)y0f - b));
  const double y1 = std::max(0.0, std::min(H, (double)y1f + b));
  if (x1 - x0 < 1 || y1 - y0 < 1) {
    out->x = 0;
    out->y = 0;
    out->width = in->image_w;
    out->height = in->image_h;
  } else {
    out->x = (int32_t)x0;
    out->y = (int32_t)y0;
    out->width = (int32_t)(x1 - x0);
    out->height = (int32_t)(y1 - y0);
  }
}
// the kernel arguments of context c's current prior for one ROI request
RoiArgs roi_args(const pfmpe_ctx* c, const pfmpe_roi_in* in) {
  RoiArgs ra{};
  std::memcpy(ra.cam, in->cam_move_inv, sizeof(ra.cam));
  std::memcpy(ra.predm, in->prediction, sizeof(ra.predm));
  std::memcpy(ra.K, c->K, sizeof(ra.K));
  std::memcpy(ra.markers, c->markers, sizeof(ra.markers));
  std::memcpy(ra.anchor, c->anchor[c->prior_idx], sizeof(ra.anchor));
  ra.N = c->N;
  ra.M = c->M;
  ra.ld = c->ld;
  ra.owner = prior_owner_ptr(c);
  return ra;
}
// what one stream of an ROI call must satisfy: its context c and its request; the text begins with `at`, on `err`
int roi_check_stream(pfmpe_ctx* err, const pfmpe_ctx* c, const pfmpe_roi_in* in, const std::string& at) {
  if (!c->has_model || !c->has_prior) return fail(err, PFMPE_E_STATE, at + "set_model and set_prior first");
  if (in->image_w < 1 || in->image_h < 1) return fail(err, PFMPE_E_ARG, at + "bad image size");
  return PFMPE_OK;
}
// The ROIs of S checked streams, 1 <= S <= kRoiMaxStreams, on ctxs[0]'s stream: pfmpe_predict_roi_multi and, as a
// batch of one, pfmpe_predict_roi.  The errors it can raise itself begin with `who`.
int roi_run(pfmpe_ctx* const* ctxs, int S, const pfmpe_roi_in* in, pfmpe_roi_out* out, const std::string& who) {
  pfmpe_ctx* c0 = ctxs[0];
  int64_t total = 0;
  for (int s = 0; s < S; ++s) total += (ctxs[s]->N + kBlock - 1) / kBlock;
  if (total > INT32_MAX) return fail(c0, PFMPE_E_CAP, who + ": too many blocks in one batch");
  RET(set_device(c0));
  // the scratch before any member's ordering state changes: pinned image (head, descriptors, result boxes) once,
  // device image + partials grown on demand (nothing of an earlier batch is pending: the call is blocking)
  constexpr size_t kDescOff = (sizeof(RoiBatch) + 255) / 256 * 256;
  constexpr size_t kBoxOff = kDescOff + kRoiMaxStreams * sizeof(RoiDesc);
  RET(c0->h_roim.ensure(c0, kBoxOff + kRoiMaxStreams * 4 * sizeof(double)));
  const size_t need = kBoxOff + (size_t)total * 4 * sizeof(double);
  RET(c0->d_roim.grow(c0, need, kBoxOff + (need - kBoxOff) * 2));
  unsigned char* hd_img = c0->h_roim.dev();
  // every member's work so far is ordered before the batch; a failure from here on gives the members their
  // ordering state back (the leader's own was set by set_device)
  OrderGuard members(ctxs, S);
  RET(members.order(1, c0->stream, c0));
  RoiBatch* hd = (RoiBatch*)c0->h_roim.get();
  RoiDesc* descs = (RoiDesc*)(c0->h_roim.get() + kDescOff);
  std::memset(hd, 0, sizeof(*hd));
  hd->S = S;
  int32_t nb = 0;
  for (int s = 0; s < S; ++s) {
    const pfmpe_ctx* c = ctxs[s];
    RoiDesc& d = descs[s];
    d.a = roi_args(c, &in[s]);
    d.prior = c->d_state[c->prior_idx].get();
    hd->first[s] = nb;
    nb += (c->N + kBlock - 1) / kBlock;
  }
  hd->first[S] = nb;
  const int stage_words = (int)((kDescOff + (size_t)S * sizeof(RoiDesc)) / sizeof(uint64_t));
  const RoiBatch* dhd = (const RoiBatch*)c0->d_roim.get();
  const RoiDesc* ddescs = (const RoiDesc*)(c0->d_roim.get() + kDescOff);
  double* part = (double*)(c0->d_roim.get() + kBoxOff);
  const double* hbox = (const double*)(c0->h_roim.get() + kBoxOff);
  double* dbox = (double*)(hd_img + kBoxOff);
  c0->timing_now = c0->timing > 0;
  int rc = launch(c0, PFMPE_K_ROI, [&] {
    hipLaunchKernelGGL((k_roi_stage<uint64_t>), dim3(1), dim3(kBlock), 0, c0->stream, (const uint64_t*)hd_img,
                       (uint64_t*)c0->d_roim.get(), stage_words);
    visit_state(c0, [&](auto s) {
      hipLaunchKernelGGL((k_roi_multi<typename decltype(s)::T, typename decltype(s)::SP>), dim3(nb), dim3(kBlock), 0,
                         c0->stream, dhd, ddescs, part);
    });
    hipLaunchKernelGGL((k_roi_multi_final<double>), dim3(S), dim3(kBlock), 0, c0->stream, dhd, (const double*)part,
                       dbox);
  });
  c0->timing_now = false;
  if (rc == PFMPE_OK && hipStreamSynchronize(c0->stream) != hipSuccess)
    rc = fail(c0, PFMPE_E_HIP, who + ": stream synchronise failed");
  if (rc == PFMPE_OK) rc = harvest_timing(c0);
  RET(rc);
  members.commit();  // nothing of the batch is pending: no member needs a fence
  for (int s = 0; s < S; ++s) {
    double bb[4];
    std::memcpy(bb, hbox + 4 * (size_t)s, sizeof(bb));
    roi_epilogue(ctxs[s]->K, ctxs[s]->markers, ctxs[s]->M, &in[s], bb, &out[s]);
  }
  return PFMPE_OK;
}
}  // namespace

int pfmpe_predict_roi(pfmpe_ctx* c, const pfmpe_roi_in* in, pfmpe_roi_out* out) {
  if (!c) return PFMPE_E_ARG;
  if (!in || !out) return fail(c, PFMPE_E_ARG, "predict_roi: null in/out");
  RET(roi_check_stream(c, c, in, "predict_roi: "));
  return roi_run(&c, 1, in, out, "predict_roi");
}

int pfmpe_predict_roi_multi(pfmpe_ctx* const* ctxs, int S, const pfmpe_roi_in* in, pfmpe_roi_out* out) {
  if (!ctxs || S < 1 || !ctxs[0]) return PFMPE_E_ARG;
  pfmpe_ctx* c0 = ctxs[0];
  if (!in || !out) return fail(c0, PFMPE_E_ARG, "predict_roi_multi: null in/out");
  if (S > PFMPE_ROI_MAX_STREAMS)
    return fail(c0, PFMPE_E_CAP, "predict_roi_multi: S exceeds PFMPE_ROI_MAX_STREAMS");
  RET(check_members(
      ctxs, S, "predict_roi_multi", "device and state type", [](const pfmpe_ctx*) { return true; },
      [&](int s, const std::string& at) { return roi_check_stream(c0, ctxs[s], &in[s], at); }));
  return roi_run(ctxs, S, in, out, "predict_roi_multi");
}

int pfmpe_host_predict_roi(const double* markers_xyz, int M, const double* K, const double* poses, int64_t N,
                           const pfmpe_roi_in* in, pfmpe_roi_out* out) {
  if (!markers_xyz || !K || !in || !out || M < 1 || M > PFMPE_MAX_MARKERS || N < 0 || (N > 0 && !poses) ||
      in->image_w < 1 || in->image_h < 1)
    return PFMPE_E_ARG;
  RoiArgs ra{};
  std::memcpy(ra.cam, in->cam_move_inv, sizeof(ra.cam));
  std::memcpy(ra.predm, in->prediction, sizeof(ra.predm));
  std::memcpy(ra.K, K, sizeof(ra.K));
  std::memcpy(ra.markers, markers_xyz, (size_t)M * 3 * sizeof(double));
  ra.N = 1;  // each pose row is a one-particle set: 12 planes of one element
  ra.M = M;
  ra.ld = 1;
  double bb[4] = {INFINITY, 0.0, INFINITY, 0.0};
  for (int64_t n = 0; n < N; ++n) roi_particle_box<double, double>(ra, poses + 12 * n, 0, bb[0], bb[1], bb[2], bb[3]);
  roi_epilogue(ra.K, ra.markers, M, in, bb, out);
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

namespace {
// exponentialMap (PE:2194-2226): twist [upsilon; omega] -> pose
void host_exp_map(const double* xi, double* pose) {
  const double* u = xi;
  const double* w = xi + 3;
  const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), th2 = th * th;
  const double O[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  double O2[9], R[9], V[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) O2[i * 3 + j] = O[i * 3] * O[j] + O[i * 3 + 1] * O[3 + j] + O[i * 3 + 2] * O[6 + j];
  for (int i = 0; i < 9; ++i) {
    const double I = (i % 4 == 0) ? 1.0 : 0.0;
    R[i] = I;
    V[i] = I;
    if (th != 0) {
      const double s = std::sin(th), c = std::cos(th);
      R[i] = I + O[i] / th * s + O2[i] / th2 * (1 - c);
      V[i] = I + (1 - c) / th2 * O[i] + (th - s) / (th2 * th) * O2[i];
    }
  }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) pose[i * 4 + j] = R[i * 3 + j];
    pose[i * 4 + 3] = V[i * 3] * u[0] + V[i * 3 + 1] * u[1] + V[i * 3 + 2] * u[2];
  }
}
// the kernel arguments of one statistics request on context c: its kept propagated set regenerated into d_xfer with
// the kept iteration's raw weights (WEIGHTED), or its current prior (POSTERIOR)
CloudArgs cloud_args(const pfmpe_ctx* c, int which, const double* ref) {
  CloudArgs ca{};
  std::memcpy(ca.ref, ref, sizeof(ca.ref));
  ca.N = c->N;
  if (which == PFMPE_CLOUD_WEIGHTED) {
    ca.dense = c->d_xfer.get();
    ca.w = c->d_w[c->last_kept_slot].get();
  } else {
    std::memcpy(ca.anchor, c->anchor[c->prior_idx], sizeof(ca.anchor));
    ca.ld = c->ld;
    ca.owner = prior_owner_ptr(c);
  }
  return ca;
}
// the kCloudWords reduced words r of a set of N particles about ref -> pfmpe_cloud_out (pfmpe_cloud_stats and every
// entry of pfmpe_cloud_stats_multi)
void cloud_epilogue(const double* r, int N, const double* ref, pfmpe_cloud_out* out) {
  std::memset(out, 0, sizeof(*out));
  out->n = N;
  out->wsum = r[0];
  if (!(r[0] > 0.0)) {  // all weights zero (the re-initialisation branch): no mean to speak of
    out->degenerate = 1;
    std::memcpy(out->mean_pose, ref, sizeof(out->mean_pose));
    return;
  }
  const double W = r[0];
  out->ess = W * W / r[1];
  for (int q = 0; q < 6; ++q) out->mean_twist[q] = r[2 + q] / W;
  int k = 8;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j, ++k) {
      const double v = r[k] / W - out->mean_twist[i] * out->mean_twist[j];
      out->cov[i * 6 + j] = v;
      out->cov[j * 6 + i] = v;
    }
  out->max_trans = std::sqrt(r[kCloudSums]);
  out->max_rot = std::sqrt(r[kCloudSums + 1]);
  // mean_pose = exp(mu) * ref: one step toward the intrinsic mean
  double E[12];
  host_exp_map(out->mean_twist, E);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      out->mean_pose[i * 4 + j] = E[i * 4] * ref[j] + E[i * 4 + 1] * ref[4 + j] + E[i * 4 + 2] * ref[8 + j];
    out->mean_pose[i * 4 + 3] = E[i * 4] * ref[3] + E[i * 4 + 1] * ref[7] + E[i * 4 + 2] * ref[11] + E[i * 4 + 3];
  }
}
}  // namespace

int pfmpe_host_cloud_plan(const int32_t* N, int S, pfmpe_cloud_plan* plan, int32_t* total_blocks) {
  if (!N || !plan || !total_blocks || S < 1) return PFMPE_E_ARG;
  if (S > PFMPE_CLOUD_MAX_STREAMS) return PFMPE_E_CAP;
  for (int s = 0; s < S; ++s)
    if (N[s] < 1) return PFMPE_E_ARG;
  int32_t nb = 0;  // at most 64 x 1024
  for (int s = 0; s < S; ++s) {
    plan[s].first_block = nb;
    // (cloud_blocks rounds N up in int: any N, not a context's only, comes through here)
    plan[s].blocks = N[s] >= kCloudMaxBlocks * kBlock ? kCloudMaxBlocks : cloud_blocks(N[s]);
    nb += plan[s].blocks;
  }
  *total_blocks = nb;
  return PFMPE_OK;
}

namespace {
// pfmpe_cloud_modes' batch: its S = K + 1 entries are one set of one context, entry s < K about seed s and restricted
// to mode s, entry K about seed 0 and restricted to the particles without a mode.
struct CloudModesRun {
  ModeSeeds seeds;
  uint8_t* mode_of;  // the caller's N bytes, or null
};
constexpr size_t kModesCountBytes = 256;  // the K + 1 member counts in front of pfmpe_ctx::d_modes' bytes
static_assert((kModesMax + 1) * sizeof(uint32_t) <= kModesCountBytes && PFMPE_MODES_MAX == kModesMax &&
                  PFMPE_MODE_NONE == kModeNone && kModesMax + 1 <= kCloudMaxStreams,
              "the modes of a call are one batch");
// The statistics of S checked entries, 1 <= S <= kCloudMaxStreams, on ctxs[0]'s stream: pfmpe_cloud_stats_multi, as a
// batch of one pfmpe_cloud_stats and, with `modes`, pfmpe_cloud_modes (the assignment runs between the regeneration
// and the reduction, and every entry reduces its mode's members: the same launches otherwise).  The errors it can
// raise itself begin with `who`.
int cloud_run(pfmpe_ctx* const* ctxs, int S, const pfmpe_cloud_in* in, pfmpe_cloud_out* out, const std::string& who,
              const CloudModesRun* modes = nullptr) {
  pfmpe_ctx* c0 = ctxs[0];
  // the distinct contexts in order of first appearance (ctxs[0] first), and which of them have a WEIGHTED entry
  std::vector<pfmpe_ctx*> distinct;
  std::vector<char> weighted;
  int32_t Ns[PFMPE_CLOUD_MAX_STREAMS];
  for (int s = 0; s < S; ++s) {
    pfmpe_ctx* c = ctxs[s];
    size_t m = 0;
    while (m < distinct.size() && distinct[m] != c) ++m;
    if (m == distinct.size()) {
      distinct.push_back(c);
      weighted.push_back(0);
    }
    if (in[s].which == PFMPE_CLOUD_WEIGHTED) weighted[m] = 1;
    Ns[s] = c->N;
  }
  pfmpe_cloud_plan plan[PFMPE_CLOUD_MAX_STREAMS];
  int32_t total = 0;
  if (pfmpe_host_cloud_plan(Ns, S, plan, &total) != PFMPE_OK)
    return fail(c0, PFMPE_E_STATE, who + ": a context without particles");
  RET(set_device(c0));
  // the scratch before any member's ordering state changes: pinned image (head, descriptors, result rows) once,
  // device image + partial rows grown on demand (nothing of an earlier batch is pending: the call is blocking)
  constexpr size_t kDescOff = (sizeof(CloudBatch) + 255) / 256 * 256;
  constexpr size_t kRowOff = (kDescOff + kCloudMaxStreams * sizeof(CloudDesc) + 255) / 256 * 256;
  constexpr size_t kRowBytes = kCloudWords * sizeof(double);
  RET(c0->h_cloudm.ensure(c0, kRowOff + kCloudMaxStreams * kRowBytes));
  const size_t need = kRowOff + (size_t)total * kRowBytes;
  RET(c0->d_cloudm.grow(c0, need, kRowOff + (need - kRowOff) * 2));
  if (modes) {
    RET(c0->h_modes.ensure(c0, kModesCountBytes));
    const size_t bytes = kModesCountBytes + (((size_t)c0->N + 3) & ~(size_t)3);
    RET(c0->d_modes.grow(c0, bytes, bytes));
  }
  for (size_t m = 0; m < distinct.size(); ++m)
    if (weighted[m]) RET(ensure_xfer(distinct[m]));
  // each WEIGHTED context's kept propagated set once, as its single call regenerates it: into its own d_xfer, on its
  // own stream (set_device: after whatever it has pending elsewhere); all its entries read that set
  for (size_t m = 0; m < distinct.size(); ++m) {
    pfmpe_ctx* c = distinct[m];
    if (!weighted[m]) continue;
    if (c != c0) RET(set_device(c));
    if (const int r_ = dispatch_regen(c, c->last_kept_iter, c->d_state[c->last_prior_idx].get(), c->d_xfer.get()))
      return c == c0 ? r_ : fail(c0, r_, who + ": " + c->err);
  }
  // every member's work so far, that regeneration included, is ordered before the batch (a context that appears
  // twice once); a failure from here on gives the members their ordering state back (the leader's own was set by
  // set_device)
  OrderGuard members(distinct.data(), (int)distinct.size());
  RET(members.order(1, c0->stream, c0));
  unsigned char* hd_img = c0->h_cloudm.dev();
  CloudBatch* hd = (CloudBatch*)c0->h_cloudm.get();
  CloudDesc* descs = (CloudDesc*)(c0->h_cloudm.get() + kDescOff);
  std::memset(hd, 0, sizeof(*hd));
  hd->S = S;
  for (int s = 0; s < S; ++s) {
    const pfmpe_ctx* c = ctxs[s];
    CloudDesc& d = descs[s];
    d.a = cloud_args(c, in[s].which, in[s].ref_pose);
    d.dense = in[s].which == PFMPE_CLOUD_WEIGHTED;
    d.st = d.dense ? nullptr : c->d_state[c->prior_idx].get();
    d.mode_of = modes ? c0->d_modes.get() + kModesCountBytes : nullptr;
    d.mode = s < S - 1 ? s : kModeNone;  // (read by a filtered entry only)
    hd->first[s] = plan[s].first_block;
  }
  hd->first[S] = total;
  const int stage_words = (int)((kDescOff + (size_t)S * sizeof(CloudDesc)) / sizeof(uint64_t));
  const CloudBatch* dhd = (const CloudBatch*)c0->d_cloudm.get();
  const CloudDesc* ddescs = (const CloudDesc*)(c0->d_cloudm.get() + kDescOff);
  double* part = (double*)(c0->d_cloudm.get() + kRowOff);
  const double* hrow = (const double*)(c0->h_cloudm.get() + kRowOff);
  hipLaunchKernelGGL((k_roi_stage<uint64_t>), dim3(1), dim3(kBlock), 0, c0->stream, (const uint64_t*)hd_img,
                     (uint64_t*)c0->d_cloudm.get(), stage_words);
  uint32_t* d_count = (uint32_t*)c0->d_modes.get();
  if (modes) {  // every entry reads the same set: entry 0's descriptor names it
    HIPCHK(c0, hipMemsetAsync(d_count, 0, kModesCountBytes, c0->stream));
    visit_state(c0, [&](auto s) {
      hipLaunchKernelGGL((k_cloud_assign<typename decltype(s)::T, typename decltype(s)::SP>), dim3(cloud_blocks(c0->N)),
                         dim3(kBlock), 0, c0->stream, descs[0], modes->seeds, c0->d_modes.get() + kModesCountBytes,
                         d_count);
    });
  }
  visit_state(c0, [&](auto s) {
    using T = typename decltype(s)::T;
    using SP = typename decltype(s)::SP;
    if (modes)
      hipLaunchKernelGGL((k_cloud_multi<T, SP, true>), dim3(total), dim3(kBlock), 0, c0->stream, dhd, ddescs, part);
    else
      hipLaunchKernelGGL((k_cloud_multi<T, SP, false>), dim3(total), dim3(kBlock), 0, c0->stream, dhd, ddescs, part);
  });
  hipLaunchKernelGGL(k_cloud_multi_final, dim3(S), dim3(kCloudSegs * kCloudWords), 0, c0->stream, dhd,
                     (const double*)part, (double*)(hd_img + kRowOff));
  HIPCHK(c0, hipGetLastError());
  if (modes) {
    HIPCHK(c0, hipMemcpyAsync(c0->h_modes.get(), d_count, (size_t)S * sizeof(uint32_t), hipMemcpyDeviceToHost, c0->stream));
    if (modes->mode_of)
      HIPCHK(c0, hipMemcpyAsync(modes->mode_of, c0->d_modes.get() + kModesCountBytes, (size_t)c0->N,
                                hipMemcpyDeviceToHost, c0->stream));
  }
  if (hipStreamSynchronize(c0->stream) != hipSuccess)
    return fail(c0, PFMPE_E_HIP, who + ": stream synchronise failed");
  members.commit();  // nothing of the batch is pending: no member needs a fence
  for (pfmpe_ctx* c : distinct)  // (as every single call ends: the brackets of sampled frames still pending)
    if (const int r_ = harvest_timing(c)) return c == c0 ? r_ : fail(c0, r_, who + ": " + c->err);
  for (int s = 0; s < S; ++s) {
    double r[kCloudWords];
    std::memcpy(r, hrow + (size_t)kCloudWords * s, sizeof(r));
    const int64_t n = modes ? (int64_t)((const uint32_t*)c0->h_modes.get())[s] : (int64_t)ctxs[s]->N;
    cloud_epilogue(r, n, in[s].ref_pose, &out[s]);
  }
  return PFMPE_OK;
}
// the checks pfmpe_cloud_modes and pfmpe_host_cloud_assign share: K, the seeds, the parameters
const char* modes_args_bad(const double* seeds, int K, const pfmpe_modes_params& p) {
  if (K < 1 || K > PFMPE_MODES_MAX) return "K outside 1..PFMPE_MODES_MAX";
  for (int q = 0; q < 12 * K; ++q)
    if (!std::isfinite(seeds[q])) return "non-finite seed";
  for (const double v : {p.trans_scale, p.rot_scale, p.max_dist})
    if (!(v >= 0.0) || !std::isfinite(v)) return "a scale or max_dist is negative or not finite";
  if (p.trans_scale == 0.0 && p.rot_scale == 0.0) return "both scales are 0";
  return nullptr;
}
ModeSeeds mode_seeds(const double* seeds, int K, const pfmpe_modes_params& p) {
  ModeSeeds ms{};
  std::memcpy(ms.seed, seeds, (size_t)K * 12 * sizeof(double));
  ms.it2 = mode_inv2(p.trans_scale);
  ms.ir2 = mode_inv2(p.rot_scale);
  ms.max_dist = p.max_dist;
  ms.K = K;
  return ms;
}
}  // namespace

void pfmpe_default_modes_params(pfmpe_modes_params* p) {
  if (!p) return;
  p->trans_scale = 0.01;
  p->rot_scale = 0.05;
  p->max_dist = 0.0;
}

int pfmpe_cloud_modes(pfmpe_ctx* c, int which, const double* seeds, int K, const pfmpe_modes_params* params,
                      pfmpe_mode_out* out, uint8_t* mode_of) {
  static_assert(sizeof(pfmpe_modes_params) == 24 && sizeof(pfmpe_mode_out) == 488, "ABI");
  if (!c) return PFMPE_E_ARG;
  if (!seeds || !out || (which != PFMPE_CLOUD_WEIGHTED && which != PFMPE_CLOUD_POSTERIOR))
    return fail(c, PFMPE_E_ARG, "cloud_modes: bad arguments");
  pfmpe_modes_params prm;
  pfmpe_default_modes_params(&prm);
  if (params) prm = *params;
  if (const char* bad = modes_args_bad(seeds, K, prm)) return fail(c, PFMPE_E_ARG, std::string("cloud_modes: ") + bad);
  if (!c->has_prior) return fail(c, PFMPE_E_STATE, "cloud_modes: no particle set");
  if (which == PFMPE_CLOUD_WEIGHTED && !c->has_last) return fail(c, PFMPE_E_STATE, "cloud_modes(weighted): no step yet");
  CloudModesRun run{mode_seeds(seeds, K, prm), mode_of};
  pfmpe_ctx* ctxs[kModesMax + 1];
  pfmpe_cloud_in in[kModesMax + 1];
  pfmpe_cloud_out stats[kModesMax + 1];
  for (int s = 0; s <= K; ++s) {
    ctxs[s] = c;
    in[s] = pfmpe_cloud_in{};
    std::memcpy(in[s].ref_pose, seeds + 12 * (s < K ? s : 0), sizeof(in[s].ref_pose));
    in[s].which = which;
  }
  RET(cloud_run(ctxs, K + 1, in, stats, "cloud_modes", &run));
  double total = 0.0;
  for (int s = 0; s <= K; ++s) total = total + stats[s].wsum;
  for (int s = 0; s <= K; ++s) {
    out[s].stats = stats[s];
    out[s].share = total > 0.0 ? stats[s].wsum / total : 0.0;
  }
  return PFMPE_OK;
}

int pfmpe_host_cloud_assign(const double* poses, int64_t N, const double* seeds, int K, const pfmpe_modes_params* params,
                            uint8_t* mode_of, int64_t* counts) {
  if (!seeds || N < 0 || (N > 0 && (!poses || !mode_of))) return PFMPE_E_ARG;
  pfmpe_modes_params prm;
  pfmpe_default_modes_params(&prm);
  if (params) prm = *params;
  if (modes_args_bad(seeds, K, prm)) return PFMPE_E_ARG;
  const ModeSeeds ms = mode_seeds(seeds, K, prm);
  int64_t cnt[kModesMax + 1] = {0};
  for (int64_t n = 0; n < N; ++n) {
    const int mode = mode_assign(poses + 12 * n, ms);
    mode_of[n] = (uint8_t)mode;
    cnt[mode == kModeNone ? K : mode] += 1;
  }
  if (counts) std::memcpy(counts, cnt, (size_t)(K + 1) * sizeof(int64_t));
  return PFMPE_OK;
}

int pfmpe_cloud_stats(pfmpe_ctx* c, int which, const double* ref, pfmpe_cloud_out* out) {
  if (!c) return PFMPE_E_ARG;
  if (!ref || !out || (which != PFMPE_CLOUD_WEIGHTED && which != PFMPE_CLOUD_POSTERIOR))
    return fail(c, PFMPE_E_ARG, "cloud_stats: bad arguments");
  for (int q = 0; q < 12; ++q)
    if (!std::isfinite(ref[q])) return fail(c, PFMPE_E_ARG, "cloud_stats: non-finite reference pose");
  if (!c->has_prior) return fail(c, PFMPE_E_STATE, "cloud_stats: no particle set");
  if (which == PFMPE_CLOUD_WEIGHTED && !c->has_last) return fail(c, PFMPE_E_STATE, "cloud_stats(weighted): no step yet");
  pfmpe_cloud_in e{};
  std::memcpy(e.ref_pose, ref, sizeof(e.ref_pose));
  e.which = which;
  return cloud_run(&c, 1, &e, out, "cloud_stats");
}

int pfmpe_cloud_stats_multi(pfmpe_ctx* const* ctxs, int S, const pfmpe_cloud_in* in, pfmpe_cloud_out* out) {
  static_assert(PFMPE_CLOUD_MAX_STREAMS == kCloudMaxStreams, "stream capacity mismatch");
  if (!ctxs || S < 1 || !ctxs[0]) return PFMPE_E_ARG;
  pfmpe_ctx* c0 = ctxs[0];
  if (!in || !out) return fail(c0, PFMPE_E_ARG, "cloud_stats_multi: null in/out");
  if (S > PFMPE_CLOUD_MAX_STREAMS)
    return fail(c0, PFMPE_E_CAP, "cloud_stats_multi: S exceeds PFMPE_CLOUD_MAX_STREAMS");
  for (int s = 0; s < S; ++s) {
    const pfmpe_ctx* c = ctxs[s];
    const std::string at = "cloud_stats_multi: stream " + std::to_string(s) + ": ";
    if (!c) return fail(c0, PFMPE_E_ARG, at + "null context");
    if (c->device != c0->device || c->state_dtype != c0->state_dtype)
      return fail(c0, PFMPE_E_ARG, at + "device and state type must match ctxs[0]");
    const int which = in[s].which;
    if (which != PFMPE_CLOUD_WEIGHTED && which != PFMPE_CLOUD_POSTERIOR) return fail(c0, PFMPE_E_ARG, at + "bad which");
    for (int q = 0; q < 12; ++q)
      if (!std::isfinite(in[s].ref_pose[q])) return fail(c0, PFMPE_E_ARG, at + "non-finite reference pose");
    if (!c->has_prior) return fail(c0, PFMPE_E_STATE, at + "no particle set");
    if (which == PFMPE_CLOUD_WEIGHTED && !c->has_last) return fail(c0, PFMPE_E_STATE, at + "weighted: no step yet");
  }
  return cloud_run(ctxs, S, in, out, "cloud_stats_multi");
}
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

namespace {
// The argument and state checks shared by pfmpe_assoc_stats / pfmpe_get_pairs, then the call's blob table built
// into d_table (every frame that reads d_table writes it first) and, for the propagated set, the kept set
// regenerated into d_xfer (written and read inside one blocking call by every user).  *blobs_out / *B_out: the
// blobs the call means (resolve_blobs).
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
// the largest table build_table can write for B blobs of this context's type (the finest grid B may get, full lists)
size_t assoc_table_bound(const pfmpe_ctx* c, int B) {
  return visit_state(c, [&](auto s) {
    return BlobTable<typename decltype(s)::T>::total_bytes(B, B >= kGridFineMinBlobs ? kGridMaxCells : kGridCoarseCells,
                                                           kGridMaxEntries);
  });
}
}  // namespace

int pfmpe_assoc_stats(pfmpe_ctx* c, int which, const pfmpe_assoc_in* in, pfmpe_assoc_out* out, uint32_t* votes) {
  if (!c) return PFMPE_E_ARG;
  if (!out) return fail(c, PFMPE_E_ARG, "assoc_stats: null out");
  const double* blobs = nullptr;
  int B = 0;
  size_t tbytes = 0;
  GridHdr gh{};
  AssocArgs aa{};
  RET(assoc_prepare(c, "assoc_stats", which, in, &blobs, &B, &tbytes, &gh, &aa));
  // scratch of the call's own: the bins of the largest table
  RET(c->d_assoc.ensure(c, (size_t)assoc_bins(kMaxMarkers, kMaxBlobs) * sizeof(uint32_t)));
  const int M = c->M, N = c->N;
  const int nbins = assoc_bins(M, B);
  HIPCHK(c, hipMemsetAsync(c->d_assoc.get(), 0, (size_t)nbins * sizeof(uint32_t), c->stream));
  aa.votes = c->d_assoc.get();
  aa.first = 0;
  aa.count = N;
  RET(assoc_launch(c, B, c->d_table.get(), tbytes, gh, aa));
  std::vector<uint32_t> bins(nbins);
  HIPCHK(c, hipMemcpyAsync(bins.data(), c->d_assoc.get(), (size_t)nbins * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  RET(harvest_timing(c));  // (a propagated call's regeneration is bracketed like the particle read-back's)
  if (!assoc_epilogue(bins.data(), M, B, N, out, votes))
    return fail(c, PFMPE_E_STATE, "assoc_stats: inconsistent votes table");
  return PFMPE_OK;
}

int pfmpe_assoc_stats_multi(pfmpe_ctx* const* ctxs, int S, const pfmpe_assoc_multi_in* in, pfmpe_assoc_out* out,
                            uint32_t* const* votes) {
  static_assert(sizeof(pfmpe_assoc_multi_in) == 24 && sizeof(pfmpe_assoc_plan) == 24 && sizeof(pfmpe_assoc_plan_total) == 80,
                "ABI");
  if (!ctxs || S < 1 || !ctxs[0]) return PFMPE_E_ARG;
  pfmpe_ctx* c0 = ctxs[0];
  if (!in || !out) return fail(c0, PFMPE_E_ARG, "assoc_stats_multi: null in/out");
  if (S > PFMPE_ASSOC_MAX_STREAMS) return fail(c0, PFMPE_E_CAP, "assoc_stats_multi: S exceeds PFMPE_ASSOC_MAX_STREAMS");
  // ---- every check, on host data alone
  AssocMultiEntry e[PFMPE_ASSOC_MAX_STREAMS];
  const double* blobs[PFMPE_ASSOC_MAX_STREAMS];
  for (int s = 0; s < S; ++s) {
    pfmpe_ctx* c = ctxs[s];
    const std::string at = "assoc_stats_multi: stream " + std::to_string(s) + ": ";
    if (!c) return fail(c0, PFMPE_E_ARG, at + "null context");
    if (c->device != c0->device || c->state_dtype != c0->state_dtype)
      return fail(c0, PFMPE_E_ARG, at + "device and state type must match ctxs[0]");
    const int which = in[s].which;
    if (which != PFMPE_ASSOC_PROPAGATED && which != PFMPE_ASSOC_POSTERIOR) return fail(c0, PFMPE_E_ARG, at + "bad which");
    int B = 0;
    RET(resolve_blobs(c, at.substr(0, at.size() - 2), &in[s].blobs, &blobs[s], &B, c0));
    if (!c->has_model || !c->has_prior) return fail(c0, PFMPE_E_STATE, at + "set_model and a particle set first");
    if (which == PFMPE_ASSOC_PROPAGATED && !c->has_last) return fail(c0, PFMPE_E_STATE, at + "propagated: no step yet");
    e[s] = AssocMultiEntry{};
    e[s].c = c;
    e[s].which = which;
    e[s].B = B;
  }
  // the distinct contexts in order of first appearance (ctxs[0] first), and which of them have a PROPAGATED entry
  std::vector<pfmpe_ctx*> distinct;
  std::vector<char> regen;
  for (int s = 0; s < S; ++s) {
    size_t m = 0;
    while (m < distinct.size() && distinct[m] != ctxs[s]) ++m;
    if (m == distinct.size()) {
      distinct.push_back(ctxs[s]);
      regen.push_back(0);
    }
    if (e[s].which == PFMPE_ASSOC_PROPAGATED) regen[m] = 1;
  }
  RET(set_device(c0));
  // ---- the image: every entry's table, built in the leader's pinned block behind the heads and descriptors (host
  // work: nothing is on the device yet).  The block holds the largest table each entry can get.
  const size_t tables_off = assoc_multi_tables_off(c0, S);
  size_t cap = tables_off;
  for (int s = 0; s < S; ++s) cap += align16(assoc_table_bound(c0, e[s].B));
  {
    size_t bins_bound = 0;  // the batch's bins, each entry's start rounded up to 4 words
    for (int s = 0; s < S; ++s) bins_bound += (((size_t)assoc_bins(e[s].c->M, e[s].B) + 3) & ~(size_t)3) * sizeof(uint32_t);
    const size_t need = (cap + 255) / 256 * 256 + bins_bound;
    RET(c0->h_assocm.grow(c0, need, need * 2));
  }
  unsigned char* himg = c0->h_assocm.get();
  int32_t Ns[PFMPE_ASSOC_MAX_STREAMS], Ms[PFMPE_ASSOC_MAX_STREAMS], Bs[PFMPE_ASSOC_MAX_STREAMS], Ws[PFMPE_ASSOC_MAX_STREAMS],
      Ps[PFMPE_ASSOC_MAX_STREAMS], Ts[PFMPE_ASSOC_MAX_STREAMS];
  size_t img_bytes = tables_off;
  for (int s = 0; s < S; ++s) {
    const pfmpe_ctx* c = e[s].c;
    e[s].table_off = img_bytes;
    e[s].tbytes = build_table(c, blobs[s], e[s].B, himg + img_bytes);
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
  int bad = 0;  // (S, the counts and B were checked above: what is left is a table that exceeds the LDS)
  if (const int r_ = assoc_plan(Ns, Ms, Bs, Ws, Ps, Ts, S, c0->state_dtype, plan, &total, &bad))
    return fail(c0, r_, "assoc_stats_multi: stream " + std::to_string(bad) + ": blob table exceeds the LDS");
  for (int s = 0; s < S; ++s) {
    e[s].bins_off = plan[s].bins_offset;
    e[s].launch = plan[s].launch;
    e[s].first_block = plan[s].first_block;
    e[s].blocks = plan[s].blocks;
    e[s].lds_votes = (plan[s].lds_votes && !(e[s].c->diag & kDiagAssocDirect)) ? 1 : 0;
  }
  // the device scratch: the image, then the bins (nothing of an earlier batch is pending: the call is blocking)
  const size_t bins_at = (img_bytes + 255) / 256 * 256;
  const size_t bins_bytes = (size_t)total.bins_words * sizeof(uint32_t);
  RET(c0->d_assocm.grow(c0, bins_at + bins_bytes, (bins_at + bins_bytes) * 2));
  for (size_t m = 0; m < distinct.size(); ++m)
    if (regen[m]) RET(ensure_xfer(distinct[m]));
  // each PROPAGATED context's kept propagated set once, as its single call regenerates it: into its own d_xfer, on its
  // own stream (set_device: after whatever it has pending elsewhere); all its entries read that set
  for (size_t m = 0; m < distinct.size(); ++m) {
    pfmpe_ctx* c = distinct[m];
    if (!regen[m]) continue;
    if (c != c0) RET(set_device(c));
    if (const int r_ = dispatch_regen(c, c->last_kept_iter, c->d_state[c->last_prior_idx].get(), c->d_xfer.get()))
      return c == c0 ? r_ : fail(c0, r_, "assoc_stats_multi: " + c->err);
  }
  // every member's work so far, that regeneration included, is ordered before the batch; a failure from here on gives
  // the members their ordering state back (the leader's own was set by set_device)
  OrderGuard members(distinct.data(), (int)distinct.size());
  RET(members.order(1, c0->stream, c0));
  uint32_t* dbins = (uint32_t*)(c0->d_assocm.get() + bins_at);
  RET(assoc_multi_run(c0, e, S, total.launches, himg, c0->d_assocm.get(), img_bytes, dbins, (size_t)total.bins_words));
  const uint32_t* hbins = (const uint32_t*)(himg + bins_at);
  HIPCHK(c0, hipMemcpyAsync((void*)hbins, dbins, bins_bytes, hipMemcpyDeviceToHost, c0->stream));
  if (hipStreamSynchronize(c0->stream) != hipSuccess)
    return fail(c0, PFMPE_E_HIP, "assoc_stats_multi: stream synchronise failed");
  members.commit();  // nothing of the batch is pending: no member needs a fence
  for (pfmpe_ctx* c : distinct)  // (as every single call ends: the brackets of sampled frames still pending)
    if (const int r_ = harvest_timing(c)) return c == c0 ? r_ : fail(c0, r_, "assoc_stats_multi: " + c->err);
  // the tables are checked before any output is written
  for (int s = 0; s < S; ++s) {
    pfmpe_assoc_out o;
    if (!assoc_epilogue(hbins + e[s].bins_off, e[s].c->M, e[s].B, e[s].c->N, &o, nullptr))
      return fail(c0, PFMPE_E_STATE, "assoc_stats_multi: stream " + std::to_string(s) + ": inconsistent votes table");
  }
  for (int s = 0; s < S; ++s)
    (void)assoc_epilogue(hbins + e[s].bins_off, e[s].c->M, e[s].B, e[s].c->N, &out[s], votes ? votes[s] : nullptr);
  return PFMPE_OK;
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
    RET(assoc_launch(c, B, c->d_table.get(), tbytes, gh, aa));
    HIPCHK(c, hipMemcpyAsync(corr + (size_t)done * kRow, aa.corr, (size_t)n * kRow * sizeof(uint32_t),
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(n_corr + done, aa.n_corr, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the chunk buffer is reused
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  RET(harvest_timing(c));
  return PFMPE_OK;
}

// ---- the K best distinct hypotheses of the kept propagated set (pf_top.hpp; the kernels are in pfmpe_top.hip)
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
    // rows mode over the dense list of the kept rows' poses (it bounds its range by first / count alone; count is
    // `rows`, the rows behind n_out hold a constant pose and are not returned)
    const size_t tbytes = build_table(c, blobs, B, c->h_table.get());
    const GridHdr gh = *(const GridHdr*)(c->h_table.get() + grid_off(c, B));
    HIPCHK(c, hipMemcpyAsync(c->d_table.get(), c->h_table.get(), tbytes, hipMemcpyHostToDevice, c->stream));
    AssocArgs aa{};
    aa.dense = (const double*)(rec + TopRows::poses(rows));
    aa.corr = (uint32_t*)(rec + TopRows::corr(rows));
    aa.n_corr = (int32_t*)(rec + TopRows::n_corr(rows));
    aa.first = 0;
    aa.count = rows;
    RET(assoc_launch(c, B, c->d_table.get(), tbytes, gh, aa));
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

// ---- Gauss-Newton refinement (optimisePose, PE:1805-2009): pf_gn.hpp on the host here, k_refine in pfmpe_refine.hip
void pfmpe_default_refine_params(pfmpe_refine_params* p) {
  if (!p) return;
  p->max_iter = 500;
  p->revert_on_divergence = 1;
  p->converged = 1e-13;
}

namespace {
bool refine_params_ok(const pfmpe_refine_params& p) {
  return p.max_iter >= 1 && p.max_iter <= 10000 && p.converged >= 0.0;  // (a NaN fails the comparison)
}
// the rows' indices: LED 1 .. M beside a blob, never above M; blob 0 .. B
bool refine_corr_ok(const uint32_t* corr, size_t n_rows, int M, int B) {
  for (size_t j = 0; j < n_rows; ++j) {
    const uint32_t led = corr[2 * j], blob = corr[2 * j + 1];
    if (led > (uint32_t)M || blob > (uint32_t)B || (blob != 0u && led == 0u)) return false;
  }
  return true;
}
bool refine_poses_finite(const double* poses, size_t n) {
  for (size_t q = 0; q < 12 * n; ++q)
    if (!std::isfinite(poses[q])) return false;
  return true;
}

// the scratch, the model and the call's blobs in fp64 (enqueued on the stream; `stage` must outlive the copy)
int refine_stage(pfmpe_ctx* c, const double* blobs, int B, int cap, std::vector<double>& stage) {
  RET(c->d_refine.ensure(c, RefineBuf::bytes(c->max_blobs, cap)));
  const size_t words = (RefineBuf::kBlobs - RefineBuf::kMarkers) / sizeof(double) + 2 * (size_t)B;
  stage.assign(words, 0.0);
  std::memcpy(stage.data(), c->markers, sizeof(c->markers));
  std::memcpy(stage.data() + (RefineBuf::kK - RefineBuf::kMarkers) / sizeof(double), c->K, sizeof(c->K));
  if (B > 0) std::memcpy(stage.data() + (RefineBuf::kBlobs - RefineBuf::kMarkers) / sizeof(double), blobs, 2 * (size_t)B * sizeof(double));
  HIPCHK(c, hipMemcpyAsync(c->d_refine.get() + RefineBuf::kMarkers, stage.data(), words * sizeof(double), hipMemcpyHostToDevice,
                           c->stream));
  return PFMPE_OK;
}
// a chunk's rows and covariances, hypotheses lo .. hi - 1 of the chunk, to the caller's arrays at index `at`
int refine_fetch(pfmpe_ctx* c, int cap, int lo, int hi, pfmpe_refine_row* rows, double* cov, int64_t at) {
  if (hi <= lo) return PFMPE_OK;
  const unsigned char* d = c->d_refine.get();
  if (rows)
    HIPCHK(c, hipMemcpyAsync(rows + at, d + RefineBuf::rows(c->max_blobs) + (size_t)lo * sizeof(pfmpe_refine_row),
                             (size_t)(hi - lo) * sizeof(pfmpe_refine_row), hipMemcpyDeviceToHost, c->stream));
  if (cov)
    HIPCHK(c, hipMemcpyAsync(cov + 36 * at, d + RefineBuf::cov(c->max_blobs, cap) + (size_t)lo * 36 * sizeof(double),
                             (size_t)(hi - lo) * 36 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  return PFMPE_OK;
}
int refine_finish(pfmpe_ctx* c, int64_t n, pfmpe_refine_out* out) {
  HIPCHK(c, hipMemcpyAsync(out, c->d_refine.get() + RefineBuf::kOut, sizeof(*out), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  RET(harvest_timing(c));  // (a propagated call's regeneration is bracketed like the particle read-back's)
  out->n = n;
  return PFMPE_OK;
}
}  // namespace

int pfmpe_refine_poses(pfmpe_ctx* c, const pfmpe_assoc_in* in, const pfmpe_refine_params* params, const double* poses,
                       const uint32_t* corr, int32_t K, pfmpe_refine_out* out, pfmpe_refine_row* rows, double* cov) {
  if (!c) return PFMPE_E_ARG;
  pfmpe_refine_params prm;
  pfmpe_default_refine_params(&prm);
  if (params) prm = *params;
  if (!out || !in || K < 0 || (K > 0 && (!poses || !corr))) return fail(c, PFMPE_E_ARG, "refine_poses: bad arguments");
  if (!refine_params_ok(prm)) return fail(c, PFMPE_E_ARG, "refine_poses: bad parameters");
  const double* blobs = nullptr;
  int B = 0;
  RET(resolve_blobs(c, "refine_poses", in, &blobs, &B));
  if (K > c->max_particles) return fail(c, PFMPE_E_CAP, "refine_poses: K exceeds max_particles");
  if (!c->has_model) return fail(c, PFMPE_E_STATE, "refine_poses: set_model first");
  if (K > 0 && !refine_corr_ok(corr, (size_t)K * kMaxMarkers, c->M, B))
    return fail(c, PFMPE_E_ARG, "refine_poses: LED or blob index out of range");
  if (K > 0 && !refine_poses_finite(poses, (size_t)K)) return fail(c, PFMPE_E_ARG, "refine_poses: non-finite start pose");
  RET(set_device(c));
  RET(ensure_xfer(c));
  constexpr size_t kRow = kPairRow;
  const int cap = pairs_cap(c);
  RET(ensure_pairs(c));
  std::vector<double> stage;
  RET(refine_stage(c, blobs, B, cap, stage));
  // d_xfer is written and read inside one blocking call by every user
  if (K > 0) HIPCHK(c, hipMemcpyAsync(c->d_xfer.get(), poses, (size_t)K * 12 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  int64_t done = 0;
  do {  // (K = 0: one empty chunk writes the empty summary)
    const int n = (int)std::min<int64_t>(cap, (int64_t)K - done);
    if (n > 0)
      HIPCHK(c, hipMemcpyAsync(c->d_pairs.get(), corr + (size_t)done * kRow, (size_t)n * kRow * sizeof(uint32_t),
                               hipMemcpyHostToDevice, c->stream));
    RET(refine_launch(c, prm, c->d_xfer.get() + 12 * done, c->d_pairs.get(), done, n, cap, done == 0));
    RET(refine_fetch(c, cap, 0, n, rows, cov, done));
    done += n;
  } while (done < K);
  return refine_finish(c, K, out);
}

int pfmpe_refine_cloud(pfmpe_ctx* c, int which, const pfmpe_assoc_in* in, const pfmpe_refine_params* params,
                       int64_t first, int32_t count, pfmpe_refine_out* out, pfmpe_refine_row* rows, double* cov) {
  if (!c) return PFMPE_E_ARG;
  pfmpe_refine_params prm;
  pfmpe_default_refine_params(&prm);
  if (params) prm = *params;
  if (!out || first < 0 || count < 0) return fail(c, PFMPE_E_ARG, "refine_cloud: null out or bad range");
  if (c->has_prior && first + (int64_t)count > (int64_t)c->N)
    return fail(c, PFMPE_E_ARG, "refine_cloud: first + count exceeds the particle count");
  if (!refine_params_ok(prm)) return fail(c, PFMPE_E_ARG, "refine_cloud: bad parameters");
  const double* blobs = nullptr;
  int B = 0;
  size_t tbytes = 0;
  GridHdr gh{};
  AssocArgs aa{};
  RET(assoc_prepare(c, "refine_cloud", which, in, &blobs, &B, &tbytes, &gh, &aa));
  const int N = c->N;
  // the start poses as get_particles delivers them: the propagated set is in d_xfer already (assoc_prepare)
  if (which == PFMPE_ASSOC_POSTERIOR) {
    RET(ensure_xfer(c));
    RET(export_prior(c, N));
  }
  constexpr size_t kRow = kPairRow;
  const int cap = pairs_cap(c);
  RET(ensure_pairs(c));
  std::vector<double> stage;
  RET(refine_stage(c, blobs, B, cap, stage));
  aa.corr = c->d_pairs.get();
  aa.n_corr = (int32_t*)(c->d_pairs.get() + (size_t)cap * kRow);
  for (int64_t done = 0; done < N; done += cap) {
    const int n = (int)std::min<int64_t>(cap, (int64_t)N - done);
    aa.first = (int32_t)done;
    aa.count = n;
    RET(assoc_launch(c, B, c->d_table.get(), tbytes, gh, aa));
    RET(refine_launch(c, prm, c->d_xfer.get() + 12 * done, c->d_pairs.get(), done, n, cap, done == 0));
    const int64_t lo = std::max<int64_t>(first, done), hi = std::min<int64_t>(first + count, done + n);
    RET(refine_fetch(c, cap, (int)(lo - done), (int)(hi - done), rows, cov, lo - first));
  }
  return refine_finish(c, N, out);
}

// pfmpe_refine_poses of S streams as one batch on ctxs[0]'s stream: the per-stream checks of the single call, the
// upload of pfmpe_refine_plan.hpp built in the leader's pinned block, one copy up, two launches, one copy down, one
// synchronise, and the results scattered to the caller's arrays.
int pfmpe_refine_multi(pfmpe_ctx* const* ctxs, int S, const pfmpe_refine_in* in, const pfmpe_refine_params* params,
                       pfmpe_refine_out* out, pfmpe_refine_row* const* rows, double* const* cov) {
  if (!ctxs || S < 1 || !ctxs[0]) return PFMPE_E_ARG;
  pfmpe_ctx* c0 = ctxs[0];
  if (!in || !out) return fail(c0, PFMPE_E_ARG, "refine_multi: null in/out");
  if (S > PFMPE_REFINE_MAX_STREAMS) return fail(c0, PFMPE_E_CAP, "refine_multi: S exceeds PFMPE_REFINE_MAX_STREAMS");
  struct Stream {
    const double* blobs;
    int B;
    pfmpe_refine_params prm;
  };
  std::vector<Stream> st(S);
  int32_t Ks[PFMPE_REFINE_MAX_STREAMS], Bs[PFMPE_REFINE_MAX_STREAMS];
  int64_t H = 0;
  for (int s = 0; s < S; ++s) {
    const pfmpe_ctx* c = ctxs[s];
    const pfmpe_refine_in& q = in[s];
    const std::string at = "refine_multi: stream " + std::to_string(s) + ": ";
    if (!c) return fail(c0, PFMPE_E_ARG, at + "null context");
    if (c->device != c0->device) return fail(c0, PFMPE_E_ARG, at + "device must match ctxs[0]");
    pfmpe_default_refine_params(&st[s].prm);
    if (params) st[s].prm = params[s];
    if (q.K < 0 || (q.K > 0 && (!q.poses || !q.corr))) return fail(c0, PFMPE_E_ARG, at + "bad arguments");
    if (!refine_params_ok(st[s].prm)) return fail(c0, PFMPE_E_ARG, at + "bad parameters");
    RET(resolve_blobs(c, at + "blobs", &q.blobs, &st[s].blobs, &st[s].B, c0));
    if (q.K > c->max_particles) return fail(c0, PFMPE_E_CAP, at + "K exceeds max_particles");
    if (!c->has_model) return fail(c0, PFMPE_E_STATE, at + "set_model first");
    if (q.K > 0 && !refine_corr_ok(q.corr, (size_t)q.K * kMaxMarkers, c->M, st[s].B))
      return fail(c0, PFMPE_E_ARG, at + "LED or blob index out of range");
    if (q.K > 0 && !refine_poses_finite(q.poses, (size_t)q.K)) return fail(c0, PFMPE_E_ARG, at + "non-finite start pose");
    Ks[s] = q.K;
    Bs[s] = st[s].B;
    H += q.K;
    if (H > PFMPE_REFINE_MULTI_MAX_HYPOTHESES)
      return fail(c0, PFMPE_E_CAP, at + "the batch exceeds PFMPE_REFINE_MULTI_MAX_HYPOTHESES hypotheses");
  }
  static_assert(PFMPE_REFINE_MULTI_MAX_HYPOTHESES <= kPairsChunk, "one launch without a grid stride");
  pfmpe_refine_plan plan[PFMPE_REFINE_MAX_STREAMS];
  pfmpe_refine_plan_total tot;
  pfmpe_plan::refine_plan(Ks, Bs, S, plan, &tot);
  RET(set_device(c0));
  // the device block: the upload, then summaries, rows and covariances; the pinned block mirrors it
  const size_t up = (size_t)tot.upload_bytes, down = (size_t)tot.download_bytes, all = up + down;
  RET(c0->d_refm.grow(c0, all, all + all / 2));
  RET(c0->h_refm.grow(c0, all, all + all / 2));
  unsigned char* h = c0->h_refm.get();
  unsigned char* d = c0->d_refm.get();
  std::memset(h, 0, up);  // the gaps between regions and unused marker slots: the same bytes for the same plan
  RefineDesc* ds = (RefineDesc*)(h + tot.desc_offset);
  int32_t* stream_of = (int32_t*)(h + tot.stream_of_offset);
  for (int s = 0; s < S; ++s) {
    const pfmpe_ctx* c = ctxs[s];
    const size_t K = (size_t)Ks[s], first = (size_t)plan[s].first;
    ds[s].model_offset = plan[s].model_offset;
    ds[s].blobs_offset = plan[s].blobs_offset;
    ds[s].first = plan[s].first;
    ds[s].count = Ks[s];
    ds[s].max_iter = st[s].prm.max_iter;
    ds[s].revert = st[s].prm.revert_on_divergence ? 1 : 0;
    ds[s].converged = st[s].prm.converged;
    for (size_t i = 0; i < K; ++i) stream_of[first + i] = s;
    if (K > 0) {
      std::memcpy(h + tot.poses_offset + first * 12 * sizeof(double), in[s].poses, K * 12 * sizeof(double));
      std::memcpy(h + tot.corr_offset + first * kPairRow * sizeof(uint32_t), in[s].corr, K * kPairRow * sizeof(uint32_t));
    }
    std::memcpy(h + plan[s].model_offset, c->markers, sizeof(c->markers));
    std::memcpy(h + plan[s].model_offset + sizeof(c->markers), c->K, sizeof(c->K));
    if (st[s].B > 0) std::memcpy(h + plan[s].blobs_offset, st[s].blobs, 2 * (size_t)st[s].B * sizeof(double));
  }
  RefineMultiArgs ma{};
  ma.up = d;
  ma.desc = (const RefineDesc*)(d + tot.desc_offset);
  ma.stream_of = (const int32_t*)(d + tot.stream_of_offset);
  ma.poses = (const double*)(d + tot.poses_offset);
  ma.corr = (const uint32_t*)(d + tot.corr_offset);
  const size_t o_rows = up + (size_t)S * sizeof(pfmpe_refine_out), o_cov = o_rows + (size_t)H * sizeof(pfmpe_refine_row);
  ma.out = (pfmpe_refine_out*)(d + up);
  ma.rows = (pfmpe_refine_row*)(d + o_rows);
  ma.cov = (double*)(d + o_cov);
  ma.H = (int32_t)H;
  // what comes back: the summaries, then the rows and the covariances as far as somebody wants them
  bool want_rows = false, want_cov = false;
  for (int s = 0; s < S; ++s) {
    want_rows = want_rows || (rows && rows[s] && Ks[s] > 0);
    want_cov = want_cov || (cov && cov[s] && Ks[s] > 0);
  }
  const size_t back = want_cov ? down : want_rows ? o_cov - up : o_rows - up;
  HIPCHK(c0, hipMemcpyAsync(d, h, up, hipMemcpyHostToDevice, c0->stream));
  RET(refine_multi_launch(c0, ma, S));
  HIPCHK(c0, hipMemcpyAsync(h + up, d + up, back, hipMemcpyDeviceToHost, c0->stream));
  HIPCHK(c0, hipStreamSynchronize(c0->stream));
  std::memcpy(out, h + up, (size_t)S * sizeof(pfmpe_refine_out));
  for (int s = 0; s < S; ++s) {
    const size_t K = (size_t)Ks[s], first = (size_t)plan[s].first;
    if (K == 0) continue;
    if (rows && rows[s]) std::memcpy(rows[s], h + o_rows + first * sizeof(pfmpe_refine_row), K * sizeof(pfmpe_refine_row));
    if (cov && cov[s]) std::memcpy(cov[s], h + o_cov + first * 36 * sizeof(double), K * 36 * sizeof(double));
  }
  return PFMPE_OK;
}

int pfmpe_host_optimise_pose(const double* markers_xyz, int M, const double* K, const double* blobs, int B,
                             const uint32_t* corr, int n_rows, const pfmpe_refine_params* params, const double* pose12,
                             pfmpe_refine_row* row, double* cov36) {
  pfmpe_refine_params prm;
  pfmpe_default_refine_params(&prm);
  if (params) prm = *params;
  if (!markers_xyz || !K || !pose12 || !row || M < 1 || B < 0 || n_rows < 0 || (B > 0 && !blobs) || (n_rows > 0 && !corr))
    return PFMPE_E_ARG;
  if (!refine_params_ok(prm) || !refine_corr_ok(corr, (size_t)n_rows, M, B) || !refine_poses_finite(pose12, 1))
    return PFMPE_E_ARG;
  double cov[36];
  gn_optimise(markers_xyz, K, blobs, corr, n_rows, prm.max_iter, prm.revert_on_divergence ? 1 : 0, prm.converged, pose12,
              *row, cov);
  if (cov36) std::memcpy(cov36, cov, sizeof(cov));
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

// the twist the cloud-statistics kernel forms for one particle
void pfmpe_host_pose_twist(const double* pose12, const double* ref_pose12, double* twist6) {
  pose_twist(pose12, ref_pose12, twist6);
}

}  // extern "C"
