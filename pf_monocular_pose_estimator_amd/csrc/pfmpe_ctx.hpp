#pragma once
// pfmpe_ctx.hpp — the context and what every translation unit of the library does with it: owned buffers, errors,
// stream ordering, the timed launch wrappers and scope, the frame record, the entries' shared preambles, a blocking
// batch's members.  No kernel: the step's sequences are in pfmpe_seq.hpp, a side call's kernels with its subject.
//
// Replaces the PF block of PoseEstimator::estimateBodyPose (pf_mpe_lib/src/pose_estimator.cpp:475-733)
// behind include/pfmpe.h.  Device layout (DESIGN.md "HBM layout"): particle state as 12 SoA planes
// (r00 r01 r02 t0 r10 r11 r12 t1 r20 r21 r22 t2) of `ld` elements each, double-buffered (prior /
// posterior); two weight slots (current iteration / best iteration so far); per-block partials;
// one control record; one output record copied to pinned host memory at the end of the frame.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <hip/hip_fp16.h>

#include <time.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstddef>
#include <cstring>
#include <string>
#include <map>
#include <memory>
#include <optional>
#include <type_traits>
#include <vector>

#include "../../include/pfmpe.h"
#include "pf_types.hpp"

using namespace pfmpe;

static_assert(offsetof(OutDev, kept_slot) == sizeof(pfmpe_frame_out), "OutDev must start with pfmpe_frame_out");
static_assert(offsetof(OutDev, corr) == offsetof(pfmpe_frame_out, corr), "OutDev layout");
static_assert(offsetof(OutDev, prob_sum) == offsetof(pfmpe_frame_out, prob_sum), "OutDev layout");
static_assert(PFMPE_MAX_MARKERS == kMaxMarkers, "marker capacity mismatch");
static_assert(PFMPE_MAX_BLOBS == kMaxBlobs, "blob capacity mismatch");

struct EventPair {
  hipEvent_t a, b;
  int kid;
};

// A batch leader's fence (pfmpe_step_multi), shared by the batch's other contexts until their next work is ordered
// after the batch; destroyed with the last reference.  The event is recorded on the leader's stream lazily: when a
// member needs the order (order_after, destroy), or when the leader puts other work on its stream while members
// still hold the fence (seal_lead_fence, ADVICE r05: a member's read-back then does not wait for the leader's later
// frames).  A steady multi-stream loop, whose members never use their own streams, records nothing (one record per
// batch cost 3-5 us of host time per batch).  stream: the leader's stream; null once the leader was destroyed (its
// destroy drained the stream first, so nothing of the batch is pending then).  recorded: the event holds the end of
// the fence's latest batch.
struct BatchFence {
  hipEvent_t ev = nullptr;
  hipStream_t stream = nullptr;
  bool recorded = false;
  ~BatchFence() {
    if (ev) (void)hipEventDestroy(ev);
  }
};

// ---------------------------------------------------------------------- owned GPU buffers
// Every block of device or pinned host memory of the engine is owned by a Buf: move-only, freed by its destructor
// with the call that matches its kind, so nothing is freed by a list somebody has to keep.  A mapped buffer keeps its
// device address beside the host one (dev()), so a regrown buffer cannot leave a stale alias behind.
enum class Mem { Device, Pinned, Mapped };  // hipMalloc; hipHostMalloc default; mapped + coherent (device-readable)
// blocks alive in this process (undocumented info key 115: a deterministic leak check on a shared device)
inline std::atomic<int64_t>& live_blocks() {
  static std::atomic<int64_t> n{0};
  return n;
}
template <typename T, Mem K = Mem::Device>
class Buf {
 public:
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept { swap(o); }
  Buf& operator=(Buf&& o) noexcept {
    Buf t(std::move(o));
    swap(t);
    return *this;
  }
  ~Buf() { reset(); }
  void swap(Buf& o) noexcept {
    std::swap(p_, o.p_);
    std::swap(dev_, o.dev_);
    std::swap(cap_, o.cap_);
  }
  T* get() const { return p_; }
  T* dev() const { return dev_; }  // Mem::Mapped: the block's device address
  size_t bytes() const { return cap_; }
  explicit operator bool() const { return p_ != nullptr; }
  // A block of `bytes` in place of the present one (if any); an error leaves the buffer empty.
  int alloc(pfmpe_ctx* c, size_t bytes);
  // allocate on first use
  int ensure(pfmpe_ctx* c, size_t bytes) { return p_ ? PFMPE_OK : alloc(c, bytes); }
  // Grow on demand: a block of `capacity` bytes when the present one holds fewer than `need` (the growth policy is
  // the caller's).  The context's stream is drained before the old block is freed: work enqueued on it may still
  // read it.  Contents are not kept.
  int grow(pfmpe_ctx* c, size_t need, size_t capacity);
  void reset() {
    if (p_) {
      (void)(K == Mem::Device ? hipFree((void*)p_) : hipHostFree((void*)p_));
      live_blocks() -= 1;
    }
    p_ = dev_ = nullptr;
    cap_ = 0;
  }

 private:
  T* p_ = nullptr;
  T* dev_ = nullptr;
  size_t cap_ = 0;
};

// The stream and the events of a context.  A base of pfmpe_ctx, so its destructor runs after pfmpe_ctx's members are
// gone: at destroy the buffers go first, then the timing events and own_ev, and the stream last.
struct CtxQueue {
  hipStream_t stream = nullptr;
  std::vector<EventPair> ev_pool;  // timing brackets
  hipEvent_t own_ev = nullptr;     // cross-stream ordering (order_after)
  CtxQueue() = default;
  CtxQueue(const CtxQueue&) = delete;
  CtxQueue& operator=(const CtxQueue&) = delete;
  ~CtxQueue() {
    for (auto& e : ev_pool) {
      (void)hipEventDestroy(e.a);
      (void)hipEventDestroy(e.b);
    }
    if (own_ev) (void)hipEventDestroy(own_ev);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

struct pfmpe_ctx : CtxQueue {
  int device = 0;
  int max_particles = 0, max_markers = 0, max_blobs = 0, state_dtype = PFMPE_STATE_F32;
  size_t es = 4;       // bytes per state element (4 fp32, 8 fp64, 2 fp16 deltas)
  size_t ws = 4;       // bytes per weight (compute type)
  double anchor[2][12] = {{0}};  // fp16 state: anchor pose of each state buffer
  int64_t ld = 0;      // plane stride (elements)
  int max_blk = 0;

  Buf<void> d_state[2];
  int prior_idx = 0;
  Buf<void> d_w[2];
  Buf<void> d_prop[2];  // two-launch path: propagated set per weight slot (keep_prop)
  // Deferred resampling (PFMPE_OPT_DEFER_RESAMPLE): a two-launch frame with the kept set writes the
  // new prior's owner indices (d_owner[frame_owner_out]) instead of the particles; the frame's kept buffer then
  // becomes the prior's storage (swapped with the unused post buffer at take_step) and prior particle n is stored
  // row d_owner[prior_owner][n].  prior_owner = -1: the prior is stored in particle order.
  Buf<uint32_t> d_owner[2];
  int prior_owner = -1;
  int frame_owner_out = -1;  // this frame's owner buffer (-1: materialised resample)
  bool defer = true;
  int max_grp = 0;
  Buf<BlockPart> d_part[2];
  Buf<BlockScan> d_bscan[2];
  Buf<GroupPart> d_gpart[2];
  Buf<GroupScan> d_gscan;
  Buf<CountPart> d_cpart;
  Buf<unsigned long long> d_winkey;  // kWinShards winner keys + the owners finish's arrival shards (kWinBytes), zero between frames
  Buf<CountPart> d_cgroup;
  Buf<uint32_t> d_counters;  // [prop group x max_grp][prop top][res group x max_grp][res top]
  Buf<uint32_t> d_gen; // k_frame iteration release word (monotonic)
  Buf<Cand> d_cand; // per-block winner candidates
  Buf<double> d_mlpose; // most likely pose (12)
  Buf<uint32_t> d_pairs; // pair rows of one chunk of particles, then their counts (pfmpe_get_pairs)
  Buf<unsigned char> d_refine; // Gauss-Newton refinement scratch (RefineBuf layout, pfmpe_refine_*)
  // pfmpe_top_particles: the selection's scratch and the record (pf_top.hpp TopBuf; one size for every N and K,
  // allocated on first use), and the pinned block the record is read back into
  Buf<unsigned char> d_top;
  Buf<unsigned char, Mem::Pinned> h_top;
  // pfmpe_refine_multi (owned by the batch's first context): the packed upload followed by the batch's summaries,
  // rows and covariances, and the pinned block the upload is built in and the results land in; grown on demand
  Buf<unsigned char> d_refm;
  Buf<unsigned char, Mem::Pinned> h_refm;
  // pfmpe_step_refine / pfmpe_step_refine_multi (owned by the call's context / the batch's first context): the mapped
  // pinned block of pf_tail.hpp, which the host writes once per call and k_step_tail reads and publishes into (the
  // descriptors, every stream's tail record, every stream's fp64 model and blobs); grown on demand, never shrunk.
  // tail_S: streams of the fused call now running on this context's stream (0: none, no tail is launched).
  Buf<unsigned char, Mem::Mapped> h_tail;
  int tail_S = 0;
  int32_t tail_seq0 = 0;           // a single call: the context's sequence number when the call began
  int64_t tail_fallbacks = 0;      // PFMPE_INFO_TAIL_FALLBACKS
  Buf<unsigned char> d_init;       // initialisation scratch (pfmpe_init.hip), grown on demand
  // the initialisation (owned by the batch's first context; pfmpe_initialise and pfmpe_p3p_histogram are batches of
  // one): the pinned block its read-backs land in (every stream's histogram; every stream's check results), grown on
  // demand
  Buf<unsigned char, Mem::Pinned> h_init;
  Buf<unsigned char> d_det;        // detector scratch (pfmpe_detect.hip), grown on demand
  Buf<uint8_t> d_img;              // staged camera image (pfmpe_stage_image), grown on demand
  int img_w = 0, img_h = 0, img_pitch = 0;
  Buf<void, Mem::Mapped> h_det;    // detector output record (pinned, host-mapped)
  // pfmpe_find_leds_multi: the batch scratch (counters, batch head + descriptors, work list, then every ROI's
  // regions; grown on demand), the pinned image of the head + descriptors, and R pinned, host-mapped output records
  Buf<unsigned char> d_detm;
  Buf<unsigned char, Mem::Mapped> h_detm;
  Buf<void, Mem::Mapped> h_detm_out;  // grown on demand
  // pfmpe_find_leds_streams (owned by the batch's first context): the pinned, host-mapped pack of the ROI crops of the
  // batch's host images, grown on demand; on the device they land in a region of d_detm
  Buf<uint8_t, Mem::Mapped> h_detm_pix;
  // pfmpe_predict_roi_multi (owned by the batch's first context; pfmpe_predict_roi is a batch of one): the batch
  // scratch (head + descriptors, then one partial per block of the batch; grown on demand), and the pinned,
  // host-mapped image of the head + descriptors followed by the result boxes of PFMPE_ROI_MAX_STREAMS streams
  Buf<unsigned char> d_roim;
  Buf<unsigned char, Mem::Mapped> h_roim;
  // pfmpe_cloud_stats_multi (owned by the batch's first context; pfmpe_cloud_stats is a batch of one): the batch
  // scratch (head + descriptors, then one partial row per block of the batch; grown on demand, never shrunk), and the
  // pinned, host-mapped image of the head + descriptors followed by the result rows of PFMPE_CLOUD_MAX_STREAMS entries
  Buf<unsigned char> d_cloudm;
  Buf<unsigned char, Mem::Mapped> h_cloudm;
  // pfmpe_cloud_modes: the member counts of the K + 1 modes (kModesCountBytes), then a byte per particle, N rounded
  // up to 4 (grown on demand, never shrunk); and the pinned block the counts are read back into
  Buf<unsigned char> d_modes;
  Buf<unsigned char, Mem::Pinned> h_modes;
  // pfmpe_resample_prior with a mode filter (owned by dst, which also lends d_modes / h_modes): the member total, then
  // the member prefixes of the source's 256-particle blocks (RsLayout, pfmpe_resample_prior.hip); grown on demand,
  // never shrunk
  Buf<unsigned char> d_resample;
  // pfmpe_assoc_stats_multi (owned by the batch's first context; pfmpe_assoc_stats is a batch of one): the device copy of the batch's image (launch heads,
  // descriptors, every entry's blob table) followed by the bins of all entries, and the pinned block the image is
  // built in and the bins are read back into (same layout); grown on demand, never shrunk
  Buf<unsigned char> d_assocm;
  Buf<unsigned char, Mem::Pinned> h_assocm;
  int num_cu = 0;
  bool coop = false;               // device supports cooperative launches
  int fused = 2;                   // PFMPE_OPT_FUSED: 2 flat one-launch (k_frame2), 1 tree (k_frame), 0 two launches
  Buf<uint32_t> d_flat; // k_frame2 sharded arrival counters (kFlatWords)
  Buf<unsigned char> d_gran; // k_frame2 granule hand-offs (kGranBytes: block partials x 2 parities, counts)
  uint32_t gframe = 0;             // granule tag frame count (1 .. kGranFrames; the area is zeroed on wrap)
  uint32_t flat_base_w = 0, flat_base_c = 0;  // their running totals (host mirror)
  int64_t fused_fallbacks = 0;     // fused frames redone with two launches
  int fused_user = 2;              // the PFMPE_OPT_FUSED value asked for (fused drops to 0 after a fallback)
  int64_t fused_rearm = 0;         // PFMPE_OPT_FUSED_REARM: clean two-launch frames before fusing again (0: never)
  int64_t clean_since_fallback = 0;
  int64_t wait_bound_us = 2000000; // PFMPE_OPT_WAIT_BOUND_US: bound of every in-launch wait
  int64_t multi_max_blocks = 160000; // PFMPE_OPT_MULTI_MAX_BLOCKS: largest batch this context leads (blocks)
  int last_shape = -1;             // PFMPE_SHAPE_* of the last frame
  int last_weigh_pass = -1;        // PFMPE_WEIGH_* of the last two-launch weighing launch
  int last_resample = -1;          // PFMPE_RESAMPLE_* of the last two-launch resampling launch
  int64_t guard_skips = 0;         // one-launch frames run as two launches because another was in flight
  std::map<std::pair<const void*, size_t>, int> occ;  // (kernel, LDS bytes) -> blocks per CU
  // host-side timing of batches this context leads (undocumented info keys 110-114): entry -> first launch,
  // the launches, last launch -> records, records -> return, batches counted
  int64_t mt_enter = 0, mt_ns[4] = {0, 0, 0, 0}, mt_batches = 0;
  Buf<Ctrl> d_ctrl;
  Buf<RecOut, Mem::Mapped> h_rec;  // pinned host memory: the record granules, written by the final wave (dev())
  std::unique_ptr<OutDev> h_out;   // the last record, unpacked on the host by wait_frame
  int32_t seq = 0;               // frame-record sequence number (publication tag = 2 * seq + finished)
  Buf<unsigned char> d_table;        // this frame's blob table (BlobTable<T> layout)
  Buf<unsigned char, Mem::Pinned> h_table;  // pinned staging
  Buf<unsigned char> d_bank;         // staged tables of a whole stream, back to back
  std::vector<size_t> bank_off;      // byte offset of frame f's table
  std::vector<int32_t> bank_B;
  std::vector<GridHdr> bank_grid;    // frame f's table grid header (host copy, for the kernel arguments)
  std::vector<double> bank_blobs;    // the staged blobs and per-frame offsets, kept to rebuild the tables when
  std::vector<int32_t> bank_offsets; // set_params changes tol_PF (the grid's window depends on it)
  double bank_tol_pf = 0.0;          // the tol_PF the bank's tables were built for
  int last_grid = -1;                // PFMPE_INFO_LAST_GRID
  Buf<double> d_xfer;            // N x 12 doubles
  Buf<uint32_t> d_counts;
  Buf<uint64_t> d_stamps;        // diagnostic stamps (diag & 4)
  // batch scratch (pfmpe_step_multi, owned by the batch's first context): stream descriptors, the
  // block -> stream map and host-supplied blob tables; the host writes the descriptors and tables into the
  // pinned image, a staging launch (k_stage_multi) moves them to HBM and builds the map
  Buf<unsigned char> d_multi;
  Buf<unsigned char, Mem::Mapped> h_multi;  // as large as d_multi
  hipEvent_t br_a = nullptr, br_b = nullptr;  // the open timing bracket (launch / klaunch)
  uint32_t multi_gen = 0;  // batch generation: one per staging launch this context leads (StreamDesc::gen)
  std::vector<int64_t> map_sig;  // the block map now in d_multi: {boff, total, then (first, nblk) per stream}
  // Cross-stream ordering.  A context's work runs on its own stream (pfmpe_step, read-backs, ...) or, inside a
  // batch, on the batch leader's stream.  last_stream is where its latest work went (nullptr: none since
  // create); when the next work goes to a different stream it is ordered after that work: through the
  // leader's fence when the latest work was a batch, else through own_ev recorded then on the own stream.
  hipStream_t last_stream = nullptr;
  std::shared_ptr<BatchFence> last_fence;
  std::shared_ptr<BatchFence> lead_fence;  // this context as a batch leader

  // model / params
  int M = 0;
  double markers[kMaxMarkers * 3] = {0};
  double K[9] = {0};
  uint32_t downgrade = 0;
  bool has_model = false;
  pfmpe_params params{};
  int N = 0;
  bool has_prior = false;

  // options
  bool record_counts = false;
  bool prune = true;
  bool keep_prop = true;           // PFMPE_OPT_KEEP_PROPAGATED (batched fp32 / fp64 frames regenerate: step_multi)
  int timing = 0;          // HIP-event sampling period in frames (0 = off)
  bool timing_now = false;  // this frame's launches are bracketed
  int64_t timing_frame = 0;
  int diag = 0;

  // last step (for get_particles / get_weights)
  FrameArgsT<float> last_fa_f{};
  FrameArgsT<double> last_fa_d{};
  bool has_last = false;
  int last_prior_idx = 0;
  bool last_accepted = false;
  int last_kept_slot = 0, last_kept_iter = 0;

  // timing
  size_t ev_used = 0;
  int64_t k_launches[PFMPE_K_COUNT] = {0};
  double k_ms[PFMPE_K_COUNT] = {0};

  std::string err;
};

namespace pfmpe_impl {

// One spin-waiting (one-launch) frame per device at a time within this process: two such kernels that each
// hold part of the CUs could wait on each other until the wait bound abandons a frame.  A context that finds
// its device busy runs the frame as two launches (they never wait on other blocks, so they always drain).
constexpr int kMaxDevices = 64;
inline std::atomic<int>& fused_inflight(int dev) {
  static std::atomic<int> flags[kMaxDevices];
  return flags[(dev >= 0 && dev < kMaxDevices) ? dev : 0];
}

inline int fail(pfmpe_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

#define HIPCHK(ctx, expr)                                                                       \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return fail((ctx), PFMPE_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));       \
  } while (0)

#define RET(expr)              \
  do {                         \
    int r_ = (expr);           \
    if (r_ != PFMPE_OK) return r_; \
  } while (0)

}  // namespace pfmpe_impl

template <typename T, Mem K>
int Buf<T, K>::alloc(pfmpe_ctx* c, size_t bytes) {
  reset();
  void* p = nullptr;
  const hipError_t e = K == Mem::Device   ? hipMalloc(&p, bytes)
                       : K == Mem::Pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault)
                                          : hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent);
  if (e != hipSuccess)
    return pfmpe_impl::fail(c, PFMPE_E_HIP, "allocating " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
  live_blocks() += 1;
  p_ = (T*)p;
  cap_ = bytes;
  if (K == Mem::Mapped) {
    void* d = nullptr;
    if (const hipError_t g = hipHostGetDevicePointer(&d, p, 0); g != hipSuccess) {
      reset();
      return pfmpe_impl::fail(c, PFMPE_E_HIP, std::string("hipHostGetDevicePointer: ") + hipGetErrorString(g));
    }
    dev_ = (T*)d;
  }
  return PFMPE_OK;
}
template <typename T, Mem K>
int Buf<T, K>::grow(pfmpe_ctx* c, size_t need, size_t capacity) {
  if (need <= cap_) return PFMPE_OK;
  if (p_)
    if (const hipError_t e = hipStreamSynchronize(c->stream); e != hipSuccess)
      return pfmpe_impl::fail(c, PFMPE_E_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
  return alloc(c, capacity);
}

// ---------------------------------------------------------------------- state-type dispatch
// The one place that maps a context's storage type (and RNG mode) to the template arguments of the kernels:
// f is called with a tag whose T is the compute type and SP the storage type (RNG: kRngReference / kRngPhilox).
template <typename T_, typename SP_, int RNG_ = 0>
struct StateTag {
  using T = T_;
  using SP = SP_;
  static constexpr int RNG = RNG_;
};
template <typename F>
auto visit_state(const pfmpe_ctx* c, F&& f) {
  switch (c->state_dtype) {
    case PFMPE_STATE_F64: return f(StateTag<double, double>{});
    case PFMPE_STATE_F16: return f(StateTag<float, __half>{});
    default: return f(StateTag<float, float>{});
  }
}
template <typename F>
auto visit_state_rng(const pfmpe_ctx* c, F&& f) {
  return visit_state(c, [&](auto s) {
    using S = decltype(s);
    return c->params.rng_mode == PFMPE_RNG_REFERENCE ? f(StateTag<typename S::T, typename S::SP, kRngReference>{})
                                                     : f(StateTag<typename S::T, typename S::SP, kRngPhilox>{});
  });
}
// The marker-count buckets (pf_types.hpp marker_live): f is called with the bucket's MAXM as an integral constant.
// exact5: the 5-slot bucket, which serves exactly kExactM markers; otherwise the smallest of 8, 12, 16 that holds M.
template <typename F>
auto visit_m(int M, bool exact5, F&& f) {
  if (exact5) return f(std::integral_constant<int, kExactM>{});
  if (M <= 8) return f(std::integral_constant<int, 8>{});
  if (M <= 12) return f(std::integral_constant<int, 12>{});
  return f(std::integral_constant<int, 16>{});
}

namespace pfmpe_impl {

// Order work about to be enqueued for context c on stream `to` after c's latest work, when that went to
// another stream (a batch runs on the leader's stream, unordered with each member's own stream).
// Free when consecutive work stays on one stream, which is every steady-state loop (pfmpe_step only, or
// batches of the same contexts only).  err: the context that reports a failure.
inline int order_after(pfmpe_ctx* c, hipStream_t to, pfmpe_ctx* err) {
  if (!c->last_stream || c->last_stream == to) return PFMPE_OK;
  if (c->last_fence) {
    if (c->last_fence->stream) {
      if (!c->last_fence->recorded) {
        HIPCHK(err, hipEventRecord(c->last_fence->ev, c->last_fence->stream));
        c->last_fence->recorded = true;
      }
      HIPCHK(err, hipStreamWaitEvent(to, c->last_fence->ev, 0));
    }
  } else {
    if (!c->own_ev) HIPCHK(err, hipEventCreateWithFlags(&c->own_ev, hipEventDisableTiming));
    HIPCHK(err, hipEventRecord(c->own_ev, c->last_stream));
    HIPCHK(err, hipStreamWaitEvent(to, c->own_ev, 0));
  }
  c->last_stream = nullptr;
  c->last_fence.reset();
  return PFMPE_OK;
}

// A batch leader about to put other work on its stream while members of its latest batch still hold the fence:
// record the fence first, so their order_after waits for the batch and not for this later work.
inline int seal_lead_fence(pfmpe_ctx* c) {
  BatchFence* f = c->lead_fence.get();
  if (!f || f->recorded || c->lead_fence.use_count() < 2) return PFMPE_OK;
  HIPCHK(c, hipEventRecord(f->ev, c->stream));
  f->recorded = true;
  return PFMPE_OK;
}

// Every C-ABI entry that enqueues work on the context's own stream starts here: the device, the leader's fence, then
// the order after the context's latest batch (if any).
inline int set_device(pfmpe_ctx* c) {
  HIPCHK(c, hipSetDevice(c->device));
  if (const int r_ = seal_lead_fence(c)) return r_;
  if (const int r_ = order_after(c, c->stream, c)) return r_;
  c->last_stream = c->stream;
  return PFMPE_OK;
}

// ---------------------------------------------------------------------- timed launch wrapper
// A bracketed launch passes its events to the dispatch itself (hipExtLaunchKernel: the start event takes the
// first kernel's start, the stop event each kernel's end, so the last one's), so the bracket is the kernels'
// own execution time as the profiler's kernel trace reports it.  Plain hipEventRecord brackets on an idle
// stream (every one-launch frame: the host waited for the previous record) also held the dispatch of the
// kernel, +8 us at C2 (37.5 against rocprofv3's 29.4).  Every kernel of a launch_ext bracket goes through
// klaunch.
inline int open_bracket(pfmpe_ctx* c, int kid, EventPair** out) {
  *out = nullptr;
  if (!c->timing_now) return PFMPE_OK;
  if (c->ev_used == c->ev_pool.size()) {
    EventPair p{};
    p.kid = kid;
    HIPCHK(c, hipEventCreate(&p.a));
    HIPCHK(c, hipEventCreate(&p.b));
    c->ev_pool.push_back(p);
  }
  *out = &c->ev_pool[c->ev_used++];
  (*out)->kid = kid;
  return PFMPE_OK;
}
// the PF frame's kernels (launched through klaunch)
template <typename Launch>
int launch_ext(pfmpe_ctx* c, int kid, Launch&& fn) {
  EventPair* ep = nullptr;
  if (const int r_ = open_bracket(c, kid, &ep)) return r_;
  if (ep) {
    c->br_a = ep->a;
    c->br_b = ep->b;
  }
  fn();
  c->br_a = c->br_b = nullptr;
  HIPCHK(c, hipGetLastError());
  return PFMPE_OK;
}
// the initialisation, ROI and detector launches: hipEventRecord brackets around the stream's work
template <typename Launch>
int launch(pfmpe_ctx* c, int kid, Launch&& fn) {
  EventPair* ep = nullptr;
  if (const int r_ = open_bracket(c, kid, &ep)) return r_;
  if (ep) HIPCHK(c, hipEventRecord(ep->a, c->stream));
  fn();
  HIPCHK(c, hipGetLastError());
  if (ep) HIPCHK(c, hipEventRecord(ep->b, c->stream));
  return PFMPE_OK;
}
template <typename... KArgs, typename... Args>
inline void klaunch(pfmpe_ctx* c, void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, Args... args) {
  if (c->br_b) {
    hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, c->stream, c->br_a, c->br_b, 0u, args...);
    c->br_a = nullptr;  // the bracket starts at its first kernel
  } else {
    hipLaunchKernelGGL(kernel, grid, block, lds, c->stream, args...);
  }
}

// The timing scope of a host-synchronous entry (detector, ROI, initialisation): fn with the brackets of c (a batch's
// leader) on.  timing_now is cleared on every exit; a failure drops the brackets this call opened and left unharvested
// (one may lack its end event, which the next harvest would trip over), the pending ones of earlier frames stay.
template <typename F>
int timed(pfmpe_ctx* c, F&& fn) {
  const size_t ev_mark = c->ev_used;
  c->timing_now = c->timing > 0;
  const int rc = fn();
  c->timing_now = false;
  if (rc != PFMPE_OK && c->ev_used > ev_mark) c->ev_used = ev_mark;
  return rc;
}

// Brackets are harvested lazily: a timed PF frame leaves its event pairs pending (no stream synchronize on the
// frame path, which had added a host round trip to every sampled frame: at --steps 20 one frame in two), and
// they are read here, when the pool holds kHarvestPairs of them, at pfmpe_get_kernel_stats, or after the
// host-synchronous entries (ROI, read-backs, initialisation, detector).  Every bracket is recorded on c->stream,
// so waiting for the last one's end event completes them all.
constexpr size_t kHarvestPairs = 256;
constexpr size_t kEventPrealloc = 64;  // event pairs created when timing is switched on (PFMPE_OPT_TIMING)
inline int harvest_timing(pfmpe_ctx* c) {
  if (c->ev_used == 0) return PFMPE_OK;
  HIPCHK(c, hipEventSynchronize(c->ev_pool[c->ev_used - 1].b));
  for (size_t i = 0; i < c->ev_used; ++i) {
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev_pool[i].a, c->ev_pool[i].b));
    c->k_launches[c->ev_pool[i].kid] += 1;
    c->k_ms[c->ev_pool[i].kid] += ms;
  }
  c->ev_used = 0;
  return PFMPE_OK;
}

// Wait for the frame record: the final wave writes it into pinned host memory as tagged granules (RecOut),
// so the host spins on those words instead of paying a stream synchronize, and unpacks them into h_out once
// every granule carries the tag.  Granule 0 alone with an even tag is an unfinished iteration batch.  The
// spin is bounded by hipStreamQuery: an idle stream without a record is an error.
inline bool take_record(pfmpe_ctx* c, int32_t want) {
  volatile const uint64_t* g = c->h_rec.get()->g;
  const uint32_t t = (uint32_t)(g[0] >> 32);
  if ((int32_t)(t >> 1) != want) return false;
  if (t & 1u) {
    for (int k = kRecWords - 1; k > 0; --k)
      if ((uint32_t)(g[k] >> 32) != t) return false;
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    uint32_t* w = (uint32_t*)c->h_out.get();
    for (int k = 0; k < kRecWords; ++k) w[k] = (uint32_t)g[k];
  }
  c->h_out->tag = (int32_t)t;
  return true;
}
// The stream is queried only after the record has been awaited for kQueryAfterNs, then at that interval: a query
// costs microseconds of host time (3.4 us under the HIP API trace), and one issued while the record lands delays
// the frame by that much (at C2 the old every-1,024-spins query fell inside nearly every frame).
constexpr int64_t kQueryAfterNs = 200000;
inline int64_t now_ns() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (int64_t)ts.tv_sec * 1000000000ll + ts.tv_nsec;
}
inline int wait_frame(pfmpe_ctx* c, hipStream_t on = nullptr) {  // on: the frame's stream
  const int32_t want = c->seq;
  int64_t next_query = 0;
  for (uint64_t spin = 0;; ++spin) {
    if (take_record(c, want)) return PFMPE_OK;
    if ((spin & 63u) != 63u) {
      __builtin_ia32_pause();
      continue;
    }
    const int64_t t = now_ns();
    if (next_query == 0) next_query = t + kQueryAfterNs;
    if (t >= next_query) {
      next_query = t + kQueryAfterNs;
      const hipError_t q = hipStreamQuery(on ? on : c->stream);
      if (q == hipSuccess) {
        if (take_record(c, want)) return PFMPE_OK;
        return fail(c, PFMPE_E_HIP, "frame record was not written");
      }
      if (q != hipErrorNotReady) return fail(c, PFMPE_E_HIP, std::string("stream error: ") + hipGetErrorString(q));
    }
    __builtin_ia32_pause();
  }
}

inline size_t counters_bytes(const pfmpe_ctx* c) { return (size_t)(2 * c->max_grp + 2) * sizeof(uint32_t); }

inline bool frame_done(const pfmpe_ctx* c) { return (c->h_out->tag & 1) != 0; }

// ---------------------------------------------------------------------- typed launch sequence
template <typename T> FrameArgsT<T>& last_args(pfmpe_ctx* c);
template <> inline FrameArgsT<float>& last_args<float>(pfmpe_ctx* c) { return c->last_fa_f; }
template <> inline FrameArgsT<double>& last_args<double>(pfmpe_ctx* c) { return c->last_fa_d; }

// the two-launch path's propagated-set buffers (PFMPE_OPT_KEEP_PROPAGATED), allocated on first use: the
// one-launch frames keep the propagated particle in registers and never need them
inline int ensure_prop(pfmpe_ctx* c) {
  if (!c->keep_prop) return PFMPE_OK;
  for (int i = 0; i < 2; ++i) RET(c->d_prop[i].ensure(c, (size_t)kPlanes * c->ld * c->es));
  if (c->defer && !c->d_owner[0]) {  // both or neither: deferral is gated on both pointers
    Buf<uint32_t> own[2];
    for (auto& o : own)
      if (o.alloc(c, (size_t)c->ld * sizeof(uint32_t)) != PFMPE_OK) return fail(c, PFMPE_E_HIP, "owner buffers: " + c->err);
    for (int i = 0; i < 2; ++i) c->d_owner[i].swap(own[i]);
  }
  return PFMPE_OK;
}
// the owner indices of the current prior (null: stored in particle order)
inline const uint32_t* prior_owner_ptr(const pfmpe_ctx* c) {
  return c->prior_owner >= 0 ? c->d_owner[c->prior_owner].get() : nullptr;
}

// ---------------------------------------------------------------------- shared preambles of the entry points
// Defined in pfmpe_engine.hip, used by the side calls' units as well: the byte offset of a table's GridHdr; the frame's
// blob table for the context's current parameters, built at dst (returns its size); the kept iteration's propagated
// set regenerated into out (N x 12), or its particles list[i], i < min(*count, limit) (list, count, out on the device),
// both bracketed as PFMPE_K_AUX; the prior's first `count` particles into d_xfer, on the context's stream.
size_t grid_off(const pfmpe_ctx* c, int B);
size_t build_table(const pfmpe_ctx* c, const double* blobs, int B, unsigned char* dst);
int dispatch_regen(pfmpe_ctx* c, int kept_iter, const void* prior, double* out);
int dispatch_regen_list(pfmpe_ctx* c, int kept_iter, const void* prior, const int32_t* list, const uint32_t* count,
                        int limit, double* out);
int export_prior(pfmpe_ctx* c, int count);
// The argument and state checks shared by pfmpe_get_pairs / pfmpe_refine_cloud (pfmpe_assoc.hip; texts begin with
// `who`), then the call's blob table built into d_table (every frame that reads d_table writes it first) and, for the
// propagated set, the kept set regenerated into d_xfer and named by aa->dense.  *blobs_out / *B_out: the blobs the call
// means (resolve_blobs).
int assoc_prepare(pfmpe_ctx* c, const char* who, int which, const pfmpe_assoc_in* in, const double** blobs_out,
                  int* B_out, size_t* tbytes, GridHdr* gh, AssocArgs* aa);
// k_assoc_votes in rows mode for the context's state type, marker bucket and pruning option on its stream
// (pfmpe_assoc.hip): the pair rows (aa.corr, aa.n_corr) of the particles aa.first .. + aa.count of the regenerated kept
// set (aa.dense) or of the resident prior, against the blob table `table` (device, tbytes, grid header gh) of B blobs,
// with the context's current model and parameters.  Not bracketed by the timing events.
int assoc_rows_launch(pfmpe_ctx* c, int B, const unsigned char* table, size_t tbytes, const GridHdr& gh, AssocArgs aa);
// k_step_tail (pfmpe_refine.hip) for the c->tail_S streams staged in c->h_tail, on c's stream, bracketed as
// PFMPE_K_AUX: each stream's wave looks for the finished record of frame sequence seq0 + delta.
int tail_launch(pfmpe_ctx* c, int32_t delta);
// behind a launch that can finish context c's own frame (nothing unless a pfmpe_step_refine is running)
inline int tail_after(pfmpe_ctx* c) {
  return c->tail_S ? tail_launch(c, (c->seq - c->tail_seq0) & 0x3fffffff) : (int)PFMPE_OK;
}
// the transfer buffer (N x 12 doubles), written and read inside one blocking call by every user
inline int ensure_xfer(pfmpe_ctx* c) { return c->d_xfer.ensure(c, (size_t)c->max_particles * 12 * sizeof(double)); }
// the pair rows of one chunk of pairs_cap(c) particles, kPairsChunk at most (132 B per particle), then their counts
// (pfmpe_get_pairs, pfmpe_refine_*)
constexpr int kPairsChunk = 1 << 16;
constexpr size_t kPairRow = 2 * kMaxMarkers;
inline int pairs_cap(const pfmpe_ctx* c) { return std::min(c->max_particles, kPairsChunk); }
inline int ensure_pairs(pfmpe_ctx* c) {
  return c->d_pairs.ensure(c, (size_t)pairs_cap(c) * (kPairRow + 1) * sizeof(uint32_t));
}

// Which blobs a pfmpe_assoc_in means: the caller's, or a frame of the staged bank (the host copy kept for
// rebuilds).  Checks the request (texts begin with `who`, reported on `err`: c itself unless a batch's leader is
// given); *blobs / *B are the resolved list.
inline int resolve_blobs(const pfmpe_ctx* c, const std::string& who, const pfmpe_assoc_in* in, const double** blobs, int* B,
                         pfmpe_ctx* err) {
  if (in->B < 0) return fail(err, PFMPE_E_ARG, who + ": B < 0");
  *blobs = in->blobs;
  *B = in->B;
  if (in->bank_frame >= 0) {
    if (c->bank_offsets.empty() || in->bank_frame >= (int)c->bank_offsets.size() - 1)
      return fail(err, PFMPE_E_ARG, who + ": bank_frame out of range");
    *B = c->bank_offsets[in->bank_frame + 1] - c->bank_offsets[in->bank_frame];
    *blobs = c->bank_blobs.data() + 2 * (size_t)c->bank_offsets[in->bank_frame];
  } else if (*B > 0 && !*blobs) {
    return fail(err, PFMPE_E_ARG, who + ": null blobs");
  }
  if (*B > c->max_blobs) return fail(err, PFMPE_E_CAP, who + ": B exceeds max_blobs");
  return PFMPE_OK;
}
inline int resolve_blobs(pfmpe_ctx* c, const std::string& who, const pfmpe_assoc_in* in, const double** blobs, int* B) {
  return resolve_blobs(c, who, in, blobs, B, c);
}

// The members of a batch (pfmpe_step_multi, pfmpe_predict_roi_multi): none null, none twice, and each agreeing
// with ctxs[0] as same(c) tells (`what` names the properties); then the entry point's own checks of that stream,
// each(s, prefix).  Errors are reported on ctxs[0] as "<who>: stream <s>: ...".
template <typename Same, typename Each>
int check_members(pfmpe_ctx* const* ctxs, int S, const char* who, const char* what, Same&& same, Each&& each) {
  pfmpe_ctx* c0 = ctxs[0];
  for (int s = 0; s < S; ++s) {
    const pfmpe_ctx* c = ctxs[s];
    const std::string at = std::string(who) + ": stream " + std::to_string(s) + ": ";
    if (!c) return fail(c0, PFMPE_E_ARG, at + "null context");
    for (int e = 0; e < s; ++e)
      if (ctxs[e] == c) return fail(c0, PFMPE_E_ARG, at + "context appears twice");
    if (c->device != c0->device || c->state_dtype != c0->state_dtype || !same(c))
      return fail(c0, PFMPE_E_ARG, at + what + " must match ctxs[0]");
    RET(each(s, at));
  }
  return PFMPE_OK;
}

// Orders a batch's members before the batch on the leader's stream `to`.  order_after clears a member's ordering
// state; whatever happens between that and the batch's fence (an ordering failure of a later member, a failed
// launch) gives every member its state back, since its pending work is then still unordered with its own stream.
// So: no path between changing a member's ordering state and either restoring it (the destructor) or setting
// the state the batch leaves (after commit()).
class OrderGuard {
 public:
  OrderGuard(pfmpe_ctx* const* cs, int S) : cs_(cs), saved_(S) {
    for (int s = 0; s < S; ++s) saved_[s] = {cs[s]->last_stream, cs[s]->last_fence};
  }
  OrderGuard(const OrderGuard&) = delete;
  OrderGuard& operator=(const OrderGuard&) = delete;
  // members first .. S - 1 after their latest work; errors are reported on `err`
  int order(int first, hipStream_t to, pfmpe_ctx* err) {
    for (int s = first; s < (int)saved_.size(); ++s) RET(order_after(cs_[s], to, err));
    return PFMPE_OK;
  }
  void commit() { committed_ = true; }
  ~OrderGuard() {
    if (committed_) return;
    for (size_t s = 0; s < saved_.size(); ++s) {
      cs_[s]->last_stream = saved_[s].first;
      cs_[s]->last_fence = saved_[s].second;
    }
  }

 private:
  pfmpe_ctx* const* cs_;
  std::vector<std::pair<hipStream_t, std::shared_ptr<BatchFence>>> saved_;
  bool committed_ = false;
};

// The members of a blocking batch (ROI, cloud statistics, association, the streams detector): the distinct contexts in
// order of first appearance, the leader first, each with a flag "its kept propagated set is read", and the steps such
// a runner takes with them.  A member's failure is reported on the leader as "<who>: <the member's text>".
class BatchMembers {
 public:
  BatchMembers(const char* who, int n) : who_(who) {  // n: at most so many members (no growth on a per-frame call)
    cs_.reserve(n);
    flag_.reserve(n);
  }
  void add(pfmpe_ctx* c, bool flag = false) {  // before order(); a context joins once, its flag sticks
    const size_t m = std::find(cs_.begin(), cs_.end(), c) - cs_.begin();
    if (m == cs_.size()) {
      cs_.push_back(c);
      flag_.push_back(0);
    }
    if (flag) flag_[m] = 1;
  }
  // every flagged member's kept propagated set once, as its single call regenerates it: into its own d_xfer (all of
  // them allocated first), on its own stream (set_device: after whatever it has pending elsewhere), bracketed as aux
  int regen() {
    for (size_t m = 0; m < cs_.size(); ++m)
      if (flag_[m]) RET(ensure_xfer(cs_[m]));
    for (size_t m = 0; m < cs_.size(); ++m) {
      pfmpe_ctx* c = cs_[m];
      if (!flag_[m]) continue;
      if (c != cs_[0]) RET(set_device(c));
      if (const int r_ = dispatch_regen(c, c->last_kept_iter, c->d_state[c->last_prior_idx].get(), c->d_xfer.get()))
        return report(c, r_);
    }
    return PFMPE_OK;
  }
  // every member's work so far, a regeneration included, before the batch on the leader's stream (through OrderGuard)
  int order() {
    guard_.emplace(cs_.data(), (int)cs_.size());
    return guard_->order(1, cs_[0]->stream, cs_[0]);
  }
  void commit() { guard_->commit(); }  // after order(), as finish(): nothing is pending, no member needs a fence
  // the end of the call: one synchronise, so the commit, then every member's pending brackets (sampled frames' too)
  int finish() {
    if (hipStreamSynchronize(cs_[0]->stream) != hipSuccess)
      return fail(cs_[0], PFMPE_E_HIP, std::string(who_) + ": stream synchronise failed");
    commit();
    for (pfmpe_ctx* c : cs_)
      if (const int r_ = harvest_timing(c)) return report(c, r_);
    return PFMPE_OK;
  }

 private:
  int report(pfmpe_ctx* c, int rc) { return c == cs_[0] ? rc : fail(cs_[0], rc, std::string(who_) + ": " + c->err); }
  const char* who_;
  std::vector<pfmpe_ctx*> cs_;
  std::vector<char> flag_;
  std::optional<OrderGuard> guard_;
};

// Blocks per batch accepted by pfmpe_step_multi (PFMPE_E_CAP above): the size the GPU tests cover
// (tests/test_gpu_multi.py: 4 x 10M fp16 particles in one batch = 156,252 blocks; 32 x 1M in the bench).
constexpr int64_t kMultiMaxBlocks = 160000;

// The step's launch sequences for one (state type, RNG), defined in pfmpe_seq.hpp and instantiated by the
// pfmpe_k_<state>_<rng>.hip units: pfmpe_step, pfmpe_step_multi for S validated contexts, and the regeneration of a
// kept iteration's propagated set.
template <typename T, int RNG, typename SP>
int dispatch_m(pfmpe_ctx* c, const pfmpe_frame_in* in, const unsigned char* table, size_t tbytes, const GridHdr& gh);
template <typename T, int RNG, typename SP>
int multi_m(pfmpe_ctx* const* cs, int S, const pfmpe_frame_in* in);
template <typename T, int RNG, typename SP>
int regen_m(pfmpe_ctx* c, int kept_iter, const void* prior, double* out);
// the same for a device list of particle indices: particle list[i] of the kept iteration into out + 12 * i, for
// i < min(*count, limit) (list, count and out on the device; pfmpe_top_particles)
template <typename T, int RNG, typename SP>
int regen_list_m(pfmpe_ctx* c, int kept_iter, const void* prior, const int32_t* list, const uint32_t* count, int limit,
                 double* out);

}  // namespace pfmpe_impl

// dispatch_m, regen_m, regen_list_m and multi_m of one (state type, RNG): defined by a pfmpe_k_*.hip unit (EXT empty),
// declared for pfmpe_engine.hip (EXT = extern).  Used at file scope.
#define PFMPE_DECLARE_INSTANCE(T, RNG, SP, EXT)                                                                        \
  namespace pfmpe_impl {                                                                                               \
  EXT template int dispatch_m<T, RNG, SP>(pfmpe_ctx*, const pfmpe_frame_in*, const unsigned char*, size_t, const GridHdr&); \
  EXT template int regen_m<T, RNG, SP>(pfmpe_ctx*, int, const void*, double*);                                         \
  EXT template int regen_list_m<T, RNG, SP>(pfmpe_ctx*, int, const void*, const int32_t*, const uint32_t*, int, double*); \
  EXT template int multi_m<T, RNG, SP>(pfmpe_ctx* const*, int, const pfmpe_frame_in*);                                 \
  }
