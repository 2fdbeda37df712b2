// pfmpe_resample_prior.hip — a new prior of n_new particles from the members of the current one, on the device
// (pfmpe_resample_prior; the definition is in include/pfmpe.h): k_rs_gather_all (no filter, one launch), and with a
// mode filter k_cloud_assign (pf_modes.hpp), k_rs_count, k_rs_top and k_rs_gather_members; the entry point, and the
// host twins pfmpe_host_resample_source and pfmpe_host_resample_rank (pf_resample_index.hpp).  DESIGN.md §4.18.
#include "pf_modes.hpp"
#include "pf_resample_index.hpp"
#include "pf_state.hpp"
#include "pf_wave.hpp"
#include "pfmpe_ctx.hpp"
#include "pfmpe_prior.hpp"

namespace pfmpe {

// Both gathers run one lane per item over at most kRsMaxBlocks blocks (8 resident blocks on each of 256 CUs at their
// register use), grid-stride beyond.
constexpr int kRsMaxBlocks = 2048;
inline int rs_blocks(int64_t items) {
  const int64_t b = (items + kBlock - 1) / kBlock;
  return (int)(b < kRsMaxBlocks ? b : kRsMaxBlocks);
}

// One stored row to another buffer: the 12 elements as they are (fp64, fp32, or the fp16 deltas as the six 32-bit pair
// words they are stored as), no anchor and no conversion.  Lanes of consecutive k write consecutive elements of every
// plane; they read runs of consecutive (or repeated, or evenly spaced) rows.
template <typename SP>
__device__ __forceinline__ void rs_load_row(const SP* __restrict__ src, int64_t ld, int row, SP* v) {
  load_state_raw<SP>(src, ld, row, v);
}

// ---- no filter: slot k copies source particle resample_rank(k, N, n_new), read through the owner indices of a
// deferred prior.  One lane per new slot.
template <typename SP>
__global__ __launch_bounds__(kBlock) void k_rs_gather_all(const SP* __restrict__ src, int64_t src_ld,
                                                         const uint32_t* __restrict__ owner, uint32_t N,
                                                         SP* __restrict__ dst, int64_t dst_ld, uint32_t n_new) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < n_new; k += stride) {
    const uint32_t j = (uint32_t)resample_rank(k, N, n_new);
    const int row = owner ? (int)owner[j] : (int)j;
    SP v[12];
    rs_load_row<SP>(src, src_ld, row, v);
    store_state_raw<SP>(dst, dst_ld, (int)k, v);
  }
}

// ---- with a filter: the rank of a member is the number of members before it.  Blocks of kBlock particles; kRsSuper
// blocks form a super-block.  All of it integer and order-free: no atomics, every word has one writer.
constexpr int kRsSuper = 256;
__device__ __forceinline__ uint32_t wave_incl_sum_u32(uint32_t x) {
  x += (uint32_t)__builtin_amdgcn_mov_dpp((int)x, kDppRowShr1, 0xf, 0xf, true);
  x += (uint32_t)__builtin_amdgcn_mov_dpp((int)x, kDppRowShr2, 0xf, 0xf, true);
  x += (uint32_t)__builtin_amdgcn_mov_dpp((int)x, kDppRowShr4, 0xf, 0xf, true);
  x += (uint32_t)__builtin_amdgcn_mov_dpp((int)x, kDppRowShr8, 0xf, 0xf, true);
  x += dpp_u32<kDppBcast15, 0xa>(x, 0u);
  x += dpp_u32<kDppBcast31, 0xc>(x, 0u);
  return x;
}
// One workgroup per super-block.  A wave takes 64 consecutive blocks, one per trip: every lane reads four of the
// block's mode bytes as one word (mode_of is 4-byte aligned and allocated up to a multiple of 4; a byte past N is not
// counted), four ballots count the block's members, and lane i keeps block i's count.  Then the exclusive prefix over
// the super-block's 256 counts (wave scan, the waves' totals through LDS): blk_excl[b] = the members of the
// super-block before block b, super_sum[sb] = all of its members.
__global__ __launch_bounds__(kBlock) void k_rs_count(const uint8_t* __restrict__ mode_of, uint32_t N, uint32_t mode,
                                                    uint32_t nb, uint32_t* __restrict__ blk_excl,
                                                    uint32_t* __restrict__ super_sum) {
  __shared__ uint32_t wtot[kWaves];
  const uint32_t lane = (uint32_t)lane_id(), wv = (uint32_t)wave_id_u();
  const uint32_t b0 = (uint32_t)blockIdx.x * kRsSuper + wv * 64u;  // this wave's first block
  const uint32_t* __restrict__ words = (const uint32_t*)mode_of;
  uint32_t mine = 0u;
  for (uint32_t i = 0; i < 64u && b0 + i < nb; ++i) {  // wave-uniform trips
    const uint64_t p = (uint64_t)(b0 + i) * kBlock + 4u * lane;  // this lane's first particle
    const uint32_t w = p < N ? words[p >> 2] : 0u;
    uint32_t c = 0u;
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q)
      c += (uint32_t)__popcll(__ballot(p + q < N && ((w >> (8u * q)) & 0xffu) == mode));
    mine = lane == i ? c : mine;
  }
  const uint32_t incl = wave_incl_sum_u32(mine);
  if (lane == 63u) wtot[wv] = incl;
  __syncthreads();
  uint32_t pre = 0u, all = 0u;
#pragma unroll
  for (uint32_t x = 0; x < (uint32_t)kWaves; ++x) {
    pre += x < wv ? wtot[x] : 0u;
    all += wtot[x];
  }
  if (b0 + lane < nb) blk_excl[b0 + lane] = pre + incl - mine;
  if (threadIdx.x == 0) super_sum[blockIdx.x] = all;
}
// One wave: super_excl[s] = the members before super-block s, *total = all members (what the counts of
// k_cloud_assign say as well; the gather reads it here, so nothing is read back in between).
__global__ __launch_bounds__(64) void k_rs_top(const uint32_t* __restrict__ super_sum, uint32_t ns,
                                              uint32_t* __restrict__ super_excl, uint32_t* __restrict__ total) {
  const uint32_t lane = (uint32_t)lane_id();
  uint32_t carry = 0u;
  for (uint32_t s0 = 0; s0 < ns; s0 += 64u) {
    const uint32_t x = s0 + lane < ns ? super_sum[s0 + lane] : 0u;
    const uint32_t incl = wave_incl_sum_u32(x);
    if (s0 + lane < ns) super_excl[s0 + lane] = carry + incl - x;
    carry += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  }
  if (lane == 0u) *total = carry;
}
// One lane per source particle.  A member's rank r = members before its super-block + before its block + before its
// wave (LDS) + before its lane (the ballot); it owns the slots first_slot(r) .. first_slot(r + 1) - 1 of the new prior
// (pf_resample_index.hpp), a possibly empty run, and writes them itself: no search, and a non-member or a member
// without a slot costs its byte of mode_of.  Shrinking, the members with a slot write consecutive slots; growing, a
// member's run is n_new / m slots long and the lanes of a wave write that far apart in every trip.
template <typename SP>
__global__ __launch_bounds__(kBlock) void k_rs_gather_members(const SP* __restrict__ src, int64_t src_ld,
                                                             const uint32_t* __restrict__ owner,
                                                             const uint8_t* __restrict__ mode_of, uint32_t N,
                                                             uint32_t mode, uint32_t nb,
                                                             const uint32_t* __restrict__ blk_excl,
                                                             const uint32_t* __restrict__ super_excl,
                                                             const uint32_t* __restrict__ total, SP* __restrict__ dst,
                                                             int64_t dst_ld, uint32_t n_new) {
  __shared__ uint32_t wtot[kWaves];
  const uint32_t lane = (uint32_t)lane_id(), wv = (uint32_t)wave_id_u();
  const uint64_t m = *total;
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {  // block-uniform trips: ballots and barriers
    const uint64_t n = (uint64_t)b * kBlock + threadIdx.x;
    const bool member = n < N && (uint32_t)mode_of[n] == mode;
    const uint64_t ball = __ballot(member);
    if (lane == 0u) wtot[wv] = (uint32_t)__popcll(ball);
    __syncthreads();
    uint32_t pre = 0u;
#pragma unroll
    for (uint32_t x = 0; x < (uint32_t)kWaves; ++x) pre += x < wv ? wtot[x] : 0u;
    __syncthreads();  // wtot is rewritten by the next trip
    if (!member) continue;
    const uint64_t r = (uint64_t)super_excl[b / kRsSuper] + blk_excl[b] + pre +
                       (uint32_t)__popcll(ball & (((uint64_t)1 << lane) - 1u));
    const uint64_t lo = resample_first_slot(r, m, n_new), hi = resample_first_slot(r + 1u, m, n_new);
    if (lo == hi) continue;
    const int row = owner ? (int)owner[n] : (int)n;
    SP v[12];
    rs_load_row<SP>(src, src_ld, row, v);
    for (uint64_t k = lo; k < hi; ++k) store_state_raw<SP>(dst, dst_ld, (int)k, v);
  }
}

// the scratch of a filtered call for N source particles (pfmpe_ctx::d_resample), every part 256-byte aligned
struct RsLayout {
  uint32_t nb, ns;
  size_t super_sum, super_excl, blk_excl, bytes;
  static size_t align(size_t x) { return (x + 255) / 256 * 256; }
  explicit RsLayout(int64_t N) {
    nb = (uint32_t)((N + kBlock - 1) / kBlock);
    ns = (nb + kRsSuper - 1) / kRsSuper;
    super_sum = 256;  // behind the member total
    super_excl = super_sum + align((size_t)ns * sizeof(uint32_t));
    blk_excl = super_excl + align((size_t)ns * sizeof(uint32_t));
    bytes = blk_excl + align((size_t)nb * sizeof(uint32_t));
  }
};

}  // namespace pfmpe

using namespace pfmpe_impl;

extern "C" {

int pfmpe_resample_prior(pfmpe_ctx* dst, pfmpe_ctx* src, const pfmpe_resample_params* params,
                         pfmpe_resample_out* out) {
  static_assert(sizeof(pfmpe_resample_params) == 48 && sizeof(pfmpe_resample_out) == 24, "ABI");
  if (!dst) return PFMPE_E_ARG;
  if (!src || !params || !out) return fail(dst, PFMPE_E_ARG, "resample_prior: bad arguments");
  const int K = params->K;
  const int64_t n_new = params->n_new;
  if (n_new < 1) return fail(dst, PFMPE_E_ARG, "resample_prior: n_new < 1");
  if (src->device != dst->device || src->state_dtype != dst->state_dtype)
    return fail(dst, PFMPE_E_ARG, "resample_prior: device and state type of src must match dst");
  if (K < 0 || K > PFMPE_MODES_MAX) return fail(dst, PFMPE_E_ARG, "resample_prior: K outside 0..PFMPE_MODES_MAX");
  if (K > 0) {
    if (!params->seeds) return fail(dst, PFMPE_E_ARG, "resample_prior: null seeds");
    if (const char* bad = modes_args_bad(params->seeds, K, params->modes))
      return fail(dst, PFMPE_E_ARG, std::string("resample_prior: ") + bad);
    if ((params->mode < 0 || params->mode >= K) && params->mode != PFMPE_MODE_NONE)
      return fail(dst, PFMPE_E_ARG, "resample_prior: mode is neither 0..K-1 nor PFMPE_MODE_NONE");
  }
  if (n_new > dst->max_particles) return fail(dst, PFMPE_E_CAP, "resample_prior: n_new exceeds max_particles");
  if (!src->has_prior) return fail(dst, PFMPE_E_STATE, "resample_prior: no particle set");

  const int N = src->N;
  BatchMembers members("resample_prior", 2);  // dst leads: its stream, its scratch
  members.add(dst);
  members.add(src);
  RET(set_device(dst));
  const RsLayout lay(N);
  if (K > 0) {  // the scratch before any member's ordering state changes
    RET(dst->h_modes.ensure(dst, kModesCountBytes));
    const size_t bytes = kModesCountBytes + (((size_t)N + 3) & ~(size_t)3);
    RET(dst->d_modes.grow(dst, bytes, bytes));
    RET(dst->d_resample.grow(dst, lay.bytes, lay.bytes));
  }
  RET(members.order());
  const int to = 1 - dst->prior_idx;  // the state buffer dst's prior does not occupy
  const void* from = src->d_state[src->prior_idx].get();
  const uint32_t* owner = prior_owner_ptr(src);
  hipStream_t on = dst->stream;
  if (K == 0) {
    visit_state(dst, [&](auto s) {
      using SP = typename decltype(s)::SP;
      hipLaunchKernelGGL((k_rs_gather_all<SP>), dim3(rs_blocks(n_new)), dim3(kBlock), 0, on, (const SP*)from, src->ld,
                         owner, (uint32_t)N, (SP*)dst->d_state[to].get(), dst->ld, (uint32_t)n_new);
    });
  } else {
    const ModeSeeds seeds = mode_seeds(params->seeds, K, params->modes);
    uint32_t* d_count = (uint32_t*)dst->d_modes.get();
    uint8_t* mode_of = dst->d_modes.get() + kModesCountBytes;
    unsigned char* scr = dst->d_resample.get();
    uint32_t* total = (uint32_t*)scr;
    uint32_t* super_sum = (uint32_t*)(scr + lay.super_sum);
    uint32_t* super_excl = (uint32_t*)(scr + lay.super_excl);
    uint32_t* blk_excl = (uint32_t*)(scr + lay.blk_excl);
    CloudDesc d{};  // src's prior as pfmpe_cloud_modes' POSTERIOR entry names it
    std::memcpy(d.a.anchor, src->anchor[src->prior_idx], sizeof(d.a.anchor));
    d.a.N = N;
    d.a.ld = src->ld;
    d.a.owner = owner;
    d.st = from;
    HIPCHK(dst, hipMemsetAsync(d_count, 0, kModesCountBytes, on));
    visit_state(dst, [&](auto s) {
      using T = typename decltype(s)::T;
      using SP = typename decltype(s)::SP;
      hipLaunchKernelGGL((k_cloud_assign<T, SP>), dim3(cloud_blocks(N)), dim3(kBlock), 0, on, d, seeds, mode_of, d_count);
      hipLaunchKernelGGL(k_rs_count, dim3(lay.ns), dim3(kBlock), 0, on, (const uint8_t*)mode_of, (uint32_t)N,
                         (uint32_t)params->mode, lay.nb, blk_excl, super_sum);
      hipLaunchKernelGGL(k_rs_top, dim3(1), dim3(64), 0, on, (const uint32_t*)super_sum, lay.ns, super_excl, total);
      hipLaunchKernelGGL((k_rs_gather_members<SP>), dim3(rs_blocks(N)), dim3(kBlock), 0, on, (const SP*)from, src->ld,
                         owner, (const uint8_t*)mode_of, (uint32_t)N, (uint32_t)params->mode, lay.nb,
                         (const uint32_t*)blk_excl, (const uint32_t*)super_excl, (const uint32_t*)total,
                         (SP*)dst->d_state[to].get(), dst->ld, (uint32_t)n_new);
    });
    HIPCHK(dst, hipMemcpyAsync(dst->h_modes.get(), d_count, (size_t)(K + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, on));
  }
  HIPCHK(dst, hipGetLastError());
  // the hand-off state as import_enqueue zeroes it for a new prior's first frame (it is zero between frames: with no
  // member this changes nothing)
  HIPCHK(dst, hipMemsetAsync(dst->d_ctrl.get(), 0, sizeof(Ctrl), on));
  HIPCHK(dst, hipMemsetAsync(dst->d_winkey.get(), 0, kWinBytes, on));
  HIPCHK(dst, hipMemsetAsync(dst->d_counters.get(), 0, counters_bytes(dst), on));
  RET(members.finish());
  int64_t m = N;
  if (K > 0) m = ((const uint32_t*)dst->h_modes.get())[params->mode == PFMPE_MODE_NONE ? K : params->mode];
  out->n_src = N;
  out->n_members = m;
  out->n_new = m > 0 ? n_new : 0;
  if (m == 0) return PFMPE_OK;  // nothing was written: dst is as it was
  std::memcpy(dst->anchor[to], src->anchor[src->prior_idx], sizeof(dst->anchor[to]));
  dst->prior_idx = to;
  dst->prior_owner = -1;
  import_done(dst, (int)n_new);
  return PFMPE_OK;
}

int pfmpe_host_resample_source(const uint8_t* mode_of, int64_t N, int32_t mode, int64_t n_new, int32_t* source,
                               int64_t* n_members) {
  if ((!source && n_new > 0) || !n_members || N < 0 || n_new < 0 || N > kResampleMaxCount || n_new > kResampleMaxCount ||
      (mode_of && (mode < 0 || mode > 255)))
    return PFMPE_E_ARG;
  resample_source(mode_of, N, mode, n_new, source, n_members);
  return PFMPE_OK;
}

int pfmpe_host_resample_rank(int64_t k, int64_t m, int64_t n_new, int64_t* rank) {
  if (!rank || m < 1 || n_new < 1 || k < 0 || k >= n_new || m > kResampleMaxCount || n_new > kResampleMaxCount)
    return PFMPE_E_ARG;
  *rank = (int64_t)resample_rank((uint64_t)k, (uint64_t)m, (uint64_t)n_new);
  return PFMPE_OK;
}

}  // extern "C"
