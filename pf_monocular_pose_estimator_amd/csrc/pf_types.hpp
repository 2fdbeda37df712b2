// pf_types.hpp — constants, kernel arguments and the records that cross launches or reach the host: what every
// unit of the library may see (no kernel, no device helper).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pfmpe {

constexpr int kBlock = 256;            // particles per block (4 waves)
constexpr int kWaves = kBlock / 64;
// Blocks per reduction group: ~sqrt(blocks), at most kGroup (one per lane of the group wave).  Arrival
// counters are agent-scope atomics that execute at the memory side and serialise per address (~25 ns
// each), so sqrt balances the group counters against the top counter (a single 391-way counter cost
// ~10 us at C2).  A grid of one group skips the top counter: its group wave is the top wave.
constexpr int kGroup = 64;
constexpr int kMaxMarkers = 16;
constexpr int kMaxBlobs = 1024;
constexpr int kMaxBuckets = 512;       // x-buckets of the blob table (see bucket_count)
constexpr int kMaxIter = 4096;         // PF iterations per frame (reference: 80); < 2^16 for k_frame's release tags
constexpr int kPlanes = 12;            // r00 r01 r02 t0 r10 r11 r12 t1 r20 r21 r22 t2

enum : int { kRngReference = 0, kRngPhilox = 1 };

// Marker-count buckets (pfmpe_ctx.hpp visit_m): the per-particle loops are unrolled to MAXM slots.
// The 5-slot bucket serves exactly M == 5 (the README object: C1, C2, C4, C5), so its "slot j holds a marker"
// tests are compile-time true: no per-marker lane masks live across the streaming loops (they held SGPR pairs
// spilled to VGPR lanes, a v_readlane pair per use).  The other buckets test j < M.
constexpr int kExactM = 5;
template <int MAXM>
__host__ __device__ __forceinline__ bool marker_live(int j, int M) {
  return MAXM == kExactM ? j < kExactM : j < M;
}

// ----------------------------------------------------------------------------- kernel arguments
// Passed by value (kernarg segment -> scalar loads), pre-converted to the compute type T on the host.
// The frame's 2D blob grid as kernel arguments (scalar registers, reloadable from the kernarg segment /
// stream descriptor instead of held in VGPRs): build_blob_table_host's GridHdr plus the byte offsets of the
// grid's parts in the table; on = 0 when the table has no grid or one built for a narrower window.
// one 2D-grid list entry of a blob table (build_blob_table_host): position and original index, one ds_read_b128
struct alignas(16) GridEnt {
  float x, y;
  int32_t orig, pad;
};
struct GridArgs {
  float inv_c, ox, oy, pad0;       // cell of (u, v): (fma(u, inv_c, ox), fma(v, inv_c, oy)), clamped, truncated;
                                   // ox = -gx0 * inv_c (square cells)
  float fmaxx, fmaxy;              // ncx - 1, ncy - 1
  int32_t ncx4, on;               // 4 * ncx: the cell row pitch in bytes
  int32_t cell_off, ent_off;      // table offsets: uint32 cell[], GridEnt ent[]
  int32_t b0fin;                  // blob 0 of the table is finite (set whether or not the grid is on)
  int32_t pad2;
};

template <typename T>
struct FrameArgsT {
  T cur[12], pred[12], predm[12], cam[12];  // 3x4 row-major
  T markers[kMaxMarkers * 3];
  T K[9];
  T lo[6], hi[6];           // draw ranges angX angY angZ tX tY tZ (scaled by fac*), Philox stream
  T rgs[6];                 // (hi - lo) * 2^-21: hi - lo rounded once on the host, then scaled exactly (Philox draw
                            // lo + u21 * (hi - lo) with u21 = v * 2^-21, computed as v * rgs: the same product)
  double dlo[6], dhi[6];    // the same in double, reference stream (draws are computed in double)
  double growth;            // 0.025
  T tol, tol_pf, tolq;      // score normaliser / acceptance gate / pruning half-window
  double exit_thr, accept_thr;
  uint32_t key0, key1, flo, fhi;  // philox key / frame counter
  uint32_t lcg_x0;                // reference engine state after seeding
  uint32_t downgrade;             // bit j: marker j downgraded
  int32_t N, M, B, it;            // particles, markers, blobs, it_since_initialized_
  int32_t cam_identity, max_iter, force_iters, nblk;
  int32_t ngrp, gsz;              // reduction groups and blocks per group (~sqrt(nblk), <= kGroup)
  int32_t diag;                   // diagnostic switches (0 in production; kDiag* below)
  int32_t small_angles;           // every angle draw of the frame has |x| <= kSmallAngle (host bound, fp32)
  int32_t k_upper;                // K = [k0 k1 k2; 0 k4 k5; 0 0 1] (host check; fp32 skips the zero terms)
  uint32_t wait_ticks;            // bound of every in-launch wait, s_memrealtime ticks (100 MHz)
  uint32_t flat_base_w, flat_base_c;  // k_frame2: running totals of the flat counter sets at frame start
  int32_t tbytes;                 // this frame's blob table, bytes (base + grid: build_blob_table_host)
  uint32_t gtag;                  // k_frame2: this frame's granule tag base (frame << 12; the iteration in the low
                                  // 12 bits), never 0 (pfmpe_seq.hpp next_gtag)
  GridArgs grid;                  // the table's 2D grid (fp32 pruned column minima)
  int64_t ld;                     // SoA plane stride in elements
  T anc_in[12], anc_out[12];      // fp16 state only: anchors of the prior / of the new prior
  // Deferred resampling: the prior may be stored as an earlier frame's kept propagated set plus
  // owner indices, prior particle n = stored particle owner[n] (null: stored in particle order).  owner_out
  // (two-launch frames with the kept set): k_resample writes the new prior's owner indices there instead of
  // gathering and scattering the particles (null: the new prior is materialised in the post buffer).
  const uint32_t* owner;
  uint32_t* owner_out;
};

// The frame-constant arrays, staged once per block into LDS and read from there (broadcast reads):
// kept in SGPRs they would spill into VGPR lanes and cap residency (MI355X_MICROARCH.md "Residency").
template <typename T>
struct LdsConst {
  T cur[12], pred[12], predm[12], cam[12];
  T markers[kMaxMarkers * 3];
  T K[9];
  T lo[6], hi[6];
  T rgs[6];
};

// Per-frame control record.  All-zero is the valid "start of frame" state (zeroed at create, set_prior
// and by the final wave of every frame).
struct Ctrl {
  double best_max;   // highestProb
  double S;          // probPartSum of the kept iteration
  double invS;       // fl(1 / S): k_resample's divisions by S as a product and two fma corrections (div_by_S)
  int32_t done, has_best, best_idx, best_iter, best_slot, cur_slot;
  int32_t iters, kept_slot, kept_iter, accepted, most_likely_idx, pad0;
  int64_t K_total;   // number of stratified targets that find a particle
};

// per block, per weight slot (written and read write-through)
struct alignas(16) BlockPart {
  double sum;             // block total (in-block scan order)
  double maxrel, minrel;  // extrema of the in-block inclusive prefix sums
  double maxw, minw;      // max / min weight
  int32_t argmax, argmin;
};
// per group, per weight slot (write-through)
struct alignas(16) GroupPart {
  double sum;          // group total
  double zmax, zmin;   // max / min over the group of fl(E_b + incl_i)
  double maxw, minw;
  int32_t argmax, argmin;
};
// per block, per weight slot: in-group exclusive prefix E_b and exclusive max/min of z (for k_resample)
struct alignas(16) BlockScan {
  double E, zin_max, zin_min, pad;
};
// per group, kept slot only: group prefix G_g and running max of c at the group start
struct alignas(16) GroupScan {
  double G, Gin;
};
struct alignas(8) CountPart {
  int32_t maxcount, idx;
};
// winner keys of the one-stream two-launch frame (k_resample -> k_resample_final): unsigned max of
// count << 32 | (2^31 - 1 - index) is the max count at its lowest index; 0 (count 0 at no index) is the identity
constexpr int kWinShards = 64;
constexpr int kWinStride = 16;  // keys one 128-B line apart: ~39k block atomics at C4 spread over 64 lines
// the key area: the key shards, then as many arrival shards of the fused finish (k_resample_owners), each counter at
// the start of its own 128-B line (one memory-side atomic unit serialises ~25 ns per arrival on one address: one
// counter for C4's 39k blocks took 400 us)
constexpr size_t kWinBytes = (size_t)(2 * kWinShards) * kWinStride * sizeof(unsigned long long);
__host__ __device__ __forceinline__ uint32_t* win_arrive(unsigned long long* winkey) {
  return (uint32_t*)(winkey + kWinShards * kWinStride);
}
constexpr int kArriveStride = 2 * kWinStride;  // uint32 words between arrival shards (128 B)
__host__ __device__ __forceinline__ unsigned long long win_key(int count, int idx) {
  return ((unsigned long long)(uint32_t)count << 32) | (uint32_t)(0x7fffffff - idx);
}

// frame record written by the final wave into pinned host memory: the pfmpe_frame_out layout, then the
// kept slot and the publication tag (2 * frame sequence + finished)
struct OutDev {
  int32_t iters, kept_iter, most_likely_idx, accepted, resampled, winner_idx, n_corr, flag_fail;
  double highest_prob, prob_sum;
  double winner_pose[12], most_likely_pose[12];
  uint32_t corr[2 * kMaxMarkers];
  int32_t kept_slot;
  int32_t tag;
};
// The record as the kernel publishes it: data-tagged granules (MI355X_MICROARCH.md "handoff-1to1"), 8-byte
// words {OutDev word k (low 32 bits), tag (high 32)}, each ONE relaxed system-scope store, so the host has
// the whole record once every granule carries the current tag, and the final wave needs no release (no
// wait for the PCIe write acknowledgements).  An unfinished iteration batch (two-launch path) writes
// granule 0 alone, with tag 2 * seq.
constexpr int kRecWords = (int)(offsetof(OutDev, tag) / 4);
constexpr int kRecGran = 128;
static_assert(offsetof(OutDev, tag) % 4 == 0 && kRecWords <= kRecGran && kRecWords > 64, "record granules");
struct RecOut {
  uint64_t g[kRecGran];
};

// Diagnostic stamps (fa.diag & 4 only): s_memrealtime (100 MHz).  0/4 first block start of K1/K2 (min),
// 1/5 last block partial (max), 2-3 / 6-7 top wave start/end, 8 table built, 9 weights done, 10 K2 scan
// done, 11 counts done, 12 scatter done, 13-18 finalize phases, 19 earliest table built (min).
constexpr int kStamps = 32;
// diagnostic switches (FrameArgsT::diag, pfmpe_set_option(ctx, 99, bits)); 0 in production
enum : int {
  kDiagStamps = 4,      // phase stamps (s_memrealtime) into d_stamps
  kDiagVisits = 8,      // pruned-candidate counts into d_stamps
  kDiagTreeCount = 16,  // k_frame: count barrier as a tree instead of flat
  kDiagSqrtGroups = 32, // groups of ~sqrt(nblk) blocks even when the frame fits k_frame2
  kDiagLagLoads = 64,   // k_frame2: the last block sleeps ~20 us before loading the block partials
  kDiagAbandon = 128,   // k_frame2: every block gives up its first weighing-barrier wait (recovery test)
  kDiagSortedScore = 256, // fp32: the sorted (extraction-order) score even when B >= M (A/B of score_unordered)
  kDiagNoStream = 512,     // two-launch path: never the streaming weighing pass (k_weigh_stream + k_group + k_top)
  kDiagForceStream = 1024, // two-launch path: always the streaming weighing pass (tests / A/B)
  kDiagSerialTop = 2048,   // streaming pass with > 64 groups: the one-wave k_top instead of k_top_wide (A/B)
  kDiagNoPk = 4096,        // two-launch path: never the two-particles-per-lane pass k_weigh_pk (A/B, tests)
  kDiagCorruptDesc = 8192, // pfmpe_step_multi: the first stream's descriptor is altered after its tag (test of the
                           // staging check; the altered word is a key word, never a pointer)
  kDiagNoDefer = 16384,    // two-launch frames materialise the new prior even with the kept set (A/B of deferral)
  kDiagMinSide = 65536,      // k_frame2: run the zmin scans (group_zmin2) even when no weight can be negative (tests)
  kDiagAbandonFinish = 131072,  // k_resample_owners(_multi): the finishing wave gives up before polling the arrivals
                                // (the two-launch recovery tests)
  kDiagBlockResample = 32768, // deferred two-launch frames resample with the block-per-256 k_resample instead of
                              // k_resample_owners' wave per 256 (A/B, identity tests)
  kDiagAssocDirect = 262144,  // pfmpe_assoc_stats: every vote straight into the device table even when the bins fit
                              // in LDS (tests: both voting paths on one input)
  kDiagDetCopy = 524288,      // pfmpe_find_leds_streams: the crops go up by one async copy command instead of the
                              // pull kernel k_detm_pull (A/B)
  kDiagTailMiss = 1 << 20     // pfmpe_step_refine(_multi): the tail reports "record not ready" (the recovery test)
};

// flat hand-off (k_frame2, pf_kernels.hpp): the sizes of its sharded arrival counters
constexpr int kShards = 8;
constexpr int kShardStride = 32;                         // uint32 words: 128 B
constexpr int kFlatCountSet = kShards * kShardStride;    // offset of set 1
constexpr int kFlatWords = 2 * kShards * kShardStride;
constexpr int kFlatMaxGroups = 8;                        // k_frame2: <= 512 blocks in groups of 64

// The flat path's area: the two parities of block partials (BlockPart, k_frame2's weighing barrier), then the count
// granules {count, index} of up to kFlatMaxGroups * kGroup blocks.
constexpr size_t kGranPartBytes = (size_t)kFlatMaxGroups * kGroup * sizeof(BlockPart);  // per parity
constexpr size_t kGranCountOff = 2 * kGranPartBytes;
constexpr size_t kGranBytes = kGranCountOff + (size_t)kFlatMaxGroups * kGroup * 16;

// the grid part of a blob table (pf_likelihood.hpp), kept by the host per staged frame
__host__ __device__ constexpr size_t align16(size_t x) { return (x + 15) / 16 * 16; }
struct GridHdr {
  float inv_c, gx0, gy0, pad0;     // cell of (u, v): ((u - gx0) * inv_c, (v - gy0) * inv_c), clamped
  float fmaxx, fmaxy;              // ncx - 1, ncy - 1
  float gtolq;                     // half-window the lists were built for (>= the frame's tolq to be used)
  int32_t ncx, ncell, nent;        // columns, cells, list entries
  int32_t b0fin, pad;              // blob 0 finite (every table, grid or not)
};
static_assert(sizeof(GridHdr) == 48, "grid header");

// Winner candidate of one block: the block's first max-count particle, its kept pose and its
// correspondences, published by the block's wave 1 (in parallel with wave 0's arrival) as data-tagged
// granules: 8-byte words {payload (low 32 bits), frame sequence (high 32)}, each written by ONE
// write-through store, so a reader that sees every tag current has every payload (MI355X_MICROARCH.md
// "handoff-1to1").  Granules 0-23: the 12 pose doubles as lo/hi halves; 24-55: the 32 corr words;
// 56: n_corr.  The global winner is one of these, so the final wave loads one block's granules.
constexpr int kCandGran = 57;
struct alignas(16) Cand {
  uint64_t g[64];
};

// the arguments of k_assoc_votes (pfmpe_assoc.hip; the launch is declared in pfmpe_ctx.hpp)
struct AssocArgs {
  const double* dense;   // DENSE: N x 12 poses (the regenerated kept set)
  uint32_t* votes;       // votes mode: M x B bins (LED m + 1 with blob b + 1 at m * B + b), then the M + 1 bins of the
                         // pair count; null: rows mode
  uint32_t* corr;        // rows mode: 2 * kMaxMarkers words per particle of the range (16-byte aligned)
  int32_t* n_corr;       // rows mode: its pair count
  int32_t first, count;  // the particles first .. first + count - 1
  int32_t lds_votes;     // votes mode: the block's bins in LDS behind the blob table, flushed once per block; 0: every
                         // vote straight into `votes` (the bins do not fit beside the table)
  int32_t pad;
};
// a block per 256 particles up to 1024 blocks (as cloud_blocks), grid-stride beyond
constexpr int kAssocMaxBlocks = 1024;
// the workgroup's LDS: the blob table, the bins and the frame constants must fit
constexpr size_t kAssocLdsLimit = 64 * 1024;
__host__ __device__ inline int assoc_bins(int M, int B) { return M * B + M + 1; }

}  // namespace pfmpe
