// pf_likelihood.hpp — projection, the blob table (host builder, LDS view, 2D grid) and the likelihood of one
// particle (PE:1017, PE:2385).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "pf_state.hpp"
#include "pf_wave.hpp"

namespace pfmpe {

template <typename T>
__device__ __forceinline__ void k_times_pose(const LdsConst<T>& sc, const T* P, bool k_upper, T* Q) {
  if (std::is_same<T, float>::value && k_upper) {
#pragma unroll
    for (int j = 0; j < 4; j += 2) {  // columns j, j + 1 as one pair
      const f32x2 p0 = pk2(P[0 * 4 + j], P[0 * 4 + j + 1]);
      const f32x2 p1 = pk2(P[1 * 4 + j], P[1 * 4 + j + 1]);
      const f32x2 p2 = pk2(P[2 * 4 + j], P[2 * 4 + j + 1]);
      f32x2 s = p0 * sc.K[0];
      s = pk_fma(pk2(sc.K[1], sc.K[1]), p1, s);
      s = pk_fma(pk2(sc.K[2], sc.K[2]), p2, s);
      const f32x2 s1 = pk_fma(pk2(sc.K[5], sc.K[5]), p2, p1 * sc.K[4]);
      Q[0 * 4 + j] = s.x;
      Q[0 * 4 + j + 1] = s.y;
      Q[1 * 4 + j] = s1.x;
      Q[1 * 4 + j + 1] = s1.y;
      Q[2 * 4 + j] = P[2 * 4 + j];
      Q[2 * 4 + j + 1] = P[2 * 4 + j + 1];
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      T s = sc.K[i * 3 + 0] * P[0 * 4 + j];
      s = fmadd(sc.K[i * 3 + 1], P[1 * 4 + j], s);
      s = fmadd(sc.K[i * 3 + 2], P[2 * 4 + j], s);
      Q[i * 4 + j] = s;
    }
  }
}

// project2d (PE:1017-1034): p = (K34*T) * [X;1], u = p/p.z — full K, no distortion, no z>0 test
template <typename T, int MAXM>
__device__ __forceinline__ void project_markers(const FrameArgsT<T>& fa, const LdsConst<T>& sc, const T* P, T* u,
                                                T* v) {
  T Q[12];
  k_times_pose<T>(sc, P, fa.k_upper != 0, Q);
  if constexpr (std::is_same<T, float>::value) {  // rows 0 and 1 as one packed pair, same operations
    // every slot up to MAXM is projected (markers past M are zeros, their u / v never read): no branch, so the
    // u / v arrays stay in registers (a conditional store per slot had put them in scratch)
    const f32x2 q0 = pk2(Q[0], Q[4]), q1 = pk2(Q[1], Q[5]), q2 = pk2(Q[2], Q[6]), q3 = pk2(Q[3], Q[7]);
#pragma unroll
    for (int j = 0; j < MAXM; ++j) {
      const float X = sc.markers[3 * j], Y = sc.markers[3 * j + 1], Z = sc.markers[3 * j + 2];
      f32x2 s = q0 * X;
      s = pk_fma(q1, pk2(Y, Y), s);
      s = pk_fma(q2, pk2(Z, Z), s);
      s = s + q3;
      float z = Q[8] * X;
      z = fmadd(Q[9], Y, z);
      z = fmadd(Q[10], Z, z);
      z = z + Q[11];
      const f32x2 uv = s * rcp_t(z);  // persp(): p0 * rcp(p2), p1 * rcp(p2)
      u[j] = uv.x;
      v[j] = uv.y;
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < MAXM; ++j) {
    if (marker_live<MAXM>(j, fa.M)) {
      const T X = sc.markers[3 * j], Y = sc.markers[3 * j + 1], Z = sc.markers[3 * j + 2];
      T p[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        T s = Q[i * 4 + 0] * X;
        s = fmadd(Q[i * 4 + 1], Y, s);
        s = fmadd(Q[i * 4 + 2], Z, s);
        p[i] = s + Q[i * 4 + 3];
      }
      persp(p[0], p[1], p[2], &u[j], &v[j]);
    } else {
      u[j] = v[j] = (T)0;
    }
  }
}

// project_markers' arithmetic for ONE marker j (wave-uniform index): the same operation order, so the
// same bits
template <typename T>
__device__ __forceinline__ void project_one(const LdsConst<T>& sc, const T* P, int j, bool k_upper, T& u, T& v) {
  T Q[12];
  k_times_pose<T>(sc, P, k_upper, Q);
  const T X = sc.markers[3 * j], Y = sc.markers[3 * j + 1], Z = sc.markers[3 * j + 2];
  T p[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    T s = Q[i * 4 + 0] * X;
    s = fmadd(Q[i * 4 + 1], Y, s);
    s = fmadd(Q[i * 4 + 2], Z, s);
    p[i] = s + Q[i * 4 + 3];
  }
  persp(p[0], p[1], p[2], &u, &v);
}

// x-buckets per frame: 2 per blob rounded up to a power of two, in [128, kMaxBuckets] — narrow enough
// that the +-tolq window stays close to its own width when B is large (C3: 200 blobs, 1.5 px buckets)
__host__ __device__ __forceinline__ constexpr int bucket_count(int B) {
  int nb = 128;
  while (nb < kMaxBuckets && nb < 2 * B) nb *= 2;
  return nb;
}
// x -> bucket index (monotone in x; identical formula for table build and queries)
template <typename T>
__host__ __device__ __forceinline__ int bucket_of(T x, T xmin, T inv_bw, int nb) {
  const T f = (x - xmin) * inv_bw;
  if (!(f >= (T)0)) return 0;
  if (f >= (T)(nb - 1)) return nb - 1;
  return (int)f;
}
template <typename T>
struct alignas(2 * sizeof(T)) BlobXY {
  T x, y;
};

// calculateEstimationProbability (PE:2385-2445) in its closed form.  Step 1: per marker the first-minimum
// blob over all blobs (column minimum of the B x M distance matrix; ties -> lowest blob index).
// Step 2 (score_minima): extraction in ascending (distance, marker) order — the order Eigen's minCoeff
// visitor finds them — with the same gate (tol_PF), score ((tol-d)/tol)^2 with tol NOT tol_PF,
// self-occlusion (3*s) and downgrade (2) penalties, capped at min(B, M) pairs.
//
// Exact pruning (DESIGN.md "Exact blob pruning"): only blobs in the x-buckets overlapping the window
// |bx-u| <= tolq (tolq >= tol_PF plus rounding slack) are visited.  Every blob within tol_PF lies in the
// window, and a marker whose true minimum lies outside it fails the gate anyway, so accepted pairs,
// penalties and the weight are unchanged; rejected markers only change their (unused) distance value.
// fp32 tables also carry a 2D cell grid (build_blob_table_host): a marker's candidates are then ONE cell's
// list (a 2D window instead of an x-strip), walked by column_minima's grid branch.
template <typename T>
struct LdsBlobs;

// bucket_of without branches (fp32 kernels): max(f, 0) maps NaN and negatives to 0 (v_max_f32 returns the
// non-NaN operand), min(., nb-1) clamps; the same bucket as bucket_of for every input
__device__ __forceinline__ int bucket_of_bf(float x, float xmin, float inv_bw, int nb) {
  const float f = (x - xmin) * inv_bw;
  return (int)__builtin_fminf(__builtin_fmaxf(f, 0.0f), (float)(nb - 1));
}

// PHASED (k_frame2, whose VGPR budget holds every marker's cell record): the grid branch in phases over the
// markers; the register-capped streaming kernels keep the per-marker form (the phases spill there)
template <typename T, int MAXM, bool PRUNE, bool PHASED = false>
__device__ __forceinline__ int column_minima(const FrameArgsT<T>& fa, const T* u, const T* v,
                                             const LdsBlobs<T>& tb, T* m, int* r) {
  const int B = fa.B, M = fa.M;
  int visited = 0;
  if constexpr (std::is_same<T, float>::value) {
    // fp32: branch-free visits on ONE 64-bit key per candidate, {distance bits : original index}.  Distances
    // are sums of squares (>= +0 or NaN), whose IEEE bits order like the values, and every NaN's bits lie
    // above +inf's, so "key < best key" is exactly "strictly closer, or equally close with a lower original
    // index" (the general form's tie rule) and a NaN distance is never taken.  A minimum that stays +inf keeps
    // r = 0 (the general form's bc < 0 case); it fails the gate anyway.  Candidates go two per step, the
    // second masked past the window end (its LDS reads stay inside the padded table, kTablePad).
    // The query buckets: f = (u - (xmin -+ tolq)) * inv_bw, clamped by one med3 (NaN -> bucket 0 or any
    // in-range bucket: a NaN projection never takes a candidate).  The two roundings of xmin -+ tolq and
    // u - base are each within half an ulp of a pixel coordinate, like bucket_of's own, far inside tolq's
    // slack (1e-3 px + 0.1 %): the window still holds every blob within tol_PF.
    // The 2D grid (when the table has one built for at least this frame's window): the candidates of marker j
    // are the one cell list its projection falls in (build_blob_table_host proves every blob within tol_PF is
    // listed there); ~1 candidate per marker instead of an x-strip's ~2, so the wave's candidate walk is
    // usually a single step.  Otherwise the x-buckets.
    const GridArgs& ga = fa.grid;
    if (PRUNE && ga.on) {  // wave-uniform (host: the table's grid covers this frame's window)
      // Grid walk: one cell list per marker (~1 candidate).  Its entries are in increasing original index, so
      // a strict "closer" test keeps the first (lowest-index) of equally close blobs, the key order above,
      // and a NaN distance is never taken.  The list's first entry (the +inf sentinel for an empty cell) is
      // taken without a test: bd = min(d, +inf) maps a NaN distance to +inf, and an empty cell leaves r = 0.
      // Further entries are walked only when some lane's cell lists more than one blob (wave-uniform branch;
      // the particles of a wave project each marker into one or two neighbouring cells, so it is rare).
      // A non-finite first distance leaves r at that entry's index instead of 0: r is read only for a finite
      // minimum within tol_PF (the gate), so no weight, pair or record changes.
      const unsigned char* cells = tb.base + ga.cell_off;
      const unsigned char* ents = tb.base + ga.ent_off;
      const f32x2 ic = pk2(ga.inv_c, ga.inv_c), oc = pk2(ga.ox, ga.oy);
      if constexpr (PHASED) {
        // In phases over the markers (every cell record, then every first entry, then the longer lists behind
        // one wave-uniform test): a per-marker branch kept each marker's two dependent LDS round trips from
        // overlapping the next marker's, and at C2 (1.5 waves per SIMD) nothing else hides them
        uint32_t rec[MAXM];
  #pragma unroll
        for (int j = 0; j < MAXM; ++j) {
          rec[j] = 0;
          if (marker_live<MAXM>(j, M)) {
            const f32x2 f = pk_fma(pk2(u[j], v[j]), ic, oc);  // both cell coordinates in one v_pk_fma_f32
            const int cx = (int)__builtin_amdgcn_fmed3f(f.x, 0.0f, ga.fmaxx);
            const int cy = (int)__builtin_amdgcn_fmed3f(f.y, 0.0f, ga.fmaxy);
            // byte offset cy * 4 ncx + 4 cx (the row pitch scaled on the host)
            rec[j] = *(const uint32_t*)(cells + mad24(cy, ga.ncx4, cx << 2));
          }
        }
        // The 12 / 16-marker buckets (C3: 200 blobs, clustered, most lists longer than one) read the first two
        // entries together; the exact 5-marker bucket (50 blobs) reads one and walks further entries only when
        // some lane of the wave needs them.
        constexpr int c1 = MAXM > kExactM ? 2 : 1;
        bool more = false;  // some live marker's list has more than c1 entries
  #pragma unroll
        for (int j = 0; j < MAXM; ++j) {
          float bd = INFINITY;
          int bo = 0;
          if (marker_live<MAXM>(j, M)) {
            const f32x2 uvj = pk2(u[j], v[j]);
            const GridEnt* e = (const GridEnt*)(ents + (rec[j] & 0xffffu));
            const int n = (int)(rec[j] >> 16);
            visited += n;
            more |= n > c1;
            const GridEnt e0 = e[0];
            const f32x2 dd = pk2(e0.x, e0.y) - uvj;  // (dx, dy) in one v_pk_add_f32
            bd = __builtin_fminf(fmadd(dd.x, dd.x, dd.y * dd.y), INFINITY);
            bo = e0.orig;
            if constexpr (c1 == 2) {
              const GridEnt e1 = e[1];
              const f32x2 d1 = pk2(e1.x, e1.y) - uvj;
              const float d = fmadd(d1.x, d1.x, d1.y * d1.y);
              const bool take = (n > 1) & (d < bd);
              bd = take ? d : bd;
              bo = take ? e1.orig : bo;
            }
          }
          m[j] = bd;
          r[j] = bo;
        }
        if (__builtin_amdgcn_ballot_w64(more)) {  // rare at 50 blobs
  #pragma unroll
          for (int j = 0; j < MAXM; ++j) {
            if (!marker_live<MAXM>(j, M)) continue;
            const int n = (int)(rec[j] >> 16);
            if (!__builtin_amdgcn_ballot_w64(n > c1)) continue;
            const f32x2 uvj = pk2(u[j], v[j]);
            const GridEnt* e = (const GridEnt*)(ents + (rec[j] & 0xffffu));
            float bd = m[j];
            int bo = r[j];
            auto visit = [&](const GridEnt& ec, bool in) {
              const f32x2 dd = pk2(ec.x, ec.y) - uvj;
              const float d = fmadd(dd.x, dd.x, dd.y * dd.y);
              const bool take = in & (d < bd);
              bd = take ? d : bd;
              bo = take ? ec.orig : bo;
            };
            // two entries per step, the second masked past the list end (its LDS read stays inside the table
            // or its 16-B tail granule, BlobTable::lds_bytes)
  #pragma unroll 2
            for (int c = c1; c < n; c += 2) {
              const GridEnt ea = e[c], eb = e[c + 1];
              visit(ea, true);
              visit(eb, c + 1 < n);
            }
            m[j] = bd;
            r[j] = bo;
          }
        }
      } else {
  #pragma unroll
        for (int j = 0; j < MAXM; ++j) {
          float bd = INFINITY;
          int bo = 0;
          if (marker_live<MAXM>(j, M)) {
            const f32x2 uvj = pk2(u[j], v[j]);
            const f32x2 f = pk_fma(uvj, ic, oc);  // both cell coordinates in one v_pk_fma_f32
            const int cx = (int)__builtin_amdgcn_fmed3f(f.x, 0.0f, ga.fmaxx);
            const int cy = (int)__builtin_amdgcn_fmed3f(f.y, 0.0f, ga.fmaxy);
            // byte offset cy * 4 ncx + 4 cx (the row pitch scaled on the host)
            const uint32_t rec = *(const uint32_t*)(cells + mad24(cy, ga.ncx4, cx << 2));
            const GridEnt* e = (const GridEnt*)(ents + (rec & 0xffffu));
            const int n = (int)(rec >> 16);
            visited += n;
            auto visit = [&](const GridEnt& ec, bool in) {
              const f32x2 dd = pk2(ec.x, ec.y) - uvj;
              const float d = fmadd(dd.x, dd.x, dd.y * dd.y);
              const bool take = in & (d < bd);
              bd = take ? d : bd;
              bo = take ? ec.orig : bo;
            };
            // The 12 / 16-marker buckets (C3: 200 blobs, clustered, most lists longer than one) read the first
            // two entries together; the exact 5-marker bucket (50 blobs) reads one and walks further entries only
            // when some lane of the wave needs them.
            constexpr int c1 = MAXM > kExactM ? 2 : 1;
            {
              const GridEnt e0 = e[0];
              const f32x2 dd = pk2(e0.x, e0.y) - uvj;  // (dx, dy) in one v_pk_add_f32
              bd = __builtin_fminf(fmadd(dd.x, dd.x, dd.y * dd.y), INFINITY);
              bo = e0.orig;
              if constexpr (c1 == 2) visit(e[1], n > 1);
            }
            if (__builtin_amdgcn_ballot_w64(n > c1)) {  // some lane's list has more entries (rare at 50 blobs)
              // two entries per step, the second masked past the list end (its LDS read stays inside the table
              // or its 16-B tail granule, BlobTable::lds_bytes)
  #pragma unroll 2
              for (int c = c1; c < n; c += 2) {
                const GridEnt ea = e[c], eb = e[c + 1];
                visit(ea, true);
                visit(eb, c + 1 < n);
              }
            }
          }
          m[j] = bd;
          r[j] = bo;
        }
      }
      return visited;
    }
    const float fmaxb = (float)(tb.nb - 1);
    const float base_lo = tb.xmin + fa.tolq, base_hi = tb.xmin - fa.tolq;
#pragma unroll
    for (int j = 0; j < MAXM; ++j) {
      uint64_t best = ((uint64_t)0x7f800000u << 32) | 0x7fffffffu;
      if (marker_live<MAXM>(j, M)) {
        int c0 = 0, c1 = B;
        if (PRUNE) {
          const float flo = (u[j] - base_lo) * tb.inv_bw;
          const float fhi = (u[j] - base_hi) * tb.inv_bw;
          c0 = tb.bstart[(int)__builtin_amdgcn_fmed3f(flo, 0.0f, fmaxb)];
          c1 = tb.bstart[(int)__builtin_amdgcn_fmed3f(fhi, 0.0f, fmaxb) + 1];
        }
        visited += c1 - c0;
        const float uj = u[j], vj = v[j];
        const f32x2 uvj = pk2(uj, vj);
        auto visit = [&](BlobXY<float> p, int o, bool in) {
          const f32x2 dd = pk2(p.x, p.y) - uvj;  // (dx, dy) in one v_pk_add_f32
          const float d = fmadd(dd.x, dd.x, dd.y * dd.y);
          const uint64_t key = ((uint64_t)__float_as_uint(d) << 32) | (uint32_t)o;
          best = (in & (key < best)) ? key : best;
        };
        for (int c = c0; c < c1; c += 2) {
          const BlobXY<float> pa = tb.bxy[c], pb = tb.bxy[c + 1];
          const int oa = tb.orig[c], ob = tb.orig[c + 1];
          visit(pa, oa, true);
          visit(pb, ob, c + 1 < c1);
        }
      }
      const float bm = __uint_as_float((uint32_t)(best >> 32));
      m[j] = bm;
      r[j] = bm < INFINITY ? (int)(uint32_t)best : 0;
    }
    return visited;
  }
#pragma unroll
  for (int j = 0; j < MAXM; ++j) {
    T best = inf_t<T>();
    int bc = -1;  // table position of the current minimum
    if (marker_live<MAXM>(j, M)) {
      int c0 = 0, c1 = B;
      if (PRUNE) {
        c0 = tb.bstart[bucket_of(u[j] - fa.tolq, tb.xmin, tb.inv_bw, tb.nb)];
        c1 = tb.bstart[bucket_of(u[j] + fa.tolq, tb.xmin, tb.inv_bw, tb.nb) + 1];
      }
      visited += c1 - c0;
      auto visit = [&](int c, BlobXY<T> p) {
        const T dx = p.x - u[j];
        const T dy = p.y - v[j];
        const T d = fmadd(dx, dx, dy * dy);
        if (d < best) {
          best = d;
          bc = c;
        } else if (d == best && bc >= 0 && tb.orig[c] < tb.orig[bc]) {
          bc = c;
        }
      };
      int c = c0;
      for (; c + 1 < c1; c += 2) {  // two candidates' LDS reads in flight per step
        const BlobXY<T> pa = tb.bxy[c], pb = tb.bxy[c + 1];
        visit(c, pa);
        visit(c + 1, pb);
      }
      if (c < c1) visit(c, tb.bxy[c]);
    }
    m[j] = best;
    r[j] = bc >= 0 ? tb.orig[bc] : 0;
  }
  return visited;
}

// Eigen's visitor starts from coeff(0,0): a NaN distance there poisons the first minCoeff -> break at k=0
template <typename T>
__device__ __forceinline__ bool nan_at_origin(T b0x, T b0y, T u0, T v0) {
  const T dx = b0x - u0, dy = b0y - v0;
  const T d = dx * dx + dy * dy;
  return d != d;
}
// The same test with the table's blob 0 finite (host flag, wave-uniform): (b0 - u0)^2 + (b0y - v0)^2 is NaN
// exactly when u0 or v0 is NaN (an infinite difference squares to +inf and inf + inf = inf), one v_cmp_u; the
// blob is read from the table header only when it is not finite.
template <typename T>
__device__ __forceinline__ bool nan_at_origin_tb(const FrameArgsT<T>& fa, const LdsBlobs<T>& tb, T u0, T v0) {
  if (fa.grid.b0fin) return __builtin_isunordered(u0, v0);
  const T* hdr = (const T*)tb.base;
  return nan_at_origin(hdr[2], hdr[3], u0, v0);
}

// Extraction order = ascending (m_j, j): column minima are never NaN (they start at +inf and a NaN
// distance never compares smaller), so a sorting network on the (m_j, j) keys yields exactly the pair
// sequence of the reference's repeated minCoeff.  Batcher's odd-even merge sort, fully unrolled
// (MAXM = 8: 19 compare-exchanges); markers j >= M sort last with key +inf and lie beyond L anyway.
template <typename T>
__device__ __forceinline__ void cas_key(T& ma, int& ja, int& ra, T& mb, int& jb, int& rb) {
  const bool sw = mb < ma || (mb == ma && jb < ja);
  const T m0 = sw ? mb : ma, m1 = sw ? ma : mb;
  const int j0 = sw ? jb : ja, j1 = sw ? ja : jb;
  const int r0 = sw ? rb : ra, r1 = sw ? ra : rb;
  ma = m0; mb = m1; ja = j0; jb = j1; ra = r0; rb = r1;
}
template <typename T, int MAXM>
__device__ __forceinline__ void sort_minima(T* km, int* kj, int* kr) {
#pragma unroll
  for (int p = 1; p < MAXM; p <<= 1)
#pragma unroll
    for (int k = p; k >= 1; k >>= 1)
#pragma unroll
      for (int j = k % p; j + k < MAXM; j += 2 * k)
#pragma unroll
        for (int i = 0; i < k; ++i)
          if (i + j + k < MAXM && (i + j) / (2 * p) == (i + j + k) / (2 * p))
            cas_key(km[i + j], kj[i + j], kr[i + j], km[i + j + k], kj[i + j + k], kr[i + j + k]);
}

template <typename T, int MAXM, bool PAIRS>
__device__ __forceinline__ T score_minima(const FrameArgsT<T>& fa, const T* m, const int* r, uint32_t* pairs,
                                          int* npairs) {
  const int B = fa.B, M = fa.M;
  const int L = B < M ? B : M;
  const T tol = fa.tol, tol_pf = fa.tol_pf, Mt = (T)M;
  T km[MAXM];
  int kj[MAXM], kr[MAXM];
#pragma unroll
  for (int j = 0; j < MAXM; ++j) {
    km[j] = marker_live<MAXM>(j, M) ? m[j] : inf_t<T>();
    kj[j] = j;
    kr[j] = r[j];
  }
  sort_minima<T, MAXM>(km, kj, kr);
  T Pr = (T)0;
  int s = 1;
  bool live = true;
  if (PAIRS) *npairs = 0;
#pragma unroll
  for (int k = 0; k < MAXM; ++k) {
    if (k < L && live) {
      const T d = sqrt_t(km[k]);
      if (!(d <= tol_pf)) {
        live = false;  // the reference's break
      } else {
        const T q = div_t(tol - d, tol);
        Pr = Pr + (Mt + q * q);
        bool dup = false;  // an earlier (accepted) pair holds the same blob
#pragma unroll
        for (int e = 0; e < k; ++e) dup |= kr[e] == kr[k];
        if (dup) {
          Pr = Pr - (T)(s * 3);
          ++s;
        }
        if ((fa.downgrade >> kj[k]) & 1u) Pr = Pr - (T)2;
        if (PAIRS) {
          pairs[2 * k] = (uint32_t)kj[k] + 1u;
          pairs[2 * k + 1] = (uint32_t)kr[k] + 1u;
          *npairs = k + 1;
        }
      }
    }
  }
  return Pr;
}

// The weight of score_minima<PAIRS = false> without the sort, for B >= M (fp32 tolerance path).  With
// L = min(B, M) = M the cap never binds, and since the extraction runs in ascending distance the reference's
// break leaves exactly the markers whose own minimum passes the gate: A = {j : sqrt(m_j) <= tol_PF}.  The
// penalties depend on A only: 3*(1 + ... + D) with D = |A| - #distinct blobs over A (each marker whose blob
// an earlier marker of A holds, in ANY fixed order, counts once: the same D as in extraction order), and 2
// per downgraded marker of A.  Only the order of the fp32 additions differs from the extraction order
// (a few ulp of a weight <= M(M+1)).
template <int MAXM>
__device__ __forceinline__ float score_unordered(const FrameArgsT<float>& fa, const float* m, const int* r) {
  const int M = fa.M;
  const float tol = fa.tol, tol_pf = fa.tol_pf, Mt = (float)M;
  const float rtol = rcp_t(tol);
  float Pr = 0.0f;
  int dups = 0;
  bool acc[MAXM];
#pragma unroll
  for (int j = 0; j < MAXM; ++j) {
    const float d = sqrt_t(m[j]);
    acc[j] = d <= tol_pf;  // markers past M have m = +inf (column_minima), never accepted
    const float q = (tol - d) * rtol;
    Pr = acc[j] ? Pr + (Mt + q * q) : Pr;
    bool dup = false;
#pragma unroll
    for (int e = 0; e < j; ++e) dup |= acc[e] & (r[e] == r[j]);
    dups += (acc[j] & dup) ? 1 : 0;
  }
  int ndg = 0;
  if (fa.downgrade) {  // wave-uniform: the downgrade penalties (2 per accepted downgraded marker)
#pragma unroll
    for (int j = 0; j < MAXM; ++j) ndg += (acc[j] && ((fa.downgrade >> j) & 1u)) ? 1 : 0;
  }
  return Pr - (float)(3 * dups * (dups + 1) / 2 + 2 * ndg);
}

// ---- blob table (DESIGN.md "Exact blob pruning"), built once per frame on the host (build_blob_table_host,
// O(B)) and copied whole into each block's LDS by the weighing kernels.  Layout, every part 16-byte aligned:
//   base  hdr {T xmin, inv_bw, b0x, b0y} | int32 bstart[nb+1] | BlobXY<T> xy[B] | int32 orig[B]
//         (the blobs grouped into nb = bucket_count(B) x-buckets, increasing original index within a bucket;
//         every blob once: the linear scans of pose_pairs / k_resample_final and the fp64 pruned minima)
//   grid  GridHdr | uint32 cell[ncell] (byte offset of the list in ent[] | count << 16) | GridEnt ent[nent + 1]
//         (fp32 tables: a 2D cell grid over the blobs' bounding box widened by the pruning half-window; cell c
//         lists every blob whose +-tolq box (plus 0.01 px) overlaps it, so a marker's candidates are ONE
//         cell's list.  ent[0] is a sentinel {+inf, +inf, 0}: an empty cell points at it, so every query reads
//         one entry without a test.  ncell = 0: no grid, the x-buckets serve; fp64 tables and large B never
//         build one)
// The cell budget of a table's grid: the coarse one (2,048 cells, 8 KB of records) for ordinary blob counts, the 4x
// finer one (8,192, 32 KB) from kGridFineMinBlobs blobs (C3's 200 with clutter), whose cell lists are otherwise long
// enough that most waves walk them: measured (profiles/r06/ab_grid_cells.txt) C3 weighing 56.5 -> 50.8 us with the
// fine grid, while at 50 blobs (C2 / C4 / C5) its larger table copy costs 1.5-1.8 us per frame.  A fine grid over the
// entry budget falls back to the coarse one, then to the x-buckets.
constexpr int kGridMaxCells = 8192;   // cell records: 32 KB
constexpr int kGridCoarseCells = 2048;
#ifndef PFMPE_GRID_FINE_MIN_BLOBS
#define PFMPE_GRID_FINE_MIN_BLOBS 128
#endif
constexpr int kGridFineMinBlobs = PFMPE_GRID_FINE_MIN_BLOBS;
constexpr int kGridMaxEntries = 1024; // list entries: 16 KB (B up to ~400 blobs at 2-3 cells each)
template <typename T>
struct BlobTable {
  static constexpr size_t off_bstart() { return align16(4 * sizeof(T)); }
  static constexpr size_t off_xy(int B) { return off_bstart() + align16((size_t)(bucket_count(B) + 1) * 4); }
  static constexpr size_t off_orig(int B) { return off_xy(B) + align16((size_t)B * sizeof(BlobXY<T>)); }
  // the base part (every blob once): all the linear scans need
  static constexpr size_t bytes(int B) { return off_orig(B) + align16((size_t)B * 4); }
  static constexpr size_t off_grid(int B) { return bytes(B); }
  static constexpr size_t grid_bytes(int ncell, int nent) {
    return sizeof(GridHdr) + align16((size_t)ncell * 4) + (size_t)(nent + 1) * sizeof(GridEnt);
  }
  // a table's total size: base + grid (the host builder returns it; FrameArgsT::tbytes carries it)
  static constexpr size_t total_bytes(int B, int ncell, int nent) { return bytes(B) + grid_bytes(ncell, nent); }
  static constexpr size_t max_bytes() { return total_bytes(kMaxBlobs, kGridMaxCells, kGridMaxEntries); }
  // LDS of the weighing kernels: the table plus one 16-B granule, so the masked second candidate of the
  // fp32 column_minima steps (x-buckets, grid lists) reads inside the allocation
  static constexpr size_t lds_bytes(size_t tbytes) { return tbytes + 16; }
};

template <typename T>
struct LdsBlobs {
  const unsigned char* base;  // the table (the grid's parts sit at FrameArgsT::grid offsets from it)
  const BlobXY<T>* bxy;
  const int32_t* orig;
  const int32_t* bstart;  // nb + 1
  T xmin, inv_bw;  // blob 0 (header words 2, 3): read where needed (nan_at_origin_tb)
  int nb;
};

template <typename T>
__host__ __device__ __forceinline__ LdsBlobs<T> view_table(const unsigned char* base, int B) {
  LdsBlobs<T> t;
  const T* hdr = (const T*)base;
  t.base = base;
  t.xmin = hdr[0];
  t.inv_bw = hdr[1];
  t.nb = bucket_count(B);
  t.bstart = (const int32_t*)(base + BlobTable<T>::off_bstart());
  t.bxy = (const BlobXY<T>*)(base + BlobTable<T>::off_xy(B));
  t.orig = (const int32_t*)(base + BlobTable<T>::off_orig(B));
  return t;
}

// The kernel arguments of a table's grid (host): on only when the table has a grid built for at least the
// frame's window (tolq: FrameArgsT::tolq of the frame).  gh: the table's GridHdr (at off_grid(B)).
template <typename T>
inline GridArgs grid_args(const GridHdr& gh, int B, float tolq) {
  GridArgs g{};
  g.b0fin = gh.b0fin;
  g.on = (gh.ncell > 0 && gh.gtolq >= tolq) ? 1 : 0;
  if (!g.on) return g;
  g.inv_c = gh.inv_c;
  g.ox = (float)(-(double)gh.gx0 * (double)gh.inv_c);  // build_blob_table_host's proof covers this rounding
  g.oy = (float)(-(double)gh.gy0 * (double)gh.inv_c);
  g.fmaxx = gh.fmaxx;
  g.fmaxy = gh.fmaxy;
  g.ncx4 = 4 * gh.ncx;
  g.cell_off = (int32_t)(BlobTable<T>::off_grid(B) + sizeof(GridHdr));
  g.ent_off = g.cell_off + (int32_t)align16((size_t)gh.ncell * 4);
  return g;
}

// Host builder; returns the table's size in bytes.  The bucket formula is bucket_of in T arithmetic (this TU:
// -ffp-contract=off), the same expression the kernels evaluate for their query windows.  tolq: the pruning
// half-window of the frames that will use the table (FrameArgsT::tolq, from tol_PF).
template <typename T>
inline size_t build_blob_table_host(const double* blobs, int B, double tolq, unsigned char* dst) {
  T xmin = (T)INFINITY, xmax = -(T)INFINITY;
  for (int i = 0; i < B; ++i) {
    const T x = (T)blobs[2 * i];
    xmin = x < xmin ? x : xmin;
    xmax = x > xmax ? x : xmax;
  }
  if (B == 0 || !(xmax - xmin < (T)INFINITY)) {
    xmin = (T)0;
    xmax = (T)1;
  }
  T span = xmax - xmin;
  if (!(span > (T)0)) span = (T)1;
  const int nb = bucket_count(B);
  const T inv_bw = (T)nb / span;
  T* hdr = (T*)dst;
  hdr[0] = xmin;
  hdr[1] = inv_bw;
  hdr[2] = B > 0 ? (T)blobs[0] : (T)0;
  hdr[3] = B > 0 ? (T)blobs[1] : (T)0;
  int32_t* bstart = (int32_t*)(dst + BlobTable<T>::off_bstart());
  BlobXY<T>* xy = (BlobXY<T>*)(dst + BlobTable<T>::off_xy(B));
  int32_t* orig = (int32_t*)(dst + BlobTable<T>::off_orig(B));
  int32_t cnt[kMaxBuckets + 1] = {0};
  for (int i = 0; i < B; ++i) ++cnt[bucket_of((T)blobs[2 * i], xmin, inv_bw, nb) + 1];
  for (int b = 0; b < nb; ++b) cnt[b + 1] += cnt[b];
  for (int b = 0; b <= nb; ++b) bstart[b] = cnt[b];
  for (int i = 0; i < B; ++i) {
    const int pos = cnt[bucket_of((T)blobs[2 * i], xmin, inv_bw, nb)]++;
    xy[pos].x = (T)blobs[2 * i];
    xy[pos].y = (T)blobs[2 * i + 1];
    orig[pos] = i;
  }
  // ---- the grid (fp32 tables).  Device query: cell coordinate f = fma(u, inv_c, ox), ox = fl(-gx0 * inv_c),
  // clamped by med3 to [0, ncx - 1], truncated.  Every blob within tol_PF of a query must be in the query's
  // cell list:
  //  * a blob is listed in every cell whose real-arithmetic interval [g(bx - m), g(bx + m)] it overlaps,
  //    g(x) = (x - gx0) * inv_c with the fp32 constants the device uses, m = tolq + 0.01 px;
  //  * the device's f differs from g(u) by the rounding of ox and of the fma (cell coordinates < 2^7: a few
  //    1e-6 cells, 1e-4 px), far below the m - tol_PF >= 0.01 px slack; a clamped query (outside the widened
  //    box) has no blob within tolq at all, so whatever its cell lists, its minimum fails the gate;
  //  * every blob's own interval is clamped to the grid the same way.
  // Each list holds its blobs in increasing original index (the fill below runs over i), so the device's
  // strict "closer" comparison keeps the lowest index among equally close blobs: the reference's tie rule.
  GridHdr* gh = (GridHdr*)(dst + BlobTable<T>::off_grid(B));
  std::memset(gh, 0, sizeof(GridHdr));
  gh->b0fin = (B > 0 && std::isfinite((double)hdr[2]) && std::isfinite((double)hdr[3])) ? 1 : 0;
  size_t total = BlobTable<T>::total_bytes(B, 0, 0);
  if (!std::is_same<T, float>::value || B == 0) return total;
  const double m = tolq + 0.01;
  double bx0 = INFINITY, bx1 = -INFINITY, by0 = INFINITY, by1 = -INFINITY;
  for (int i = 0; i < B; ++i) {
    const double x = (double)(float)blobs[2 * i], y = (double)(float)blobs[2 * i + 1];
    if (!(x - x == 0.0) || !(y - y == 0.0)) return total;  // a non-finite blob: no grid
    bx0 = std::min(bx0, x), bx1 = std::max(bx1, x), by0 = std::min(by0, y), by1 = std::max(by1, y);
  }
  const double gx0 = bx0 - m, gy0 = by0 - m, w = bx1 - bx0 + 2 * m, h = by1 - by0 + 2 * m;
  for (int budget = B >= kGridFineMinBlobs ? kGridMaxCells : kGridCoarseCells;; budget = kGridCoarseCells) {
  // square cells: at least the window (2m) and few enough for the cell budget
  double cs = std::max(2.0 * m, std::sqrt(w * h / (double)budget));
  int ncx = (int)std::ceil(w / cs), ncy = (int)std::ceil(h / cs);
  while ((int64_t)ncx * ncy > budget) {
    cs *= 1.0625;
    ncx = (int)std::ceil(w / cs);
    ncy = (int)std::ceil(h / cs);
  }
  ncx = std::max(1, ncx);
  ncy = std::max(1, ncy);
  const float inv_c = (float)(1.0 / cs), gx0f = (float)gx0, gy0f = (float)gy0;
  // The device's cell coordinate fma(u, inv_c, ox) rounds twice (ox = fl(-gx0 * inv_c), then the fma), each by at
  // most half an ulp of a value below |ox| + ncx cells, i.e. 2^-24 (|ox| + ncx) cells of cs px.  The lists hold
  // every blob within m = tolq + 0.01 px of a cell, so the proof needs that error well inside m - tolq = 0.01 px:
  // far-out blob coordinates (|gx0| ~ 1e5 px and beyond) make |ox| large, and then the x-buckets
  // serve instead of the grid.
  {
    const double ex = std::ldexp(std::abs((double)gx0f) * (double)inv_c + ncx + 1.0, -23) * cs;
    const double ey = std::ldexp(std::abs((double)gy0f) * (double)inv_c + ncy + 1.0, -23) * cs;
    if (!(std::max(ex, ey) <= 0.25 * (m - tolq))) return total;
  }
  auto crange = [&](double lo, double hi, float inv, float org, int n, int& c0, int& c1) {
    const double f0 = (lo - (double)org) * (double)inv, f1 = (hi - (double)org) * (double)inv;
    c0 = (int)std::max(0.0, std::min((double)(n - 1), std::floor(f0)));
    c1 = (int)std::max(0.0, std::min((double)(n - 1), std::floor(f1)));
  };
  const int ncell = ncx * ncy;
  std::vector<int32_t> count(ncell + 1, 0);
  int nent = 0;
  for (int pass = 0; pass < 2; ++pass) {
    std::vector<int32_t> fill;
    if (pass == 1) {
      for (int c = 0; c < ncell; ++c) count[c + 1] += count[c];
      fill.assign(count.begin(), count.end() - 1);
    }
    for (int i = 0; i < B; ++i) {
      const double x = (double)(float)blobs[2 * i], y = (double)(float)blobs[2 * i + 1];
      int cx0, cx1, cy0, cy1;
      crange(x - m, x + m, inv_c, gx0f, ncx, cx0, cx1);
      crange(y - m, y + m, inv_c, gy0f, ncy, cy0, cy1);
      for (int cy = cy0; cy <= cy1; ++cy)
        for (int cx = cx0; cx <= cx1; ++cx) {
          const int c = cy * ncx + cx;
          if (pass == 0) {
            ++count[c + 1];
            ++nent;
          } else {
            const int e = 1 + fill[c]++;  // ent[0]: the sentinel
            GridEnt* ent = (GridEnt*)((unsigned char*)gh + sizeof(GridHdr) + align16((size_t)ncell * 4));
            ent[e] = GridEnt{(float)blobs[2 * i], (float)blobs[2 * i + 1], i, 0};
          }
        }
    }
    if (pass == 0 && nent > kGridMaxEntries) break;  // too many entries: a coarser grid, then the x-buckets
  }
  if (nent > kGridMaxEntries) {
    if (budget == kGridCoarseCells) return total;
    continue;
  }
  uint32_t* cell = (uint32_t*)((unsigned char*)gh + sizeof(GridHdr));
  for (int c = 0; c < ncell; ++c) {  // an empty cell points at the sentinel (byte offset 0)
    const uint32_t n = (uint32_t)(count[c + 1] - count[c]);
    cell[c] = (n ? (uint32_t)(1 + count[c]) * (uint32_t)sizeof(GridEnt) : 0u) | (n << 16);
  }
  GridEnt* ent = (GridEnt*)((unsigned char*)cell + align16((size_t)ncell * 4));
  ent[0] = GridEnt{INFINITY, INFINITY, 0, 0};  // sentinel: distance +inf (NaN for a non-finite query), index 0

  gh->inv_c = inv_c;
  gh->gx0 = gx0f;
  gh->gy0 = gy0f;
  gh->fmaxx = (float)(ncx - 1);
  gh->fmaxy = (float)(ncy - 1);
  gh->gtolq = (float)tolq;
  gh->ncx = ncx;
  gh->ncell = ncell;
  gh->nent = nent;
  return BlobTable<T>::total_bytes(B, ncell, nent);
  }
}

// block-wide copy of the table into LDS (16-byte words); callers barrier before use
__device__ __forceinline__ void copy_table(const unsigned char* __restrict__ src, unsigned char* dst, size_t bytes) {
  // global loads (src may come from a batched launch's stream descriptor, which hides its address space)
  typedef __attribute__((address_space(1))) const u32x4_t gv4_t;
  gv4_t* s4 = (gv4_t*)src;
  u32x4_t* d4 = (u32x4_t*)dst;
  const int n4 = (int)(bytes / 16);
  for (int i = threadIdx.x; i < n4; i += kBlock) d4[i] = s4[i];
}

// copy_table + stage_consts_from with every load issued before the first LDS store: one memory round trip for the
// table (its first 8 KB: two 16-B loads per thread), the frame constants and whatever the caller issued before
// (k_frame2: the prior), instead of one per loop and per copy
template <typename T>
__device__ __forceinline__ void stage_table_consts(const unsigned char* __restrict__ src, unsigned char* dst, size_t bytes,
                                                   const uint32_t* cw_src, LdsConst<T>& sc) {
  typedef __attribute__((address_space(1))) const u32x4_t gv4_t;
  gv4_t* s4 = (gv4_t*)src;
  u32x4_t* d4 = (u32x4_t*)dst;
  const int n4 = (int)(bytes / 16);
  const int t = threadIdx.x;
  constexpr int kWordsC = (int)(sizeof(LdsConst<T>) / 4);
  static_assert(kWordsC <= kBlock, "one constant word per thread");
  u32x4_t r0 = {0u, 0u, 0u, 0u}, r1 = {0u, 0u, 0u, 0u};
  uint32_t cw = 0u;
  if (t < n4) r0 = s4[t];
  if (t + kBlock < n4) r1 = s4[t + kBlock];
  if (t < kWordsC) cw = cw_src[t];
  if (t < n4) d4[t] = r0;
  if (t + kBlock < n4) d4[t + kBlock] = r1;
  if (t < kWordsC) ((uint32_t*)&sc)[t] = cw;
  for (int i = t + 2 * kBlock; i < n4; i += kBlock) d4[i] = s4[i];  // tables past 8 KB (large B)
}

// ---- one particle through the motion model, projection and likelihood (PE:543-604, PE:2385)
template <typename T, int RNG, int MAXM, bool PRUNE, bool PHASED = false>
__device__ __forceinline__ T weigh_particle(const FrameArgsT<T>& fa, const LdsConst<T>& sc, const LdsBlobs<T>& tb,
                                            const T* A, int n, int iter, T* P, int* nvisit = nullptr,
                                            uint64_t* st = nullptr) {
  T u[MAXM], v[MAXM];
  propagate<T, RNG>(fa, sc, A, n, iter, P);
  if (st && threadIdx.x == 0) stamp_max(st, 27, rt_now() + (P[11] == (T)12345 ? 1 : 0));
  project_markers<T, MAXM>(fa, sc, P, u, v);
  if (st && threadIdx.x == 0) stamp_max(st, 28, rt_now() + (u[0] == (T)12345 ? 1 : 0));
  T w = (T)0;
  if (fa.B > 0 && !nan_at_origin_tb(fa, tb, u[0], v[0])) {
    T m[MAXM];
    int r[MAXM];
    const int visited = column_minima<T, MAXM, PRUNE, PHASED>(fa, u, v, tb, m, r);
    if (nvisit) *nvisit = visited;
    if (st && threadIdx.x == 0) stamp_max(st, 29, rt_now() + (m[0] == (T)12345 ? 1 : 0));
    if constexpr (std::is_same<T, float>::value) {
      if (fa.B >= fa.M && !(fa.diag & kDiagSortedScore))  // wave-uniform
        w = score_unordered<MAXM>(fa, m, r);
      else
        w = score_minima<T, MAXM, false>(fa, m, r, nullptr, nullptr);
    } else {
      w = score_minima<T, MAXM, false>(fa, m, r, nullptr, nullptr);
    }
  }
  return w;
}

}  // namespace pfmpe
