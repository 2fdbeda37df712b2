// pf_wave.hpp — wave and block primitives: DPP steps, reductions, scans, and the diagnostic stamps.
#pragma once
#include <math.h>

#include "pf_types.hpp"

namespace pfmpe {

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
// Lanes of ONE wave exchanging data through LDS without a workgroup barrier: the hardware keeps a
// wave's LDS operations in order, but the compiler must also be told that other lanes wrote (else it
// may forward a lane's own earlier store to its read).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int wave_id() { return threadIdx.x >> 6; }
// the same, as an SGPR (block sizes are multiples of 64): a loop over the earlier waves then has a scalar trip
// count instead of a per-wave v_cndmask chain.  (Used where that pays: as the general wave_id it moved the
// weighing pass's register allocation for the worse.)
__device__ __forceinline__ int wave_id_u() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// All wave-level scans and reductions run on DPP lane moves (no LDS, no ds_bpermute): row_shr 1/2/4/8
// builds the inclusive scan inside each 16-lane row, row_bcast:15 / row_bcast:31 carry row totals
// across rows (GFX9-family DPP, kept by gfx950), so lane 63 ends with the wave total.  The pattern is
// fixed, so a sum has ONE association everywhere it is evaluated (k_propagate_weigh and k_resample
// must agree bit-for-bit).  Every lane of the wave must execute these (no divergent calls).
enum : int {
  kDppRowShr1 = 0x111, kDppRowShr2 = 0x112, kDppRowShr4 = 0x114, kDppRowShr8 = 0x118,
  kDppWaveShr1 = 0x138, kDppBcast15 = 0x142, kDppBcast31 = 0x143
};
template <int CTRL, int RM = 0xf>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t src, uint32_t old) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)src, CTRL, RM, 0xf, false);
}
template <int CTRL, int RM = 0xf>
__device__ __forceinline__ int dpp(int src, int old) {
  return (int)dpp_u32<CTRL, RM>((uint32_t)src, (uint32_t)old);
}
template <int CTRL, int RM = 0xf>
__device__ __forceinline__ float dpp(float src, float old) {
  return __uint_as_float(dpp_u32<CTRL, RM>(__float_as_uint(src), __float_as_uint(old)));
}
template <int CTRL, int RM = 0xf>
__device__ __forceinline__ double dpp(double src, double old) {
  const uint64_t s = (uint64_t)__double_as_longlong(src), o = (uint64_t)__double_as_longlong(old);
  const uint32_t lo = dpp_u32<CTRL, RM>((uint32_t)s, (uint32_t)o);
  const uint32_t hi = dpp_u32<CTRL, RM>((uint32_t)(s >> 32), (uint32_t)(o >> 32));
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
// value of lane L in every lane (scalar result)
// A value the optimiser may not look through.  In a select chain over a register array (lane q picks word
// q) the loads would otherwise be folded into ONE load of a selected address, which pins the array in
// scratch memory (a VMEM round trip per use); with the values opaque the chain stays v_cndmask.
template <typename V>
__device__ __forceinline__ V opaque(V x) {
  asm volatile("" : "+v"(x));
  return x;
}
__device__ __forceinline__ int lane_value(int x, int L) { return __builtin_amdgcn_readlane(x, L); }
__device__ __forceinline__ float lane_value(float x, int L) {
  return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(x), L));
}
__device__ __forceinline__ double lane_value(double x, int L) {
  const uint64_t v = (uint64_t)__double_as_longlong(x);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, L);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), L);
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
// lane i receives lane i-1's value, lane 0 receives `fill`
template <typename V>
__device__ __forceinline__ V wave_shr1(V x, V fill) {
  return dpp<kDppWaveShr1>(x, fill);
}

struct OpSum {
  __device__ double operator()(double a, double b) const { return a + b; }
};
struct OpMax {
  __device__ double operator()(double a, double b) const { return b > a ? b : a; }
};
struct OpMin {
  __device__ double operator()(double a, double b) const { return b < a ? b : a; }
};
struct OpMaxI {
  __device__ int operator()(int a, int b) const { return b > a ? b : a; }
};
// inclusive scan x_0 op ... op x_i; `id` is the identity of op
template <typename V, typename Op>
__device__ __forceinline__ V wave_scan(V x, V id, Op op) {
  x = op(x, dpp<kDppRowShr1>(x, id));
  x = op(x, dpp<kDppRowShr2>(x, id));
  x = op(x, dpp<kDppRowShr4>(x, id));
  x = op(x, dpp<kDppRowShr8>(x, id));
  x = op(x, dpp<kDppBcast15, 0xa>(x, id));
  x = op(x, dpp<kDppBcast31, 0xc>(x, id));
  return x;
}
// Sum scan of doubles: the four row_shr steps read 0 (bound_ctrl) from a lane outside the row, which is the
// sum's identity (+0.0 is all-zero bits), so they need no fill register; the two row_bcast steps write only
// some rows and keep the fill.  Bit-identical to wave_scan(v, 0.0, OpSum()).
template <int CTRL>
__device__ __forceinline__ double dpp_zf(double x) {
  const uint64_t v = (uint64_t)__double_as_longlong(x);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)v, CTRL, 0xf, 0xf, true);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)(v >> 32), CTRL, 0xf, 0xf, true);
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
__device__ __forceinline__ double wave_incl_sum(double x) {
  x = x + dpp_zf<kDppRowShr1>(x);
  x = x + dpp_zf<kDppRowShr2>(x);
  x = x + dpp_zf<kDppRowShr4>(x);
  x = x + dpp_zf<kDppRowShr8>(x);
  x = x + dpp<kDppBcast15, 0xa>(x, 0.0);
  x = x + dpp<kDppBcast31, 0xc>(x, 0.0);
  return x;
}
__device__ __forceinline__ double wave_incl_max(double v) { return wave_scan(v, -(double)INFINITY, OpMax()); }
__device__ __forceinline__ double wave_incl_min(double v) { return wave_scan(v, (double)INFINITY, OpMin()); }
__device__ __forceinline__ double wave_max(double v) { return lane_value(wave_incl_max(v), 63); }
__device__ __forceinline__ double wave_min(double v) { return lane_value(wave_incl_min(v), 63); }

// (value, index): larger value wins, lower index on ties
// (selects, not branches: the wave reductions stay one basic block)
template <typename V>
__device__ __forceinline__ void cmb_max(V& v, int& i, V v2, int i2) {
  const bool t = (v2 > v) | ((v2 == v) & (i2 < i));  // non-short-circuit: no exec-mask branches
  v = t ? v2 : v;
  i = t ? i2 : i;
}
template <typename V>
__device__ __forceinline__ void cmb_min(V& v, int& i, V v2, int i2) {
  const bool t = (v2 < v) | ((v2 == v) & (i2 < i));
  v = t ? v2 : v;
  i = t ? i2 : i;
}
// wave arg-reductions: the lexicographic (value, index) order is associative and commutative, so the
// scan pattern reduces it exactly; the result is broadcast to every lane
template <typename V, int CTRL, int RM = 0xf>
__device__ __forceinline__ void argmax_step(V& v, int& i, V idv) {
  const V v2 = dpp<CTRL, RM>(v, idv);
  const int i2 = dpp<CTRL, RM>(i, 0x7fffffff);
  cmb_max(v, i, v2, i2);
}
template <typename V, int CTRL, int RM = 0xf>
__device__ __forceinline__ void argmin_step(V& v, int& i, V idv) {
  const V v2 = dpp<CTRL, RM>(v, idv);
  const int i2 = dpp<CTRL, RM>(i, 0x7fffffff);
  cmb_min(v, i, v2, i2);
}
template <typename V>
__device__ __forceinline__ void wave_argmax(V& v, int& i) {
  const V id = -(V)INFINITY;
  argmax_step<V, kDppRowShr1>(v, i, id);
  argmax_step<V, kDppRowShr2>(v, i, id);
  argmax_step<V, kDppRowShr4>(v, i, id);
  argmax_step<V, kDppRowShr8>(v, i, id);
  argmax_step<V, kDppBcast15, 0xa>(v, i, id);
  argmax_step<V, kDppBcast31, 0xc>(v, i, id);
  v = lane_value(v, 63);
  i = lane_value(i, 63);
}
template <typename V>
__device__ __forceinline__ void wave_argmin(V& v, int& i) {
  const V id = (V)INFINITY;
  argmin_step<V, kDppRowShr1>(v, i, id);
  argmin_step<V, kDppRowShr2>(v, i, id);
  argmin_step<V, kDppRowShr4>(v, i, id);
  argmin_step<V, kDppRowShr8>(v, i, id);
  argmin_step<V, kDppBcast15, 0xa>(v, i, id);
  argmin_step<V, kDppBcast31, 0xc>(v, i, id);
  v = lane_value(v, 63);
  i = lane_value(i, 63);
}
// int counts: "-infinity" is INT_MIN
template <>
__device__ __forceinline__ void wave_argmax<int>(int& v, int& i) {
  const int id = (int)0x80000000;
  argmax_step<int, kDppRowShr1>(v, i, id);
  argmax_step<int, kDppRowShr2>(v, i, id);
  argmax_step<int, kDppRowShr4>(v, i, id);
  argmax_step<int, kDppRowShr8>(v, i, id);
  argmax_step<int, kDppBcast15, 0xa>(v, i, id);
  argmax_step<int, kDppBcast31, 0xc>(v, i, id);
  v = lane_value(v, 63);
  i = lane_value(i, 63);
}

// Deterministic block inclusive scan: pre_w = ((0 + t_0) + t_1) + ... over earlier waves' totals, then
// incl = pre_w + (wave inclusive).  k_propagate_weigh derives its partial extrema with exactly this
// association, so both launches see bit-identical prefixes.  sh: >= kWaves doubles.
// The wave scan of fp32 weights on the 2^-21 grid as integers.  Every weight of an M >= 4 frame is a multiple of
// 2^-21 (each score term Mt + q^2 is >= 4, so every partial score, the integer penalties subtracted, is too), so
// with 0 <= w < 32 in the wave, w * 2^21 is an integer below 2^26 and every 64-lane prefix lies below 2^32: the u32
// scan is the exact prefix sum, which wave_incl_sum's fp64 partial sums (at most 32 significant bits) also are.
// One v_add_u32_dpp per step instead of two v_mov_b32_dpp and a v_add_f64.
__device__ __forceinline__ double wave_incl_sum_fx(float w) {
  uint32_t x = (uint32_t)(w * 0x1p21f);
  x += (uint32_t)__builtin_amdgcn_mov_dpp((int)x, kDppRowShr1, 0xf, 0xf, true);
  x += (uint32_t)__builtin_amdgcn_mov_dpp((int)x, kDppRowShr2, 0xf, 0xf, true);
  x += (uint32_t)__builtin_amdgcn_mov_dpp((int)x, kDppRowShr4, 0xf, 0xf, true);
  x += (uint32_t)__builtin_amdgcn_mov_dpp((int)x, kDppRowShr8, 0xf, 0xf, true);
  x += dpp_u32<kDppBcast15, 0xa>(x, 0u);
  x += dpp_u32<kDppBcast31, 0xc>(x, 0u);
  return (double)x * 0x1p-21;
}
// block inclusive prefix from the wave's inclusive scan wi (the earlier waves' totals through LDS)
__device__ __forceinline__ void block_incl_from_wave(double wi, double& incl, double* sh) {
  if (lane_id() == 63) sh[wave_id()] = wi;
  __syncthreads();
  double pre = 0.0;
  const int wv = wave_id_u();
#pragma clang loop unroll(disable)
  for (int w = 0; w < wv; ++w) pre = pre + sh[w];  // a scalar trip count: no per-wave select chain
  incl = pre + wi;
}
__device__ __forceinline__ void block_incl_sum(double v, double& incl, double* sh) {
  const double wi = wave_incl_sum(v);
  if (lane_id() == 63) sh[wave_id()] = wi;
  __syncthreads();
  double pre = 0.0;
  const int wv = wave_id_u();
#pragma clang loop unroll(disable)
  for (int w = 0; w < wv; ++w) pre = pre + sh[w];  // a scalar trip count: no per-wave select chain
  incl = pre + wi;
}

// ---- interleaved wave scans: several independent chains advanced step by step in ONE basic block, so
// the DPP / f64 latencies of one chain hide behind the others.  Each chain's arithmetic is exactly that
// of wave_scan / wave_argmax / wave_argmin (same steps, same identities, same operand order).
template <int C, int R>
struct DppStep {
  static constexpr int ctrl = C, rm = R;
};
template <typename F>
__device__ __forceinline__ void scan_steps(F&& f) {
  f(DppStep<kDppRowShr1, 0xf>{});
  f(DppStep<kDppRowShr2, 0xf>{});
  f(DppStep<kDppRowShr4, 0xf>{});
  f(DppStep<kDppRowShr8, 0xf>{});
  f(DppStep<kDppBcast15, 0xa>{});
  f(DppStep<kDppBcast31, 0xc>{});
}
template <typename S>
__device__ __forceinline__ void st_sum(double& x) {
  x = x + dpp<S::ctrl, S::rm>(x, 0.0);
}
template <typename S>
__device__ __forceinline__ void st_max(double& x) {
  const double y = dpp<S::ctrl, S::rm>(x, -(double)INFINITY);
  x = y > x ? y : x;
}
template <typename S>
__device__ __forceinline__ void st_min(double& x) {
  const double y = dpp<S::ctrl, S::rm>(x, (double)INFINITY);
  x = y < x ? y : x;
}
template <typename S, typename V>
__device__ __forceinline__ void st_argmax(V& v, int& i) {
  const V v2 = dpp<S::ctrl, S::rm>(v, -(V)INFINITY);
  const int i2 = dpp<S::ctrl, S::rm>(i, 0x7fffffff);
  cmb_max(v, i, v2, i2);
}
template <typename S, typename V>
__device__ __forceinline__ void st_argmin(V& v, int& i) {
  const V v2 = dpp<S::ctrl, S::rm>(v, (V)INFINITY);
  const int i2 = dpp<S::ctrl, S::rm>(i, 0x7fffffff);
  cmb_min(v, i, v2, i2);
}
template <typename V>
__device__ __forceinline__ void bcast63(V& v, int& i) {
  v = lane_value(v, 63);
  i = lane_value(i, 63);
}

// fl(a / b) without the fp64 division: y = fl(1 / b) (Ctrl::invS, one division per frame), q0 = fl(a y), then two
// Newton corrections with fma residuals.  After the first, q1 is a faithful approximation of a / b, so its residual
// a - b q1 is exact, and fl(q1 + r1 y) = fl(a / b) (Markstein's theorem: y correctly rounded, no overflow or
// underflow; tests/test_div_by_s.py checks 10^7 cases against IEEE division).  Callers use it only where the
// quotient is in [0, ~1] and b is a normal positive double (fp32 weights, no negative weight in the wave), and
// keep the IEEE division otherwise.
__device__ __forceinline__ double div_by_S(double a, double b, double y) {
  const double q0 = a * y;
  const double r0 = __builtin_fma(-b, q0, a);
  const double q1 = __builtin_fma(r0, y, q0);
  const double r1 = __builtin_fma(-b, q1, a);
  return __builtin_fma(r1, y, q1);
}

__device__ __forceinline__ uint64_t rt_now() { return __builtin_amdgcn_s_memrealtime(); }
// per-block stamps go to the block's own row (plain stores, no contended atomics); the host reduces rows
// (min for 0/4/19, max otherwise).  Row 0 holds the single-writer stamps (top / final waves).
__device__ __forceinline__ void stamp_min(uint64_t* st, int idx, uint64_t t) {
  if (st) st[(size_t)(1 + blockIdx.x) * kStamps + idx] = t;
}
__device__ __forceinline__ void stamp_max(uint64_t* st, int idx, uint64_t t) {
  if (st) st[(size_t)(1 + blockIdx.x) * kStamps + idx] = t;
}

}  // namespace pfmpe
