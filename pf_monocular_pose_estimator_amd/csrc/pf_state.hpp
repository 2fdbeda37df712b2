// pf_state.hpp — scalar helpers, pose algebra, particle state load / store and the motion model.
#pragma once
#include <hip/hip_fp16.h>
#include <math.h>

#include <type_traits>

#include "pf_rng.hpp"
#include "pf_types.hpp"

namespace pfmpe {

// ----------------------------------------------------------------------------- scalar helpers
__host__ __device__ __forceinline__ float fmadd(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
// fp64: deliberately UNFUSED (TU built with -ffp-contract=off): a*b rounded, then +c rounded, the
// reference's x86-64 arithmetic.
__host__ __device__ __forceinline__ double fmadd(double a, double b, double c) { return a * b + c; }
// fp32: the motion noise angles are tiny (|x| <= 0.015 * 1.x rad with README parameters), so a short
// Taylor polynomial is accurate to float rounding there; larger angles take sincosf.
__device__ __forceinline__ void sincos_t(float x, float* s, float* c) {
  if (fabsf(x) <= 0.25f) {
    const float x2 = x * x;
    *s = x * fmadd(x2, fmadd(x2, fmadd(x2, fmadd(x2, 1.0f / 362880.0f, -1.0f / 5040.0f), 1.0f / 120.0f),
                             -1.0f / 6.0f), 1.0f);
    *c = fmadd(x2, fmadd(x2, fmadd(x2, fmadd(x2, 1.0f / 40320.0f, -1.0f / 720.0f), 1.0f / 24.0f), -0.5f), 1.0f);
  } else {
    sincosf(x, s, c);
  }
}
// |x| <= kSmallAngle (the host proves it for every angle draw of a frame: FrameArgsT::small_angles): the
// next Taylor terms are below half an fp32 ulp there (x^5/120 / x <= 6.8e-9, x^6/720 <= 1e-12)
constexpr float kSmallAngle = 0.03f;
__device__ __forceinline__ void sincos_small(float x, float* s, float* c) {
  const float x2 = x * x;
  *s = x * fmadd(x2, -1.0f / 6.0f, 1.0f);
  *c = fmadd(x2, fmadd(x2, 1.0f / 24.0f, -0.5f), 1.0f);
}
__device__ __forceinline__ void sincos_t(double x, double* s, double* c) {
  *s = sin(x);
  *c = cos(x);
}
__device__ __forceinline__ void sincos_small(double x, double* s, double* c) { sincos_t(x, s, c); }  // fp64: exact path
// fp32: the hardware square root (v_sqrt_f32, 1 ulp) instead of sqrtf's correctly rounded 14-instruction
// sequence (tolerance path, like div_t); fp64 stays IEEE
// max / min for the wave extrema (operands are never NaN: weights are finite, identities are +-inf)
__device__ __forceinline__ float fmax_t(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ double fmax_t(double a, double b) { return __builtin_fmax(a, b); }
__device__ __forceinline__ float fmin_t(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ double fmin_t(double a, double b) { return __builtin_fmin(a, b); }
__device__ __forceinline__ float sqrt_t(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ double sqrt_t(double x) { return sqrt(x); }
// fp32 quotient a/b through the hardware reciprocal (v_rcp_f32, 1 ulp): one instruction instead of the
// ~10-instruction IEEE division sequence; the fp32 path is a tolerance path, fp64 divides
// exactly
__device__ __forceinline__ float rcp_t(float b) { return __builtin_amdgcn_rcpf(b); }
__device__ __forceinline__ float div_t(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
__device__ __forceinline__ double div_t(double a, double b) { return a / b; }
// perspective division: fp32 uses one hardware reciprocal, fp64 the exact IEEE quotient (PE:1032)
__device__ __forceinline__ void persp(float p0, float p1, float p2, float* u, float* v) {
  const float r = rcp_t(p2);
  *u = p0 * r;
  *v = p1 * r;
}
__device__ __forceinline__ void persp(double p0, double p1, double p2, double* u, double* v) {
  *u = p0 / p2;
  *v = p1 / p2;
}
template <typename T>
__device__ __forceinline__ T inf_t() {
  return (T)INFINITY;
}

// The frame-constant arrays lead FrameArgsT in exactly LdsConst's layout, and FrameArgsT is every
// kernel's first argument, so the block copies them from the kernarg segment with one vector load per
// lane (no SGPR round trip: kept in SGPRs they spill into VGPR lanes).  Callers barrier afterwards.
template <typename T>
__device__ __forceinline__ void stage_consts_from(const uint32_t* src, LdsConst<T>& sc) {
  static_assert(offsetof(FrameArgsT<T>, cur) == 0 && offsetof(FrameArgsT<T>, hi) == offsetof(LdsConst<T>, hi) &&
                    offsetof(FrameArgsT<T>, rgs) == offsetof(LdsConst<T>, rgs),
                "LdsConst must mirror the head of FrameArgsT");
  static_assert(sizeof(LdsConst<T>) % 4 == 0, "dword copy");
  uint32_t* dst = (uint32_t*)&sc;
  constexpr int kWordsC = (int)(sizeof(LdsConst<T>) / 4);
  for (int i = threadIdx.x; i < kWordsC; i += kBlock) dst[i] = src[i];
}
template <typename T>
__device__ __forceinline__ void stage_consts(const FrameArgsT<T>& fa, LdsConst<T>& sc) {
  (void)fa;
  stage_consts_from<T>((const uint32_t*)__builtin_amdgcn_kernarg_segment_ptr(), sc);
}

// ----------------------------------------------------------------------------- pose algebra
// 3x4 affine compose C = A*B with the reference's full-4x4 summation order (k = 0..3 sequential; the
// zero bottom-row terms add +0 and are skipped without changing any non-zero value).
template <typename T>
__host__ __device__ __forceinline__ void compose(const T* A, const T* B, T* C) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      T s = A[i * 4 + 0] * B[0 * 4 + j];
      s = fmadd(A[i * 4 + 1], B[1 * 4 + j], s);
      s = fmadd(A[i * 4 + 2], B[2 * 4 + j], s);
      if (j == 3) s = s + A[i * 4 + 3];
      C[i * 4 + j] = s;
    }
  }
}

typedef float f32x2 __attribute__((ext_vector_type(2)));  // packed fp32 pairs (v_pk_* forms)
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));  // one 16-byte load or store

// Particle state storage S for compute type T: S == T (fp32 / fp64 planes), or fp16 planes holding
// deltas to the set's anchor pose (PFMPE_STATE_F16, fp32 compute): 24 B per particle.
template <typename T, typename SP>
struct StateIO {
  static __host__ __device__ __forceinline__ T load(SP v, T) { return (T)v; }
  static __host__ __device__ __forceinline__ SP store(T v, T) { return (SP)v; }
};
template <>
struct StateIO<float, __half> {
  static __device__ __forceinline__ float load(__half v, float anchor) { return __half2float(v) + anchor; }
  static __device__ __forceinline__ __half store(float v, float anchor) { return __float2half(v - anchor); }
};

// SoA plane access through a buffer resource (cdna_hip_programming.md T8) for the fp32 / fp16 planes: every
// plane of particle n is at byte n*sizeof(SP) (one 32-bit VGPR offset shared by all 12 planes) plus the
// wave-uniform plane offset q*ld*sizeof(SP) in the SGPR soffset, so no plane costs a 64-bit VALU address
// (a flat access costs two v_mad_u64_u32 and moves per plane).  The resource covers the 12 planes
// (pfmpe_create caps 12*ld*sizeof(SP) below 4 GiB).  fp64 (the parity mode) keeps flat accesses.
template <typename SP>
struct BufPlanes : std::false_type {};
template <>
struct BufPlanes<float> : std::true_type {};
template <>
struct BufPlanes<__half> : std::true_type {};

template <typename SP>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t plane_rsrc(const SP* base, int64_t ld) {
  const uint32_t bytes = (uint32_t)(12 * ld * (int64_t)sizeof(SP));
  return __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, (int)bytes, 0x00020000);
}
template <typename SP, int POL = 0>
__device__ __forceinline__ SP buf_ld(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
  if constexpr (std::is_same<SP, float>::value)
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, POL));
  else
    return __ushort_as_half(__builtin_amdgcn_raw_buffer_load_b16(r, voff, soff, POL));
}
// cache policy of a vector memory access: 16 = sc1 (a store writes through and drops the line from the XCD's L2)
constexpr int kPolSc1 = 16;
template <int POL = 0>
__device__ __forceinline__ void buf_st(float v, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, voff, soff, POL);
}
template <int POL = 0>
__device__ __forceinline__ void buf_st(__half v, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
  __builtin_amdgcn_raw_buffer_store_b16(__half_as_ushort(v), r, voff, soff, POL);
}

// fp16 state layout (PFMPE_F16_PAIRS, default 1): planes 2j and 2j + 1 interleaved as ONE plane of 32-bit pairs,
// element (q, n) at half index (q >> 1) * 2 ld + 2 n + (q & 1).  Every fp16 state access is then a 4-byte
// access per lane (6 instead of 12 VMEM instructions per particle, 256 B per wave instruction), and the pair is
// the register layout the kernels already use (RawState<__half>, store_state_words_f16).  0 keeps 12 planes of
// halves (A/B).  fp32 / fp64 planes are unchanged.
// fp32 state keeps 12 plain planes.  Round 3 also tried 6 planes of 64-bit pairs (PFMPE_F32_PAIRS): -2 us on C5's
// k_resample, +1..5 us on C3's weighing; round 4 removed it: deferred resampling (k_resample writes owner indices,
// no state planes) took away the only kernel it helped.
#ifndef PFMPE_F16_PAIRS
#define PFMPE_F16_PAIRS 1
#endif
template <typename SP>
__host__ __device__ __forceinline__ constexpr bool f16_pairs() {
  return std::is_same<SP, __half>::value && PFMPE_F16_PAIRS != 0;
}
template <typename SP>
__host__ __device__ __forceinline__ int64_t plane_index(int q, int64_t n, int64_t ld) {
  if constexpr (f16_pairs<SP>())
    return (int64_t)(q >> 1) * 2 * ld + 2 * n + (q & 1);
  else
    return (int64_t)q * ld + n;
}

// the 12 state values of particle n of a state buffer (raw SP values, no anchor / conversion).  POL kPolSc1: the
// loads bypass L1
template <typename SP, int POL = 0>
__device__ __forceinline__ void load_state_raw(const SP* __restrict__ base, int64_t ld, int n, SP* v) {
  if constexpr (f16_pairs<SP>()) {
    const __amdgpu_buffer_rsrc_t r = plane_rsrc(base, ld);
    const uint32_t pps = (uint32_t)(ld * 4);
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      const uint32_t w = __builtin_amdgcn_raw_buffer_load_b32(r, (uint32_t)n * 4u, (uint32_t)p * pps, POL);
      v[2 * p] = __ushort_as_half((unsigned short)(w & 0xffffu));
      v[2 * p + 1] = __ushort_as_half((unsigned short)(w >> 16));
    }
  } else if constexpr (BufPlanes<SP>::value) {
    const __amdgpu_buffer_rsrc_t r = plane_rsrc(base, ld);
    const uint32_t ps = (uint32_t)(ld * (int64_t)sizeof(SP));
#pragma unroll
    for (int q = 0; q < 12; ++q) v[q] = buf_ld<SP, POL>(r, (uint32_t)n * (uint32_t)sizeof(SP), (uint32_t)q * ps);
  } else if constexpr (POL != 0) {
#pragma unroll
    for (int q = 0; q < 12; ++q)
      v[q] = __hip_atomic_load((const __attribute__((address_space(1))) SP*)(base + (int64_t)q * ld + n),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
#pragma unroll
    for (int q = 0; q < 12; ++q) v[q] = base[(int64_t)q * ld + n];
  }
}
// store 12 raw state values as particle k
template <typename SP>
__device__ __forceinline__ void store_state_raw(SP* __restrict__ base, int64_t ld, int k, const SP* v) {
  constexpr int pol = 0;
  if constexpr (f16_pairs<SP>()) {
    const __amdgpu_buffer_rsrc_t r = plane_rsrc((const SP*)base, ld);
    const uint32_t pps = (uint32_t)(ld * 4);
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      const uint32_t w = (uint32_t)__half_as_ushort(v[2 * p]) | ((uint32_t)__half_as_ushort(v[2 * p + 1]) << 16);
      __builtin_amdgcn_raw_buffer_store_b32(w, r, (uint32_t)k * 4u, (uint32_t)p * pps, pol);
    }
  } else if constexpr (BufPlanes<SP>::value) {
    const __amdgpu_buffer_rsrc_t r = plane_rsrc((const SP*)base, ld);
    const uint32_t ps = (uint32_t)(ld * (int64_t)sizeof(SP));
#pragma unroll
    for (int q = 0; q < 12; ++q) buf_st<pol>(v[q], r, (uint32_t)k * (uint32_t)sizeof(SP), (uint32_t)q * ps);
  } else {
#pragma unroll
    for (int q = 0; q < 12; ++q) base[(int64_t)q * ld + k] = v[q];
  }
}

// fp16 planes, particle k from six words holding planes (2j, 2j + 1) in their (low, high) halves: the high half
// goes out through buffer_store_short_d16_hi, so no word is shifted first (the compiler does not select the
// _d16_hi form for a store of x >> 16).  A vector store; the "memory" clobber keeps it ordered with the
// compiler's own memory operations, and it carries its own VALU-SGPR-write -> VMEM wait states (below).
__device__ __forceinline__ void store_state_words_f16(__half* __restrict__ base, int64_t ld, int k, const uint32_t* w) {
  const __amdgpu_buffer_rsrc_t r = plane_rsrc((const __half*)base, ld);
  if constexpr (f16_pairs<__half>()) {  // the words are the layout: one dword store each
    const uint32_t pps = (uint32_t)(ld * 4);
#pragma unroll
    for (int j = 0; j < 6; ++j) __builtin_amdgcn_raw_buffer_store_b32(w[j], r, (uint32_t)k * 4u, (uint32_t)j * pps, 0);
    return;
  }
  const uint32_t ps = (uint32_t)(ld * (int64_t)sizeof(__half));
  const uint32_t voff = (uint32_t)k * 2u;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    __builtin_amdgcn_raw_buffer_store_b16((uint16_t)w[j], r, voff, (uint32_t)(2 * j) * ps, 0);
    // s_nop 4 first: the compiler's hazard recognizer does not look inside inline asm, and the soffset /
    // resource SGPRs may have just been written by a VALU (v_readlane of a spilled SGPR), which a VMEM
    // instruction may read only 5 wait states later; without it the store used the stale offset
    asm volatile("s_nop 4\n\tbuffer_store_short_d16_hi %0, %1, %2, %3 offen" ::"v"(w[j]), "v"(voff), "s"(r),
                 "s"((uint32_t)(2 * j + 1) * ps)
                 : "memory");
  }
}

// Prefetch form (k_weigh_stream): the 12 raw plane words of particle n as 32-bit registers (fp16 values
// zero-extended), loaded by every lane without a branch.  The caller clamps the particle index into [0, N) for
// lanes past N (in_planes): the buffer resource's range check covers the VGPR offset only, not the plane offset
// in soffset, so an unclamped lane past ld read past the end of the allocation (up to a plane beyond it for the
// streaming pass's last prefetch); the loaded values of such lanes are never used.  Raw halves kept as halves were packed in pairs by the compiler right after the loads
// (v_perm), which waited for the prefetch at once; a branch around the loads made the next wait vmcnt(0).
// fp64 planes (flat accesses) keep the guarded load.
// fp16 planes: planes 2k and 2k + 1 share one register: one dword load from the pair plane (PFMPE_F16_PAIRS),
// or buffer_load_short_d16 / _d16_hi into its two halves (12 half planes), so the pair needs no packing.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
template <typename SP>
struct RawState {
  SP v[12];
};
template <>
struct RawState<__half> {
  u16x2 p[6];
};
template <>
struct RawState<float> {
  uint32_t v[12];
};
// a particle index every plane access may use: n for n < N, else N - 1 (one v_min; see load_state_prefetch)
__device__ __forceinline__ int in_planes(int n, int N) { return (int)min((unsigned)n, (unsigned)(N - 1)); }
template <typename SP>
__device__ __forceinline__ void load_state_prefetch(const SP* __restrict__ base, int64_t ld, int n, bool want,
                                                    RawState<SP>& R) {
  if constexpr (BufPlanes<SP>::value) {
    const __amdgpu_buffer_rsrc_t r = plane_rsrc(base, ld);
    const uint32_t ps = (uint32_t)(ld * (int64_t)sizeof(SP));
    if constexpr (f16_pairs<SP>()) {  // one dword per pair plane
#pragma unroll
      for (int k = 0; k < 6; ++k)
        R.p[k] = __builtin_bit_cast(u16x2, __builtin_amdgcn_raw_buffer_load_b32(r, (uint32_t)n * 4u, (uint32_t)k * (uint32_t)(ld * 4), 0));
    } else if constexpr (sizeof(SP) == 2) {
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        u16x2 x = R.p[k];
        x.x = __builtin_amdgcn_raw_buffer_load_b16(r, (uint32_t)n * 2u, (uint32_t)(2 * k) * ps, 0);
        x.y = __builtin_amdgcn_raw_buffer_load_b16(r, (uint32_t)n * 2u, (uint32_t)(2 * k + 1) * ps, 0);
        R.p[k] = x;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 12; ++q) R.v[q] = __builtin_amdgcn_raw_buffer_load_b32(r, (uint32_t)n * 4u, (uint32_t)q * ps, 0);
    }
  } else {
    if (want) load_state_raw<SP>(base, ld, n, R.v);
  }
}
// StateIO::load of prefetched plane q
template <typename T, typename SP>
__device__ __forceinline__ T state_from_raw(const RawState<SP>& R, int q, T anchor) {
  if constexpr (std::is_same<SP, __half>::value)
    return StateIO<T, SP>::load(__ushort_as_half((q & 1) ? R.p[q >> 1].y : R.p[q >> 1].x), anchor);
  else if constexpr (std::is_same<SP, float>::value)
    return StateIO<T, SP>::load(__uint_as_float(R.v[q]), anchor);
  else
    return StateIO<T, SP>::load(R.v[q], anchor);
}

// prior particle n (SoA planes), loaded ahead of use so the loads overlap other work
// the stored row of prior particle n (deferred prior: its owner index)
template <typename T>
__device__ __forceinline__ int prior_row(const FrameArgsT<T>& fa, int n) {
  return fa.owner ? (int)fa.owner[n] : n;
}
template <typename T, typename SP, int POL = 0>
__device__ __forceinline__ void load_prior(const FrameArgsT<T>& fa, const SP* __restrict__ prior, int n, T* A) {
  SP v[12];
  load_state_raw<SP, POL>(prior, fa.ld, prior_row(fa, n), v);
#pragma unroll
  for (int q = 0; q < 12; ++q) A[q] = StateIO<T, SP>::load(v[q], fa.anc_in[q]);
}
// particle k of a state buffer from its pose P (quantised against the anchor `anc` for fp16 state)
template <typename T, typename SP>
__device__ __forceinline__ void store_pose(SP* __restrict__ dst, int64_t ld, int k, const T* P, const T* anc) {
  if constexpr (std::is_same<SP, __half>::value && std::is_same<T, float>::value) {
    // fp16 deltas two planes at a time: one v_pk_add_f32 (the same fp32 subtractions) and one v_cvt_pk_f16_f32
    // (round to nearest even, as __float2half) per pair, then the pair's halves as planes 2j / 2j + 1
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    uint32_t w[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const f32x2 d = f32x2{P[2 * j], P[2 * j + 1]} - f32x2{anc[2 * j], anc[2 * j + 1]};
      w[j] = __builtin_bit_cast(uint32_t, __builtin_convertvector(d, f16x2));
    }
    store_state_words_f16(dst, ld, k, w);
    return;
  }
  SP v[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) v[q] = StateIO<T, SP>::store(P[q], anc[q]);
  store_state_raw<SP>(dst, ld, k, v);
}

// The motion model (PE:543-588) for particle n in PF iteration `iter` from its prior pose A (loaded by
// load_prior; unused for n < 2); P receives the 3x4 pose.
template <typename T>
__device__ __forceinline__ T u21_t(uint32_t v);
template <>
__device__ __forceinline__ float u21_t<float>(uint32_t v) { return u21f(v); }
template <>
__device__ __forceinline__ double u21_t<double>(uint32_t v) { return u21d(v); }

template <typename T, int RNG>
__device__ __forceinline__ void propagate(const FrameArgsT<T>& fa, const LdsConst<T>& sc, const T* A_in, int n,
                                          int iter, T* P) {
  if (n == 0) {  // current_pose_ (PE:547)
#pragma unroll
    for (int q = 0; q < 12; ++q) P[q] = sc.cur[q];
    return;
  }
  if (n == 1) {  // predicted_pose_ (PE:551)
#pragma unroll
    for (int q = 0; q < 12; ++q) P[q] = sc.pred[q];
    return;
  }
  T A[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) A[q] = A_in[q];
  if (fa.it > 1) {
    if (!fa.cam_identity) {  // camMoveInv * prior (PE:556-558)
      T X[12];
      compose(sc.cam, A, X);
#pragma unroll
      for (int q = 0; q < 12; ++q) A[q] = X[q];
    }
    if ((iter % 10) != 0) {  // ... * predictionMatrix (PE:556)
      T X[12];
      compose(A, sc.predm, X);
#pragma unroll
      for (int q = 0; q < 12; ++q) A[q] = X[q];
    }
  }
  // draws in reference order: angX, angY, angZ, tX, tY, tZ (PE:563-587)
  const double gd = 1.0 + fa.growth * (double)(iter / 10);
  T d[6];
  if (RNG == kRngReference) {
    const uint64_t before = 12u * ((uint64_t)(fa.N - 2) * (uint64_t)iter + (uint64_t)(n - 2));
    uint32_t g = lcg_output(fa.lcg_x0, before + 1u);
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const uint32_t g1 = g;
      const uint32_t g2 = lcg_next(g1);
      g = lcg_next(g2);
      d[q] = (T)(ref_uniform(ref_canonical(g1, g2), fa.dlo[q], fa.dhi[q]) * gd);
    }
  } else {
    const Draws6 r = philox_motion6((uint32_t)n, (uint32_t)iter, fa.flo, fa.fhi, fa.key0, fa.key1);
    // draw = u21 * (hi - lo) + lo, u21 = v * 2^-21 (exact): v * rgs is the same product rounded once, so the
    // conversion's scaling multiply is folded into the host constant
#pragma unroll
    for (int q = 0; q < 6; ++q) d[q] = (T)r.v[q] * sc.rgs[q] + sc.lo[q];
    if (iter >= 10) {  // wave-uniform: the growth factor 1 + growth * (iter / 10) is exactly 1 before iteration 10
      // (the empty asm keeps this a scalar branch: if-converted, every frame paid the six products and six
      // v_cndmask selects)
      asm volatile("");
      const T g = (T)gd;
#pragma unroll
      for (int q = 0; q < 6; ++q) d[q] = d[q] * g;
    }
  }
  T sa, ca, sb, cb, sz, cz;
  if (fa.small_angles) {  // wave-uniform (fp32 only: the host never sets it for fp64)
    sincos_small(d[0], &sa, &ca);
    sincos_small(d[1], &sb, &cb);
    sincos_small(d[2], &sz, &cz);
  } else {
    sincos_t(d[0], &sa, &ca);
    sincos_t(d[1], &sb, &cb);
    sincos_t(d[2], &sz, &cz);
  }
  // R = ((R_A * Rz(c)) * Ry(b)) * Rx(a)   (PE:582)
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const T a0 = A[i * 4 + 0], a1 = A[i * 4 + 1], a2 = A[i * 4 + 2];
    const T z0 = fmadd(a1, sz, a0 * cz);      // A*Rz col 0
    const T z1 = fmadd(a1, cz, a0 * (-sz));   // A*Rz col 1
    const T y0 = fmadd(a2, (-sb), z0 * cb);   // *Ry col 0
    const T y2 = fmadd(a2, cb, z0 * sb);      // *Ry col 2
    const T x1 = fmadd(y2, sa, z1 * ca);      // *Rx col 1
    const T x2 = fmadd(y2, ca, z1 * (-sa));   // *Rx col 2
    P[i * 4 + 0] = y0;
    P[i * 4 + 1] = x1;
    P[i * 4 + 2] = x2;
    P[i * 4 + 3] = A[i * 4 + 3] + d[3 + i];   // translation added unrotated (PE:585-587)
  }
}

template <typename T, int RNG, typename SP>
__device__ __forceinline__ void make_particle(const FrameArgsT<T>& fa, const LdsConst<T>& sc,
                                              const SP* __restrict__ prior, int n, int iter, T* P) {
  T A[12];
  if (n >= 2) load_prior(fa, prior, n, A);
  propagate<T, RNG>(fa, sc, A, n, iter, P);
}

// Q = K * P (3x4).  fp32 with an upper-triangular K whose last row is (0 0 1) (every pinhole CameraInfo,
// README.md:95-143; the host checks, FrameArgsT::k_upper): the zero terms are skipped, 16 instead of 36
// operations.  A skipped term is an exact +-0 added before the first rounding, so the sums are the same
// except for the sign of an exact zero.  fp64 (the parity mode) keeps the literal form.
// fp32 pairs for the packed VALU forms (v_pk_mul_f32 / v_pk_fma_f32 / v_pk_add_f32: two fp32 operations per
// instruction).  Each lane of a pair sees exactly the scalar operation sequence (mul, fma, add rounded the
// same way; the TUs are built with -ffp-contract=off, so nothing else fuses), so packed and scalar forms
// give the same bits.
// a * b + c for 0 <= a, b < 2^24: one full-rate v_mad_u32_u24 (v_mul_lo_u32 is quarter rate)
__device__ __forceinline__ int mad24(int a, int b, int c) {
  return (int)(((unsigned)a & 0xffffffu) * ((unsigned)b & 0xffffffu)) + c;
}
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 pk2(float a, float b) { return f32x2{a, b}; }

}  // namespace pfmpe
